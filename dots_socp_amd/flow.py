"""Flow map of a transport: particles traced along the velocity ``E / mu`` (host only, numpy).

``flow_map_host`` is the specification of ``dots_flow_map`` (include/dots_socp_hip.h; csrc/kernels_flow.hip): scalar Python floats
in a fixed order of operations, which the kernel performs in the same order, so that both return the same bits -- as
``cascade.closest_scalar_order`` is for the locate kernel.  It extends what the reference returns (solver_socp.py:855-869, ``mu``
and ``E``): where the mass at a point ends up, and where it is at time t.

``mu`` lives on the intervals and ``E`` on the nodes of the time grid (the staggering of the solver): in interval j a particle moves
with ``0.5 * (E[j] + E[j + 1]) / rho``, ``rho`` the mean of ``mu[j]`` over the vertices of its triangle.  Starts at arbitrary points
of the surface come from ``cascade.locate_device`` (triangle and weights of the closest point); ``vertex_starts`` puts one particle
on every vertex.
"""
from __future__ import annotations

import numpy as np


def triangle_neighbours(triangles):
    """``nbr`` (F, 3) int32: ``nbr[f][k]`` is the triangle across the edge opposite corner k of f -- the edge between
    ``triangles[f][(k + 1) % 3]`` and ``triangles[f][(k + 2) % 3]`` --, -1 on a boundary edge.  Orientation does not matter.
    ``ValueError``: an edge with more than two triangles."""
    t = np.asarray(triangles).astype(np.int64)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("triangle_neighbours: triangles (F, 3) expected")
    a, b = t[:, [1, 2, 0]].reshape(-1), t[:, [2, 0, 1]].reshape(-1)      # entry 3 f + k: the edge opposite corner k of f
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    order = np.lexsort((hi, lo))
    same = (lo[order][1:] == lo[order][:-1]) & (hi[order][1:] == hi[order][:-1])      # neighbours in the sorted list on one edge
    if np.any(same[1:] & same[:-1]):
        i = order[int(np.flatnonzero(same[1:] & same[:-1])[0])]
        n = int(np.sum((lo == lo[i]) & (hi == hi[i])))
        raise ValueError(f"triangle_neighbours: the edge ({int(lo[i])}, {int(hi[i])}) belongs to {n} triangles")
    nbr = np.full(t.size, -1, dtype=np.int32)
    first, second = order[:-1][same], order[1:][same]
    nbr[first], nbr[second] = second // 3, first // 3
    return nbr.reshape(t.shape)


def vertex_starts(triangles, n_vertices):
    """``(triangle (V,) int32, weights (V, 3))``: particle i sits at vertex i, in the incident triangle with the smallest index, with
    unit weight on that corner.  ``ValueError``: a vertex without a triangle."""
    t = np.asarray(triangles).astype(np.int64)
    tri = np.full(int(n_vertices), t.shape[0], dtype=np.int32)
    w = np.zeros((int(n_vertices), 3))
    np.minimum.at(tri, t.reshape(-1), np.repeat(np.arange(t.shape[0], dtype=np.int32), 3))
    if np.any(tri == t.shape[0]):
        raise ValueError("vertex_starts: a vertex without a triangle")
    corner = np.argmax(t[tri] == np.arange(int(n_vertices))[:, None], axis=1)
    w[np.arange(int(n_vertices)), corner] = 1.0
    return tri, w


def positions(vertices, triangles, triangle, weights):
    """The points ``(w0 * a + w1 * b) + w2 * c`` of particles ``(triangle (...,), weights (..., 3))`` on the mesh: ``(..., 3)``."""
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles).astype(np.int64)[np.asarray(triangle).astype(np.int64)]
    w = np.asarray(weights, dtype=np.float64)
    return (w[..., 0:1] * v[t[..., 0]] + w[..., 1:2] * v[t[..., 1]]) + w[..., 2:3] * v[t[..., 2]]


def _clamp0(x):
    """``max(x, 0.0)``: a NaN stays a NaN (the kernel's select)."""
    return 0.0 if 0.0 > x else x


def flow_map_host(mu, E, triangles, hat, nbr, start_triangle, start_weights, floor, max_crossings=16, trajectory=False):
    """Trace particles through the transport ``(mu (T, V) on the intervals, E (T + 1, F, 3) on the nodes)`` -- both in the same units,
    the raw iterate or the recovered solution: they share one recovery factor and only their ratio is used.  ``hat`` (F, 3, 3): the
    hat-function gradients of the plan (``DevicePlan.hat_grad`` in the numbering of ``triangles``; the ones the device holds, not
    recomputed); ``nbr``: ``triangle_neighbours(triangles)``.

    A particle is a triangle ``f`` and three weights ``l0, l1, l2``.  With ``h = 1.0 / T``, for the intervals j = 0 .. T - 1 in turn
    every particle that has not stopped starts with ``rem = h`` and ``crossings = 0`` and repeats:

    1. ``rho = ((mu[j][v0] + mu[j][v1]) + mu[j][v2]) * (1.0 / 3.0)`` over the vertices of ``f``;
    2. ``u[c] = (0.5 * (E[j][f][c] + E[j + 1][f][c])) / rho`` if ``rho > floor``, else ``u = 0`` (a NaN compares false);
    3. ``rate[k] = (hat[f][k][0] * u[0] + hat[f][k][1] * u[1]) + hat[f][k][2] * u[2]``: the time derivatives of the weights (only the
       tangential part of ``u`` enters);
    4. ``best = rem``, ``kmin = -1``; for k = 0, 1, 2: if ``rate[k] < 0`` then ``s = l[k] / (-rate[k])``, taken if ``s < best`` (strict:
       the first k wins a tie, an exit exactly at ``rem`` is no exit);
    5. no exit: ``l[k] = max(l[k] + rem * rate[k], 0.0)`` for all k, the interval is done;
    6. exit through corner ``kmin``: ``l[k] = max(l[k] + best * rate[k], 0.0)`` for the other two, ``l[kmin] = 0.0``,
       ``rem = rem - best``, ``g = nbr[f][kmin]``;
    7. ``g < 0``: ``status = 1``, the particle stays where it is for all later intervals;
    8. else ``crossings == max_crossings``: ``rested += 1``, the interval is done (two triangles that push the particle at each other
       across an edge: it rests there until the next interval);
    9. else ``crossings += 1`` and the particle moves to ``g``: each of the two kept weights goes to the corner of ``g`` that names the
       same vertex, the third weight is 0.0.

    The weights are never renormalised.  Returns ``{"triangle" (P,) int32, "weights" (P, 3), "status" (P,) int32, "rested" (P,) int32,
    "crossings" (P,) int32 (the total)}``, with ``trajectory=True`` also ``"triangles_at" (T + 1, P)`` and ``"weights_at" (T + 1, P, 3)``:
    layer 0 is the start, layer l the state after l intervals."""
    mu_a, E_a = np.asarray(mu, dtype=np.float64), np.asarray(E, dtype=np.float64)
    tri_a = np.asarray(triangles).astype(np.int64)
    T, F = mu_a.shape[0], tri_a.shape[0]
    if T < 1 or E_a.shape != (T + 1, F, 3) or np.asarray(hat).shape != (F, 3, 3) or np.asarray(nbr).shape != (F, 3):
        raise ValueError("flow_map_host: mu (T, V), E (T + 1, F, 3), hat (F, 3, 3) and nbr (F, 3) expected")
    if not 1 <= int(max_crossings) <= 255:
        raise ValueError("flow_map_host: max_crossings must be 1 .. 255")
    start_f = np.asarray(start_triangle).astype(np.int64)
    start_w = np.asarray(start_weights, dtype=np.float64)
    P = start_f.shape[0]
    if P < 1 or start_w.shape != (P, 3) or start_f.min() < 0 or start_f.max() >= F:
        raise ValueError("flow_map_host: start_triangle (P,) within the mesh and start_weights (P, 3) expected")
    mu_l, E_l, tri_l = mu_a.tolist(), E_a.tolist(), tri_a.tolist()
    hat_l = np.asarray(hat, dtype=np.float64).tolist()
    nbr_l = np.asarray(nbr).astype(np.int64).tolist()
    floor, max_crossings = float(floor), int(max_crossings)
    h = 1.0 / T
    third = 1.0 / 3.0
    out = {"triangle": np.empty(P, dtype=np.int32), "weights": np.empty((P, 3)), "status": np.empty(P, dtype=np.int32),
           "rested": np.empty(P, dtype=np.int32), "crossings": np.empty(P, dtype=np.int32)}
    if trajectory:
        out["triangles_at"] = np.empty((T + 1, P), dtype=np.int32)
        out["weights_at"] = np.empty((T + 1, P, 3))
    for p in range(P):
        f = int(start_f[p])
        l = start_w[p].tolist()
        status = rested = total = 0
        if trajectory:
            out["triangles_at"][0, p], out["weights_at"][0, p] = f, l
        for j in range(T):
            if status == 0:
                rem, crossings = h, 0
                mu_j, E_j, E_n = mu_l[j], E_l[j], E_l[j + 1]
                while True:
                    v = tri_l[f]
                    rho = ((mu_j[v[0]] + mu_j[v[1]]) + mu_j[v[2]]) * third
                    if rho > floor:
                        e0, e1 = E_j[f], E_n[f]
                        u0, u1, u2 = (0.5 * (e0[0] + e1[0])) / rho, (0.5 * (e0[1] + e1[1])) / rho, (0.5 * (e0[2] + e1[2])) / rho
                    else:
                        u0 = u1 = u2 = 0.0
                    g = hat_l[f]
                    rate = [(g[k][0] * u0 + g[k][1] * u1) + g[k][2] * u2 for k in range(3)]
                    best, kmin = rem, -1
                    for k in range(3):
                        if rate[k] < 0.0:
                            s = l[k] / (-rate[k])
                            if s < best:
                                best, kmin = s, k
                    if kmin < 0:
                        l = [_clamp0(l[k] + rem * rate[k]) for k in range(3)]
                        break
                    l = [0.0 if k == kmin else _clamp0(l[k] + best * rate[k]) for k in range(3)]
                    rem = rem - best
                    g = nbr_l[f][kmin]
                    if g < 0:
                        status = 1
                        break
                    if crossings == max_crossings:
                        rested += 1
                        break
                    crossings += 1
                    total += 1
                    moved = [0.0, 0.0, 0.0]
                    for k in ((kmin + 1) % 3, (kmin + 2) % 3):
                        moved[tri_l[g].index(v[k])] = l[k]
                    f, l = g, moved
            if trajectory:
                out["triangles_at"][j + 1, p], out["weights_at"][j + 1, p] = f, l
        out["triangle"][p], out["weights"][p], out["status"][p], out["rested"][p], out["crossings"][p] = f, l, status, rested, total
    return out

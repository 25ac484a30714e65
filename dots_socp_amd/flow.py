"""Flow map of a transport: particles traced along the velocity ``E / mu`` (host only, numpy).

``flow_map_host`` is the specification of ``dots_flow_map`` (include/dots_socp_hip.h; csrc/kernels_flow.hip): scalar Python floats
in a fixed order of operations, which the kernel performs in the same order, so that both return the same bits -- as
``cascade.closest_scalar_order`` is for the locate kernel.  It extends what the reference returns (solver_socp.py:855-869, ``mu``
and ``E``): where the mass at a point ends up, and where it is at time t.

``mu`` lives on the intervals and ``E`` on the nodes of the time grid (the staggering of the solver): in interval j a particle moves
with ``0.5 * (E[j] + E[j + 1]) / rho``, ``rho`` the mean of ``mu[j]`` over the vertices of its triangle.  Starts at arbitrary points
of the surface come from ``cascade.locate_device`` (triangle and weights of the closest point); ``vertex_starts`` puts one particle
on every vertex, ``triangle_starts`` one on every sub-triangle of a regular subdivision.

With ``span=(node_from, node_to)`` and ``action=True`` the same function is the specification of ``dots_flow_trace``: the trace between
any two time nodes, backward with the velocity negated (the inverse map: a source point for every start on the target, which
``pull_back`` turns into a texture pull), and the kinetic action of every particle.

With ``slide=True`` and the triangle ``areas`` it is the specification of ``dots_flow_slide``: on an edge where two neighbouring
triangles push a particle at each other it moves along the edge (the sliding mode of the discontinuous field) instead of resting.

``push_forward_host`` is the specification of ``dots_flow_push``: what the particles carry (``start_masses``, attributes) summed onto
the vertices in 64-bit fixed point with the exponents of ``push_scales`` -- integer sums, so the device returns the same bits in
every order of arrival.
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


def check_span(span, n_time=None, who="flow_map"):
    """``(node_from, node_to)`` as two ints: two different integers >= 0, and <= ``n_time`` where it is known.  ``ValueError`` otherwise."""
    ok = isinstance(span, (tuple, list)) and len(span) == 2 and all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in span)
    if not ok:
        raise ValueError(f"{who}: span must be None or (node_from, node_to), two integers")
    a, b = int(span[0]), int(span[1])
    if a == b:
        raise ValueError(f"{who}: span: node_from equals node_to ({a}): no interval to trace")
    if min(a, b) < 0 or (n_time is not None and max(a, b) > int(n_time)):
        raise ValueError(f"{who}: span {(a, b)} outside the time nodes 0 .. {'n_time' if n_time is None else int(n_time)}")
    return a, b


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


SLIDE_ENDS = ("done", "passed_on", "vertex_rest", "cap")      # how a slide ends (the keys of ``tally`` of flow_map_host)


def flow_map_host(mu, E, triangles, hat, nbr, start_triangle, start_weights, floor, max_crossings=16, trajectory=False, span=None, action=False,
                  slide=False, areas=None, tally=None):
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
    layer 0 is the start, layer l the state after l intervals.

    ``span = (node_from, node_to)``, two different nodes of 0 .. T (the specification of ``dots_flow_trace``; None: the above, bit for
    bit): n = |node_to - node_from| intervals are traversed, forward (node_to > node_from) ``j = node_from + i``, backward
    ``j = node_from - 1 - i``, i = 0 .. n - 1.  The steps are the ones above in the interval j, except that backward step 2 negates the
    quotient, ``u[c] = -((0.5 * (E[j][f][c] + E[j + 1][f][c])) / rho)`` (a floored triangle has ``u = +0.0`` in both directions).
    Layer i is the state after i traversed intervals: n + 1 layers.

    ``action=True``: every particle starts with ``act = 0.0``, and after step 4 has found ``best``, once per turn of the inner loop,
    ``uu = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]`` and ``act = act + best * uu`` (a step that ends in a stop or a rest has still
    spent ``best``; ``u`` as formed, nothing projected): the time integral of |u|^2 along the path, ``"action"`` (P,) of the result.
    Its mass-weighted sum is twice the transport cost the particles account for.

    ``slide=True`` with ``areas`` (F,), the triangle areas of the plan (the specification of ``dots_flow_slide``; False: the above, bit
    for bit): the sliding mode of the discontinuous velocity field.  Where the triangle a particle has just entered pushes it back
    across the edge it came through, it moves ALONG that edge with the convex combination of the two velocities whose normal
    component vanishes (Filippov), instead of crossing back and forth until the cap.  ``dot(a, b) = (a[0] * b[0] + a[1] * b[1]) +
    a[2] * b[2]``.  Every interval starts with ``ent = -1``.  Step 9 saves, before ``f`` and ``l`` are replaced, with
    ``ka = (kmin + 1) % 3``:

    - ``hh = dot(hat[f][kmin], hat[f][kmin])``, ``ah = dot(hat[f][ka], hat[f][kmin])``,
      ``sP = rate[ka] - (ah / hh) * rate[kmin]`` (the rate of the weight of the vertex at corner ka with u projected onto the edge),
      ``mP = (-rate[kmin]) * areas[f]`` (proportional to the speed at which f pushes across the edge);
    - ``ca``, ``cb``: the corners of g that name the vertices of corners ka and (kmin + 2) % 3 of f, and ``ent = 3 - ca - cb``, the
      corner of g opposite the edge just crossed.

    Step 3a, after the rates of a turn are formed, applies if ``ent >= 0 and rate[ent] < 0.0`` (g pushes back), with ``c = ent`` and
    f now being g:

    - ``cc = dot(hat[f][c], hat[f][c])``, ``ac = dot(hat[f][ca], hat[f][c])``, ``sG = rate[ca] - (ac / cc) * rate[c]``,
      ``mG = (-rate[c]) * areas[f]``, ``s = (mG * sP + mP * sG) / (mP + mG)`` (each side weighted with the OTHER side's normal speed);
    - ``best = rem``, ``hit = -1``; if ``s > 0.0``: ``tau = l[cb] / s``, taken with ``hit = cb`` if ``tau < best``; else if ``s < 0.0``:
      ``tau = l[ca] / (-s)``, taken with ``hit = ca`` if ``tau < best``;
    - with ``action``: ``aa = dot(hat[f][ca], hat[f][ca])`` and ``act = act + best * ((s * s) * (cc / (aa * cc - ac * ac)))`` (the
      squared length of the edge from the hat gradients);
    - ``l[ca] = max(l[ca] + best * s, 0.0)``, ``l[cb] = max(l[cb] - best * s, 0.0)``, ``l[hit] = 0.0`` if ``hit >= 0``; ``slides += 1``;
    - ``hit < 0``: the interval is done.  Else ``rem = rem - best``; ``crossings == max_crossings``: ``rested += 1``, the interval is
      done; ``rate[hit] < 0.0`` false: ``rested += 1``, the interval is done (the particle is at a vertex and this triangle does not
      pass it on round the fan); else ``crossings += 1`` (it bounds the loop; the total ``"crossings"`` is not incremented: a slide is
      not an edge crossed) and the turn goes on with step 4 with corner c left out of the candidates (it finds ``kmin = hit``,
      ``best = 0.0``).

    ``ent`` is -1 again after the test of step 3a in every turn, taken or not.  A floored triangle has ``rate = 0`` and never slides.
    The result gains ``"slides"`` (P,) int32, the slides of every particle, and ``"steps"`` (P,) int32, the turns of its inner loop.
    ``tally``: a dict which receives, under the keys ``SLIDE_ENDS``, how many slides ended with the interval done, with the vertex
    passing the particle on, with a rest at the vertex and with a rest at the cap (for tests)."""
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
    slide = bool(slide)
    if slide:
        if areas is None or np.asarray(areas).shape != (F,):
            raise ValueError("flow_map_host: slide needs areas (F,), the triangle areas of the plan")
        area_l = np.asarray(areas, dtype=np.float64).tolist()
        if tally is not None:
            for key in SLIDE_ENDS:
                tally.setdefault(key, 0)
    h = 1.0 / T
    third = 1.0 / 3.0
    out = {"triangle": np.empty(P, dtype=np.int32), "weights": np.empty((P, 3)), "status": np.empty(P, dtype=np.int32),
           "rested": np.empty(P, dtype=np.int32), "crossings": np.empty(P, dtype=np.int32)}
    if span is None:
        intervals, backward = range(T), False
    else:
        node_from, node_to = check_span(span, T, "flow_map_host")
        backward = node_to < node_from
        intervals = range(node_from - 1, node_to - 1, -1) if backward else range(node_from, node_to)
    n = len(intervals)
    if trajectory:
        out["triangles_at"] = np.empty((n + 1, P), dtype=np.int32)
        out["weights_at"] = np.empty((n + 1, P, 3))
    if action:
        out["action"] = np.empty(P)
    if slide:
        out["slides"], out["steps"] = np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int32)
    for p in range(P):
        f = int(start_f[p])
        l = start_w[p].tolist()
        status = rested = total = slides = steps = 0
        act = 0.0
        if trajectory:
            out["triangles_at"][0, p], out["weights_at"][0, p] = f, l
        for i, j in enumerate(intervals):
            if status == 0:
                rem, crossings, ent = h, 0, -1
                mu_j, E_j, E_n = mu_l[j], E_l[j], E_l[j + 1]
                while True:
                    v = tri_l[f]
                    rho = ((mu_j[v[0]] + mu_j[v[1]]) + mu_j[v[2]]) * third
                    if rho > floor:
                        e0, e1 = E_j[f], E_n[f]
                        u0, u1, u2 = (0.5 * (e0[0] + e1[0])) / rho, (0.5 * (e0[1] + e1[1])) / rho, (0.5 * (e0[2] + e1[2])) / rho
                        if backward:
                            u0, u1, u2 = -u0, -u1, -u2
                    else:
                        u0 = u1 = u2 = 0.0
                    g = hat_l[f]
                    rate = [(g[k][0] * u0 + g[k][1] * u1) + g[k][2] * u2 for k in range(3)]
                    steps += 1
                    left_out = -1
                    if slide:
                        c, ent = ent, -1
                        if c >= 0 and rate[c] < 0.0:      # step 3a: g pushes back across the edge just crossed
                            cc, ac = _dot(g[c], g[c]), _dot(g[ca], g[c])
                            sG = rate[ca] - (ac / cc) * rate[c]
                            mG = (-rate[c]) * area_l[f]
                            s = (mG * sP + mP * sG) / (mP + mG)
                            best, hit = rem, -1
                            if s > 0.0:
                                tau = l[cb] / s
                                if tau < best:
                                    best, hit = tau, cb
                            elif s < 0.0:
                                tau = l[ca] / (-s)
                                if tau < best:
                                    best, hit = tau, ca
                            if action:
                                aa = _dot(g[ca], g[ca])
                                act = act + best * ((s * s) * (cc / (aa * cc - ac * ac)))
                            l[ca], l[cb] = _clamp0(l[ca] + best * s), _clamp0(l[cb] - best * s)
                            if hit >= 0:
                                l[hit] = 0.0
                            slides += 1
                            if hit < 0:
                                end = "done"
                            else:
                                rem = rem - best
                                if crossings == max_crossings:
                                    rested += 1
                                    end = "cap"
                                elif not rate[hit] < 0.0:
                                    rested += 1
                                    end = "vertex_rest"
                                else:
                                    crossings += 1
                                    left_out = c
                                    end = "passed_on"
                            if tally is not None:
                                tally[end] += 1
                            if left_out < 0:
                                break
                    best, kmin = rem, -1
                    for k in range(3):
                        if k != left_out and rate[k] < 0.0:
                            s = l[k] / (-rate[k])
                            if s < best:
                                best, kmin = s, k
                    if action:
                        act = act + best * ((u0 * u0 + u1 * u1) + u2 * u2)
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
                    if slide:      # what step 3a of the next turn needs of the triangle left
                        ka, hf = (kmin + 1) % 3, hat_l[f]
                        hh, ah = _dot(hf[kmin], hf[kmin]), _dot(hf[ka], hf[kmin])
                        sP = rate[ka] - (ah / hh) * rate[kmin]
                        mP = (-rate[kmin]) * area_l[f]
                        ca, cb = tri_l[g].index(v[ka]), tri_l[g].index(v[(kmin + 2) % 3])
                        ent = 3 - ca - cb
                    f, l = g, moved
            if trajectory:
                out["triangles_at"][i + 1, p], out["weights_at"][i + 1, p] = f, l
        if action:
            out["action"][p] = act
        if slide:
            out["slides"][p], out["steps"][p] = slides, steps
        out["triangle"][p], out["weights"][p], out["status"][p], out["rested"][p], out["crossings"][p] = f, l, status, rested, total
    return out


# ---- push-forward: what the particles carry, summed onto the vertices ------------------------------------------------------------------

PUSH_MAX_ATTRIBUTES = 4
PUSH_EXPONENT_LIMIT = 1000


def _carried(mass, attributes, n_particles):
    """``g`` (1 + A, P): ``g[0] = m`` and ``g[c] = m * a[c - 1]``, one fp64 multiply each."""
    m = np.asarray(mass, dtype=np.float64)
    a = np.zeros((0, n_particles)) if attributes is None else np.asarray(attributes, dtype=np.float64)
    if m.shape != (n_particles,) or a.ndim != 2 or a.shape[1] != n_particles or a.shape[0] > PUSH_MAX_ATTRIBUTES:
        raise ValueError(f"push: mass ({n_particles},) and attributes (A <= {PUSH_MAX_ATTRIBUTES}, {n_particles}) expected, got {m.shape} and {a.shape}")
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.concatenate([m[None, :], m[None, :] * a], axis=0)
    if not np.all(np.isfinite(g)):
        raise ValueError("push: a mass, or a mass times an attribute, that is not finite")
    return g


def push_scales(mass, attributes, start_weights):
    """The exponents ``k_c`` (1 + A,) int32 of ``push_forward_host`` / ``dots_flow_push`` for these particles:
    ``B_c = fsum_p |g[p][c]| * max(1.0, (w0 + w1) + w2)``, ``e_c`` the least integer with ``2^e_c >= B_c``,
    ``k_c = clip(60 - e_c, -1000, 1000)``, and ``k_c = 0`` where ``B_c = 0``.  A vertex sum then stays below 2^60 as long as the weight
    sums stay below 4 times their start (rates sum to zero and the clamps only lift rounding negatives: they do not grow past that
    in practice)."""
    import math

    w = np.asarray(start_weights, dtype=np.float64)
    g = _carried(mass, attributes, w.shape[0])
    wsum = np.maximum(1.0, (w[:, 0] + w[:, 1]) + w[:, 2])
    out = np.zeros(g.shape[0], dtype=np.int32)
    for c in range(g.shape[0]):
        B = math.fsum((np.abs(g[c]) * wsum).tolist())
        if B == 0.0:
            continue
        if not math.isfinite(B):
            raise ValueError("push_scales: the bound of a channel is not finite")
        frac, e = math.frexp(B)      # B = frac * 2^e, 0.5 <= frac < 1
        if frac == 0.5:
            e -= 1
        out[c] = min(max(60 - e, -PUSH_EXPONENT_LIMIT), PUSH_EXPONENT_LIMIT)
    return out


def push_forward_host(result_with_trajectory, triangles, n_vertices, mass, attributes, exponents, layers="end"):
    """The specification of ``dots_flow_push``: what the particles of a traced map carry, summed onto the vertices.

    Channels are ``c = 0`` (mass) and ``c = 1 .. A`` (attributes), with ``0 <= A <= 4``.

    - Particle p carries ``g[p][0] = m[p]`` and ``g[p][c] = m[p] * a[p][c-1]``, one fp64 multiply each.
    - Every ``g`` must be finite.  Signs are free.

    Layers:

    - ``layers="end"`` gives ``L = 1``: the state after interval T.
    - ``layers="all"`` gives ``L = T + 1``: layer 0 the starts, layer l the state after l intervals.  These are the layers of
      ``triangles_at``.
    - A result traced over a ``span`` of n intervals (in either direction) has n + 1 layers: ``"all"`` gives ``L = n + 1``, ``"end"``
      the state at ``node_to``.

    At each layer, for each corner ``k = 0, 1, 2`` of the triangle ``f`` the particle is in and each channel c, in this order of
    operations:

    1. ``x = g[p][c] * l_k`` and ``y = x * scale_c``, where ``scale_c = ldexp(1.0, k_c)`` and ``k_c`` is an int32 the caller passes.
    2. If ``|y| < 2^62`` is false (this includes NaN), the contribution is dropped and counted in one ``dropped`` counter.
    3. Otherwise ``q = rint(y)``, round to nearest even, as int64.  ``acc[c][layer][tri[f][k]] += q`` in two's complement.
    4. A ``q`` of zero issues no atomic.  Vertex starts have two zero weights.

    Stopped (``status 1``) and resting particles keep depositing where they are.  Mass is not lost.

    The result is ``float(acc) * ldexp(1.0, -k_c)``, with int64 -> fp64 rounding to nearest even.  Output arrays are in the caller's
    vertex numbering: ``mass_at [L][V]`` and ``attr_at [A][L][V]``.

    ``result_with_trajectory``: the dict of ``flow_map_host(..., trajectory=True)`` (its ``triangles_at`` and ``weights_at`` are used);
    ``attributes``: None or (A, P).  The sums are formed in Python integers from the two halves of every ``q`` (each half summed in
    int64, which cannot overflow below 2^31 contributions), and ``|sum| < 2^63`` is asserted.  Returns ``{"mass" (L, V), "attributes"
    (A, L, V) or None, "dropped", "integers" (1 + A, L, V) int64: the sums themselves, "issued": the non-zero q}``."""
    import math

    tri_at = np.asarray(result_with_trajectory["triangles_at"]).astype(np.int64)
    w_at = np.asarray(result_with_trajectory["weights_at"], dtype=np.float64)
    if layers not in ("end", "all"):
        raise ValueError("push_forward_host: layers must be 'end' or 'all'")
    if layers == "end":
        tri_at, w_at = tri_at[-1:], w_at[-1:]
    L, P = tri_at.shape
    V = int(n_vertices)
    g = _carried(mass, attributes, P)
    C = g.shape[0]
    k = np.asarray(exponents).astype(np.int64).reshape(-1)
    if k.shape != (C,) or np.any(np.abs(k) > PUSH_EXPONENT_LIMIT):
        raise ValueError(f"push_forward_host: {C} exponents within -{PUSH_EXPONENT_LIMIT} .. {PUSH_EXPONENT_LIMIT} expected")
    vert = np.asarray(triangles).astype(np.int64)[tri_at]      # (L, P, 3)
    hi_sum, lo_sum = np.zeros((C, L, V), dtype=np.int64), np.zeros((C, L, V), dtype=np.int64)
    dropped = issued = 0
    index = (np.arange(L, dtype=np.int64)[:, None, None] * V + vert).reshape(-1)
    for c in range(C):
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            x = g[c][None, :, None] * w_at
            y = x * math.ldexp(1.0, int(k[c]))
            keep = np.abs(y) < 2.0 ** 62      # (False for a NaN)
        dropped += int(keep.size - np.count_nonzero(keep))
        q = np.rint(np.where(keep, y, 0.0)).astype(np.int64)      # (to nearest even; exact: |y| < 2^62)
        issued += int(np.count_nonzero(q))
        np.add.at(hi_sum[c].reshape(-1), index, (q >> 32).reshape(-1))
        np.add.at(lo_sum[c].reshape(-1), index, (q & 0xFFFFFFFF).reshape(-1))
    acc = hi_sum.astype(object) * (1 << 32) + lo_sum.astype(object)      # Python integers
    assert all(abs(s) < 1 << 63 for s in acc.reshape(-1)), "push_forward_host: a sum left the 64-bit range"
    out = np.empty((C, L, V))
    for c in range(C):
        out[c] = acc[c].astype(np.float64) * math.ldexp(1.0, -int(k[c]))      # (float(int) rounds to nearest even)
    return {"mass": out[0], "attributes": out[1:] if C > 1 else None, "dropped": dropped, "integers": acc.astype(np.int64), "issued": issued}


def pull_back(fields, result, triangles):
    """Vertex fields ``(V, A)`` or ``(V,)`` interpolated at the landing points of a traced map: ``(w0 * x[v0] + w1 * x[v1]) + w2 * x[v2]``
    over the vertices of ``result["triangle"]`` with ``result["weights"]``: ``(P, A)`` or ``(P,)``.  With a backward trace from the
    vertices of the target this pulls a texture or a labelling on the source onto every target vertex."""
    x = np.asarray(fields, dtype=np.float64)
    t = np.asarray(triangles).astype(np.int64)[np.asarray(result["triangle"]).astype(np.int64)]      # (P, 3)
    w = np.asarray(result["weights"], dtype=np.float64)
    if x.ndim not in (1, 2) or t.ndim != 2 or w.shape != (t.shape[0], 3):
        raise ValueError("pull_back: fields (V, A) or (V,), and a result with triangle (P,) and weights (P, 3) expected")
    if x.ndim == 1:
        return (w[:, 0] * x[t[:, 0]] + w[:, 1] * x[t[:, 1]]) + w[:, 2] * x[t[:, 2]]
    return (w[:, 0:1] * x[t[:, 0]] + w[:, 1:2] * x[t[:, 1]]) + w[:, 2:3] * x[t[:, 2]]


def triangle_starts(triangles, level=1):
    """``(triangle (F * level^2,) int32, weights (F * level^2, 3))``: every triangle cut into ``level^2`` congruent sub-triangles, one
    particle at the centroid of each (triangle by triangle; the upright sub-triangles of a triangle first, then the inverted ones)."""
    n = int(level)
    if n < 1:
        raise ValueError("triangle_starts: level >= 1 expected")
    F = np.asarray(triangles).shape[0]
    up = [(3 * i + 1, 3 * j + 1) for i in range(n) for j in range(n - i)]
    down = [(3 * i + 2, 3 * j + 2) for i in range(n - 1) for j in range(n - 1 - i)]
    ab = np.array(up + down, dtype=np.int64)
    w = np.stack([ab[:, 0], ab[:, 1], 3 * n - ab[:, 0] - ab[:, 1]], axis=1) / float(3 * n)
    return np.repeat(np.arange(F, dtype=np.int32), n * n), np.ascontiguousarray(np.tile(w, (F, 1)))


def start_masses(mu0, area_vertices, area_triangles, triangles, start_triangle, start_weights, level=None):
    """The mass of ``mu0`` every start carries.  ``level`` (``triangle_starts``): ``m_p = (area_f / level^2) sum_k w_k mu0[v_k] /
    (area_vertices[v_k] / 3)`` -- the density of ``mu0``, linear on the triangle, at the particle, times the area of its sub-triangle:
    the centroid rule is exact for linear functions, so the masses sum to ``sum(mu0)``.  ``level=None`` (``vertex_starts``):
    ``m_v = mu0[v]`` of the corner with the largest weight."""
    m0 = np.asarray(mu0, dtype=np.float64)
    t = np.asarray(triangles).astype(np.int64)[np.asarray(start_triangle).astype(np.int64)]      # (P, 3)
    w = np.asarray(start_weights, dtype=np.float64)
    if level is None:
        return m0[t[np.arange(t.shape[0]), np.argmax(w, axis=1)]]
    rho = m0 / (np.asarray(area_vertices, dtype=np.float64) / 3.0)
    area = np.asarray(area_triangles, dtype=np.float64)[np.asarray(start_triangle).astype(np.int64)]
    return (area / float(int(level) ** 2)) * ((w[:, 0] * rho[t[:, 0]] + w[:, 1] * rho[t[:, 1]]) + w[:, 2] * rho[t[:, 2]])

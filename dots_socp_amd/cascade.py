"""Coarse-to-fine cascades: the transfer of a solution between two time grids, or between two nested meshes, as a specification on
the host.

A solution on a coarse time grid is a good starting point for a finer one (``init_solution``, solver_socp.py:38,70-71).  This
module is the single definition of the interpolation that the device kernel (``dots_prolong_time``, csrc/kernels_carry.hip), the
tests and the oracle-side checks share:

* node arrays (``phi``, ``B``, ``E``; n + 1 entries along the time axis) live at ``t_i = i / n``; interval arrays (``A``,
  ``lambda_c``, ``z_fst``, ``z_end``, ``mu``, ``beta_fst``, ``beta_end``, and ``z_mid`` / ``beta_mid`` along their first axis) at
  the interval centres ``(i + 1/2) / n``;
* a destination time ``td`` takes ``(1 - w) * a[j] + w * a[j + 1]`` with ``j = clip(searchsorted(ts, td, "right") - 1, 0, len(ts) - 2)``
  and ``w = clip((td - ts[j]) / (ts[j + 1] - ts[j]), 0, 1)``: linear inside, constant beyond the first / last source point;
* a single source interval (``n_src = 1``) has one centre only: interval arrays are then constant in time (``j = 0``, ``w = 0``, and
  ``a[j + 1]`` reads ``a[j]``);
* the twelve arrays are interpolated independently (``A`` and ``B`` are not re-derived from ``phi``).

``time_weights`` computes the tables ``j`` and ``w`` once, on the host; the device reads the same tables, so both sides perform the
same operations on the same numbers.

The transfer in space (``prolong_space``; ``dots_prolong_space``, k_carry_space in csrc/kernels_carry.hip) goes from a mesh to its
nested refinement (``meshes.subdivide``: ``parents``) on one time grid; ``space_row_maps`` turns ``parents`` and the two device
numberings into the row maps the kernel reads.

Between two independent triangulations of one surface (no ``parents``) the transfer is barycentric (``transfer_space``;
``dots_transfer_space``, k_carry_space): ``locate`` finds the closest point of the coarse mesh to every fine vertex and triangle
centroid, ``mesh_transfer`` turns that into the tables of the transfer, ``transfer_row_maps`` puts them into the two device numberings.

A step that changes the mesh AND the time grid (``carry_spacetime``; ``dots_carry_spacetime``, k_carry_spacetime) is the composition
of the two: the transfer in space first, then the interpolation in time, with the functions above unchanged.
"""
from __future__ import annotations

import numpy as np

NODE_ARRAYS = ("phi", "B", "E")
INTERVAL_ARRAYS = ("A", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "beta_fst", "beta_mid", "beta_end")
MIN_LEVEL_NODES = 16      # default_levels: n_time + 1 is halved while it stays at least this


def _grid(n, node):
    n = int(n)
    if n < 1:
        raise ValueError(f"a time grid needs at least one interval (got {n})")
    return np.arange(n + 1) / n if node else (np.arange(n) + 0.5) / n


def time_weights(n_src, n_dst, node):
    """The tables ``j[t]`` (int32) and ``w[t]`` (float64) of the interpolation from the grid of ``n_src`` intervals to the one of
    ``n_dst``: ``node`` selects the node grids (n + 1 points) or the interval centres (n points)."""
    ts, td = _grid(n_src, node), _grid(n_dst, node)
    if ts.size == 1:      # one interval centre: constant in time
        return np.zeros(td.size, dtype=np.int32), np.zeros(td.size)
    j = np.clip(np.searchsorted(ts, td, side="right") - 1, 0, ts.size - 2)
    w = np.clip((td - ts[j]) / (ts[j + 1] - ts[j]), 0.0, 1.0)
    return j.astype(np.int32), w.astype(np.float64)


def prolong_time(array, name, n_src, n_dst):
    """``array`` (the state array ``name`` on the grid of ``n_src`` intervals, reference layout: time along axis 0) on the grid of
    ``n_dst`` intervals."""
    if name not in NODE_ARRAYS and name not in INTERVAL_ARRAYS:
        raise ValueError(f"unknown state array {name!r}")
    node = name in NODE_ARRAYS
    a = np.asarray(array, dtype=np.float64)
    n_pts = int(n_src) + 1 if node else int(n_src)
    if a.shape[0] != n_pts:
        raise ValueError(f"{name}: expected {n_pts} entries along the time axis, got {a.shape[0]}")
    j, w = time_weights(n_src, n_dst, node)
    j1 = np.minimum(j + 1, n_pts - 1)
    shp = (-1,) + (1,) * (a.ndim - 1)
    return (1 - w).reshape(shp) * a[j] + w.reshape(shp) * a[j1]


def prolong_solution(solution, n_src, n_dst):
    """Every state array of ``solution`` (a dict as ``solver_socp`` returns it) on the grid of ``n_dst`` intervals: an ``init_solution``."""
    names = NODE_ARRAYS + INTERVAL_ARRAYS
    return {k: prolong_time(v, k, n_src, n_dst) for k, v in solution.items() if k in names and v is not None}


def default_levels(n_time):
    """The levels of a cascade that ends at ``n_time``: ``n_time + 1`` is halved while it is even and the half stays >= 16 nodes
    (1023 -> 15, 31, ..., 1023; 31 -> 15, 31; 20 -> 20 alone: an odd number of nodes is not halved)."""
    nodes = int(n_time) + 1
    levels = [nodes - 1]
    while nodes % 2 == 0 and nodes // 2 >= MIN_LEVEL_NODES:
        nodes //= 2
        levels.append(nodes - 1)
    return levels[::-1]


def check_levels(levels, n_time):
    """The levels as a list of ints: increasing, at least one interval each, ending in ``n_time``."""
    if levels is None:
        return default_levels(n_time)
    try:
        out = [int(x) for x in levels]
    except (TypeError, ValueError):
        raise ValueError("levels must be a list of n_time values") from None
    if not out or any(int(a) != a for a in levels):
        raise ValueError("levels must be a non-empty list of integers")
    if out[0] < 1:
        raise ValueError("levels: every level needs n_time >= 1")
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"levels must increase (got {out})")
    if out[-1] != int(n_time):
        raise ValueError(f"the last level must be n_time = {int(n_time)} (got {out[-1]})")
    return out


def inverse_numbering(perm, n, who):
    """Caller index -> device row for the device numbering ``perm`` of ``n`` rows (``perm[i]`` = caller index of device row i, None =
    identity), int64; ``who`` names the caller in the error for a ``perm`` of another size."""
    if perm is None:
        return np.arange(n, dtype=np.int64)
    perm = np.asarray(perm, dtype=np.int64)
    if perm.shape != (n,):
        raise ValueError(f"{who}: a permutation of the wrong size")
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    return inv


def row_map(perm_dst, perm_src, n):
    """Destination device row -> source device row for two plans of one mesh (``perm[i]`` = caller index of device row i, None =
    identity); None when both numberings agree."""
    if perm_dst is None and perm_src is None:
        return None
    pd = np.arange(n, dtype=np.int64) if perm_dst is None else np.asarray(perm_dst, dtype=np.int64)
    ps = np.arange(n, dtype=np.int64) if perm_src is None else np.asarray(perm_src, dtype=np.int64)
    if np.array_equal(pd, ps):
        return None
    return np.ascontiguousarray(inverse_numbering(perm_src, n, "row_map")[pd], dtype=np.int32)


# ---- coarse-to-fine in space: a mesh to its nested refinement --------------------------------------------------------------------
VERTEX_ARRAYS = ("phi", "A", "lambda_c", "z_fst", "z_end", "mu", "beta_fst", "beta_end")
TRIANGLE_ARRAYS = ("B", "E")
CORNER_ARRAYS = ("z_mid", "beta_mid")
DEFAULT_COARSE_LEVELS = 2      # coarse levels below the finest mesh that paid on the 100k torus; small meshes: solve cold


def check_parents(parents, n_vertices=None, n_triangles=None):
    """``(vertex_parents (Vf, 2), triangle_parent (Ff,))`` of ``parents`` (``meshes.subdivide``) as int64 arrays; ``n_vertices`` /
    ``n_triangles``: the size of the coarse mesh they must refer to (every coarse vertex and triangle has a child)."""
    try:
        vp = np.asarray(parents["vertex_parents"])
        tp = np.asarray(parents["triangle_parent"])
    except (KeyError, TypeError, IndexError):
        raise ValueError("parents must hold 'vertex_parents' and 'triangle_parent' (meshes.subdivide)") from None
    if vp.ndim != 2 or vp.shape[1] != 2 or tp.ndim != 1 or vp.shape[0] < 1 or tp.shape[0] < 1:
        raise ValueError("parents: vertex_parents must be (Vf, 2) and triangle_parent (Ff,)")
    if not (np.issubdtype(vp.dtype, np.integer) and np.issubdtype(tp.dtype, np.integer)):
        raise ValueError("parents: integer arrays expected")
    vp, tp = vp.astype(np.int64), tp.astype(np.int64)
    if vp.min() < 0 or tp.min() < 0:
        raise ValueError("parents: negative index")
    if n_vertices is not None and int(vp.max()) + 1 != int(n_vertices):
        raise ValueError(f"parents: vertex_parents refer to a mesh of {int(vp.max()) + 1} vertices, not {int(n_vertices)}")
    if n_triangles is not None and int(tp.max()) + 1 != int(n_triangles):
        raise ValueError(f"parents: triangle_parent refers to a mesh of {int(tp.max()) + 1} triangles, not {int(n_triangles)}")
    return vp, tp


def prolong_space(array, name, parents):
    """``array`` (the state array ``name`` on the coarse mesh, reference layout) on the refinement that ``parents`` describes; the
    time axis is untouched.

    * vertex arrays (``phi``, ``A``, ``lambda_c``, ``z_fst``, ``z_end``, ``mu``, ``beta_fst``, ``beta_end``): a kept vertex
      (``p0 == p1``) takes ``x[..., p0]``, an exact copy; a midpoint ``(x[..., p0] + x[..., p1]) * 0.5``, in this order of operations;
    * triangle arrays (``B``, ``E``): a child takes the three components of its parent unchanged.  They are NOT projected into the
      child's plane: on a curved surface a child is tilted against its parent, and the small normal component is left to the
      first iterations on the fine mesh;
    * corner arrays (``z_mid``, ``beta_mid``): child ``(f', k)`` takes parent ``(triangle_parent[f'], k)`` for both interval ends
      and every component."""
    a = np.asarray(array, dtype=np.float64)
    if name in VERTEX_ARRAYS:
        if a.ndim != 2:
            raise ValueError(f"{name}: expected (time, V), got shape {a.shape}")
        vp, _ = check_parents(parents, n_vertices=a.shape[-1])
        p0, p1 = vp[:, 0], vp[:, 1]
        return np.where(p0 == p1, a[..., p0], (a[..., p0] + a[..., p1]) * 0.5)
    if name in TRIANGLE_ARRAYS or name in CORNER_ARRAYS:
        if a.ndim != (3 if name in TRIANGLE_ARRAYS else 5) or a.shape[-1] != 3:
            raise ValueError(f"{name}: expected (time, {'' if name in TRIANGLE_ARRAYS else '2, 3, '}F, 3), got shape {a.shape}")
        _, tp = check_parents(parents, n_triangles=a.shape[-2])
        return np.ascontiguousarray(a[..., tp, :])
    raise ValueError(f"unknown state array {name!r}")


def prolong_space_solution(solution, parents):
    """Every state array of ``solution`` (a dict as ``solver_socp`` returns it) on the refinement: an ``init_solution``."""
    names = VERTEX_ARRAYS + TRIANGLE_ARRAYS + CORNER_ARRAYS
    return {k: prolong_space(v, k, parents) for k, v in solution.items() if k in names and v is not None}


def space_row_maps(parents, n_src_vertices, n_src_triangles, perm_vert_dst=None, perm_tri_dst=None, perm_vert_src=None, perm_tri_src=None):
    """The row maps of ``dots_prolong_space``: ``vmap`` (Vf, 2) int32, the two source device rows of every destination device vertex
    row (equal for a kept vertex), and ``fmap`` (Ff,) int32, the source device triangle of every destination device triangle.
    ``perm[i]`` = caller index of device row i (None = identity), as in ``row_map``: the two meshes are numbered independently."""
    vp, tp = check_parents(parents, n_vertices=n_src_vertices, n_triangles=n_src_triangles)

    for perm, n in ((perm_vert_dst, vp.shape[0]), (perm_tri_dst, tp.shape[0])):
        if perm is not None and np.asarray(perm).shape != (n,):
            raise ValueError("space_row_maps: a permutation of the wrong size")
    vd = vp if perm_vert_dst is None else vp[np.asarray(perm_vert_dst, dtype=np.int64)]
    td = tp if perm_tri_dst is None else tp[np.asarray(perm_tri_dst, dtype=np.int64)]
    vmap = inverse_numbering(perm_vert_src, int(n_src_vertices), "space_row_maps")[vd]
    fmap = inverse_numbering(perm_tri_src, int(n_src_triangles), "space_row_maps")[td]
    return np.ascontiguousarray(vmap, dtype=np.int32), np.ascontiguousarray(fmap, dtype=np.int32)


# ---- coarse-to-fine in space between two independent triangulations of one surface -----------------------------------------------
LOCATE_CHUNK = 1 << 16      # points per pass of locate (bounds the candidate arrays)


def closest_on_triangles(p, a, b, c):
    """The closest point to ``p[i]`` on the triangle ``(a[i], b[i], c[i])``, all (N, 3): ``(weights (N, 3), distance (N,))`` with the
    clamped barycentric weights of the corners, all >= 0 and summing to 1.  The region test of Ericson's closest-point-on-triangle
    (Real-Time Collision Detection, 5.1.5), vectorised: vertex regions, edge regions, then the interior."""
    ab, ac, ap = b - a, c - a, p - a
    dot = lambda x, y: np.einsum("ij,ij->i", x, y)      # noqa: E731
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = p - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = p - c
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ab, t_ac = d1 / (d1 - d3), d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = 1.0 / (va + vb + vc)
    v_in, w_in = vb * denom, vc * denom
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    w1 = np.select(conds, [zero, one, t_ab, zero, zero, 1.0 - t_bc], default=v_in)
    w2 = np.select(conds, [zero, zero, zero, one, t_ac, t_bc], default=w_in)
    w1, w2 = np.clip(w1, 0.0, 1.0), np.clip(w2, 0.0, 1.0)
    w0 = np.maximum(1.0 - w1 - w2, 0.0)
    w = np.stack([w0, w1, w2], axis=1)
    q = w0[:, None] * a + w1[:, None] * b + w2[:, None] * c
    return w, np.linalg.norm(p - q, axis=1)


def locate(points, vertices, triangles, k=3):
    """The closest point of the mesh ``(vertices, triangles)`` to every one of ``points``: ``(triangle (N,) int64, weights (N, 3),
    distance (N,))``.  The candidates of a point are the triangles incident to its ``k`` nearest mesh vertices; of these the one with
    the smallest distance (``closest_on_triangles``) is kept, on a tie the one with the smallest index.  This rule is the definition
    of the result (deterministic; no claim beyond the candidate set).  A triangle of zero area raises ``ValueError``."""
    from scipy.spatial import cKDTree

    p = np.ascontiguousarray(points, dtype=np.float64)
    v = np.ascontiguousarray(vertices, dtype=np.float64)
    t = np.asarray(triangles).astype(np.int64)
    if p.ndim != 2 or p.shape[1] != 3 or v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise ValueError("locate: points (N, 3), vertices (V, 3) and triangles (F, 3) expected")
    if t.min() < 0 or t.max() >= v.shape[0]:
        raise ValueError("locate: a triangle names a vertex the mesh does not have")
    if not np.all(np.linalg.norm(np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]), axis=1) > 0.0):
        raise ValueError("locate: the mesh has a triangle of zero area")
    k = max(1, min(int(k), v.shape[0]))
    # the triangles around every vertex as a padded table (V, max degree), -1 where a vertex has fewer
    corner_vertex = t.reshape(-1)
    order = np.argsort(corner_vertex, kind="stable")
    degree = np.bincount(corner_vertex, minlength=v.shape[0])
    start = np.concatenate([[0], np.cumsum(degree)])
    around = np.full((v.shape[0], max(int(degree.max()), 1)), -1, dtype=np.int64)
    sorted_vertex = corner_vertex[order]
    around[sorted_vertex, np.arange(order.size) - start[sorted_vertex]] = order // 3
    tree = cKDTree(v)
    tri = np.empty(p.shape[0], dtype=np.int64)
    weights = np.empty((p.shape[0], 3))
    distance = np.empty(p.shape[0])
    for lo in range(0, p.shape[0], LOCATE_CHUNK):
        pc = p[lo:lo + LOCATE_CHUNK]
        near = tree.query(pc, k=k)[1].reshape(pc.shape[0], k)
        cand = np.sort(around[near].reshape(pc.shape[0], -1), axis=1)      # (ascending: the first minimum is the smallest index)
        n_c = cand.shape[1]
        f = np.maximum(cand, 0).reshape(-1)
        w, d = closest_on_triangles(np.repeat(pc, n_c, axis=0), v[t[f, 0]], v[t[f, 1]], v[t[f, 2]])
        d = np.where(cand >= 0, d.reshape(pc.shape[0], n_c), np.inf)
        if not np.all(np.isfinite(d.min(axis=1))):
            raise ValueError("locate: a nearest vertex belongs to no triangle")
        best = np.argmin(d, axis=1)
        rows = np.arange(pc.shape[0])
        tri[lo:lo + pc.shape[0]] = cand[rows, best]
        weights[lo:lo + pc.shape[0]] = w.reshape(pc.shape[0], n_c, 3)[rows, best]
        distance[lo:lo + pc.shape[0]] = d[rows, best]
    return tri, weights, distance


_locate_kdtree = locate      # (mesh_transfer's keyword ``locate`` shadows the function)
LOCATE_MODES = ("kdtree", "exact", "device")
LOCATE_EXACT_PAIRS = 1 << 21      # point-triangle pairs per pass of locate_exact


def check_locate(locate, who):
    if locate not in LOCATE_MODES:
        raise ValueError(f"{who}: locate must be one of {list(LOCATE_MODES)}")


def closest_scalar_order(p, a, b, c):
    """``closest_on_triangles`` restated in a fixed order of operations (arrays that broadcast against each other, last axis 3):
    ``(w0, w1, w2, d2)``, the clamped weights and the SQUARED distance.  Every dot product is ``(x0*y0 + x1*y1) + x2*y2``, the closest
    point ``q = (w0*a + w1*b) + w2*c``, ``d2 = (rx*rx + ry*ry) + rz*rz`` with ``r = p - q``; the six region conditions are those of
    ``closest_on_triangles`` in the same order.  The device kernel (k_locate, csrc/kernels_locate.hip) performs these operations."""
    def dot(x, y):
        return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]

    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = p - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = p - c
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t_ab, t_ac = d1 / (d1 - d3), d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = 1.0 / ((va + vb) + vc)
        v_in, w_in = vb * denom, vc * denom
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    w1 = np.select(conds, [zero, one, t_ab, zero, zero, 1.0 - t_bc], default=v_in)
    w2 = np.select(conds, [zero, zero, zero, one, t_ac, t_bc], default=w_in)
    clamp = lambda x: np.where(x < 0.0, 0.0, np.where(x > 1.0, 1.0, x))      # noqa: E731  (as the kernel's two selects)
    w1, w2 = clamp(w1), clamp(w2)
    w0 = (1.0 - w1) - w2
    w0 = np.where(w0 < 0.0, 0.0, w0)
    r = p - ((w0[..., None] * a + w1[..., None] * b) + w2[..., None] * c)
    return w0, w1, w2, dot(r, r)


def _locate_arguments(points, vertices, triangles, who):
    p = np.ascontiguousarray(points, dtype=np.float64)
    v = np.ascontiguousarray(vertices, dtype=np.float64)
    t = np.asarray(triangles).astype(np.int64)
    if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1 or v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise ValueError(f"{who}: points (N, 3), vertices (V, 3) and triangles (F, 3) expected")
    return p, v, t


def locate_exact(points, vertices, triangles):
    """The closest point of the mesh ``(vertices, triangles)`` to every one of ``points`` over ALL triangles: ``(triangle (N,) int64,
    weights (N, 3), distance (N,))``.  Per point and triangle ``closest_scalar_order``; the winner is the smallest ``(d2, triangle
    index)``; ``distance = sqrt(d2)``.  Brute force in chunks: the specification of ``dots_mesh_locate``, which returns these arrays bit
    for bit.  ``ValueError``: an index out of range, a triangle of zero area, non-finite coordinates or points."""
    p, v, t = _locate_arguments(points, vertices, triangles, "locate_exact")
    if t.min() < 0 or t.max() >= v.shape[0]:
        raise ValueError("locate_exact: a triangle names a vertex the mesh does not have")
    if not (np.all(np.isfinite(p)) and np.all(np.isfinite(v))):
        raise ValueError("locate_exact: non-finite coordinates or points")
    if not np.all(np.linalg.norm(np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]), axis=1) > 0.0):
        raise ValueError("locate_exact: the mesh has a triangle of zero area")
    a, b, c = v[t[:, 0]][None], v[t[:, 1]][None], v[t[:, 2]][None]
    tri = np.empty(p.shape[0], dtype=np.int64)
    weights = np.empty((p.shape[0], 3))
    distance = np.empty(p.shape[0])
    chunk = max(1, LOCATE_EXACT_PAIRS // t.shape[0])
    for lo in range(0, p.shape[0], chunk):
        pc = p[lo:lo + chunk]
        w0, w1, w2, d2 = closest_scalar_order(pc[:, None, :], a, b, c)
        best = np.argmin(d2, axis=1)      # (the first minimum: the smallest triangle index on a tie)
        rows = np.arange(pc.shape[0])
        tri[lo:lo + pc.shape[0]] = best
        weights[lo:lo + pc.shape[0]] = np.stack([w0[rows, best], w1[rows, best], w2[rows, best]], axis=1)
        distance[lo:lo + pc.shape[0]] = np.sqrt(d2[rows, best])
    return tri, weights, distance


def corner_exact(corner_points, vertices, triangles, triangle):
    """For point i with the three corner points ``corner_points[i]`` (N, 3, 3): the corner of ``triangle[i]`` with the largest clamped
    weight (``closest_scalar_order``) of each corner point with respect to that one triangle, the first maximum on a tie: (N, 3) int32."""
    v, t = np.asarray(vertices, dtype=np.float64), np.asarray(triangles).astype(np.int64)
    f = np.asarray(triangle).astype(np.int64)
    a, b, c = v[t[f, 0]][:, None, :], v[t[f, 1]][:, None, :], v[t[f, 2]][:, None, :]
    w0, w1, w2, _ = closest_scalar_order(np.asarray(corner_points, dtype=np.float64), a, b, c)
    return np.argmax(np.stack([w0, w1, w2], axis=-1), axis=-1).astype(np.int32)


def locate_device(points, vertices, triangles, corner_points=None, device=0, timing=None):
    """``locate_exact`` (and ``corner_exact`` when ``corner_points`` (N, 3, 3) is given) on the device (``dots_mesh_locate``): the same
    arrays bit for bit, ``(triangle, weights, distance)`` or ``(triangle, weights, distance, corner)``.  ``timing``: a dict that
    receives "kernel_ms" (device events around the launches).  There is no host fall-back: without the library or a device it raises."""
    import ctypes as C

    from . import _lib

    p, v, t = _locate_arguments(points, vertices, triangles, "locate_device")
    if t.max() >= 2 ** 31 or t.min() < -2 ** 31 or max(p.shape[0], v.shape[0], t.shape[0]) >= 2 ** 31:
        raise ValueError("locate_device: sizes and indices must fit 32 bits")
    t32 = np.ascontiguousarray(t, dtype=np.int32)
    n = p.shape[0]
    tri, weights, distance = np.empty(n, dtype=np.int32), np.empty((n, 3)), np.empty(n)
    corner = cp = None
    if corner_points is not None:
        cp = np.ascontiguousarray(corner_points, dtype=np.float64)
        if cp.shape != (n, 3, 3):
            raise ValueError("locate_device: corner_points must be (N, 3, 3)")
        corner = np.empty((n, 3), dtype=np.int32)
    ms = C.c_double(0.0)
    desc = _lib.MeshLocateDesc(
        n_points=n, n_vertices=v.shape[0], n_triangles=t32.shape[0], reserved=0, points=p.ctypes.data_as(_lib._f64p),
        vertices=v.ctypes.data_as(_lib._f64p), triangles=t32.ctypes.data_as(_lib._i32p),
        corner_points=None if cp is None else cp.ctypes.data_as(_lib._f64p), triangle=tri.ctypes.data_as(_lib._i32p),
        weights=weights.ctypes.data_as(_lib._f64p), distance=distance.ctypes.data_as(_lib._f64p),
        corner=None if corner is None else corner.ctypes.data_as(_lib._i32p), ms=C.pointer(ms))
    lib = _lib.load()
    rc = lib.dots_mesh_locate(C.byref(desc), int(device))
    if rc == _lib.ERR_ARGUMENT:
        raise ValueError("locate_device: " + lib.dots_last_error().decode("utf-8", "replace"))
    _lib.check(rc, "dots_mesh_locate")
    if timing is not None:
        timing["kernel_ms"] = float(ms.value)
    out = (tri.astype(np.int64), weights, distance)
    return out if corner is None else out + (corner,)


def mesh_transfer(coarse_geometry, fine_geometry, locate="kdtree", device=0):
    """The transfer from the mesh of ``coarse_geometry`` to that of ``fine_geometry``, two independent triangulations of one surface
    in the same coordinates (normalise them together): a dict with

    * ``vertex_sources`` (Vf, 3) int32, ``vertex_weights`` (Vf, 3) float64: the three coarse vertices of the triangle ``locate``
      finds for every fine vertex, in that triangle's corner order, and their clamped barycentric weights;
    * ``triangle_source`` (Ff,) int32: the coarse triangle located for the centroid of every fine triangle;
    * ``corner_source`` (Ff, 3) int32: for the fine corner ``(f', k)`` the corner of ``triangle_source[f']`` with the largest clamped
      barycentric weight of the fine vertex ``triangles_f[f', k]`` with respect to that one triangle (a tie: the smallest corner);
    * ``max_distance``: the largest distance of a fine vertex or centroid from the coarse mesh; ``n_source_vertices``,
      ``n_source_triangles``.

    ``locate``: "kdtree" is ``locate`` (the candidates around the three nearest vertices); "exact" is ``locate_exact`` /
    ``corner_exact`` (the closest point over all triangles: what a decimated pair needs, ``meshes.coarsen_levels``); "device" is
    ``locate_device`` on GPU ``device`` and returns what "exact" returns.

    ``ValueError`` when ``max_distance`` exceeds the longest edge of the coarse mesh: not the same surface, or not the same scaling."""
    check_locate(locate, "mesh_transfer")
    vc = np.asarray(coarse_geometry["vertices"], dtype=np.float64)
    tc = np.asarray(coarse_geometry["triangles"]).astype(np.int64)
    vf = np.asarray(fine_geometry["vertices"], dtype=np.float64)
    tf = np.asarray(fine_geometry["triangles"]).astype(np.int64)
    centroid = (vf[tf[:, 0]] + vf[tf[:, 1]] + vf[tf[:, 2]]) / 3.0
    if locate == "kdtree":
        tri_v, w_v, d_v = _locate_kdtree(vf, vc, tc)
        tri_f, _, d_f = _locate_kdtree(centroid, vc, tc)
        corner = np.empty((tf.shape[0], 3), dtype=np.int32)
        for k in range(3):
            w, _ = closest_on_triangles(vf[tf[:, k]], vc[tc[tri_f, 0]], vc[tc[tri_f, 1]], vc[tc[tri_f, 2]])
            corner[:, k] = np.argmax(w, axis=1)      # (the first maximum: the smallest corner index on a tie)
    elif locate == "exact":
        tri_v, w_v, d_v = locate_exact(vf, vc, tc)
        tri_f, _, d_f = locate_exact(centroid, vc, tc)
        corner = corner_exact(vf[tf], vc, tc, tri_f)
    else:      # one call: the vertices first, then the centroids with the corner points of their triangles
        points = np.concatenate([vf, centroid], axis=0)
        corner_points = np.concatenate([np.repeat(vf[:, None, :], 3, axis=1), vf[tf]], axis=0)
        tri, w, d, cn = locate_device(points, vc, tc, corner_points=corner_points, device=device)
        n = vf.shape[0]
        tri_v, w_v, d_v, tri_f, d_f, corner = tri[:n], w[:n], d[:n], tri[n:], d[n:], np.ascontiguousarray(cn[n:])
    max_distance = float(max(d_v.max(), d_f.max()))
    edges = np.concatenate([vc[tc[:, 1]] - vc[tc[:, 0]], vc[tc[:, 2]] - vc[tc[:, 1]], vc[tc[:, 0]] - vc[tc[:, 2]]], axis=0)
    longest = float(np.linalg.norm(edges, axis=1).max())
    if not max_distance <= longest:
        raise ValueError(f"mesh_transfer: the fine mesh is up to {max_distance:.3g} away from the coarse one, whose longest edge is "
                         f"{longest:.3g}: not the same surface, or not the same scaling (normalise the geometries together)")
    return {"vertex_sources": np.ascontiguousarray(tc[tri_v], dtype=np.int32), "vertex_weights": np.ascontiguousarray(w_v),
            "triangle_source": np.ascontiguousarray(tri_f, dtype=np.int32), "corner_source": corner, "max_distance": max_distance,
            "n_source_vertices": int(vc.shape[0]), "n_source_triangles": int(tc.shape[0])}


def check_transfer(transfer, n_vertices=None, n_triangles=None):
    """``(vertex_sources (Vf, 3), vertex_weights (Vf, 3), triangle_source (Ff,), corner_source (Ff, 3))`` of ``transfer``
    (``mesh_transfer``), the index arrays as int64; ``n_vertices`` / ``n_triangles``: the size of the source mesh it must refer to."""
    try:
        vs, vw = np.asarray(transfer["vertex_sources"]), np.asarray(transfer["vertex_weights"])
        ts, cs = np.asarray(transfer["triangle_source"]), np.asarray(transfer["corner_source"])
        nv, nt = int(transfer["n_source_vertices"]), int(transfer["n_source_triangles"])
    except (KeyError, TypeError, IndexError, ValueError):
        raise ValueError("transfer must hold 'vertex_sources', 'vertex_weights', 'triangle_source', 'corner_source', 'n_source_vertices' "
                         "and 'n_source_triangles' (cascade.mesh_transfer)") from None
    if vs.ndim != 2 or vs.shape[1] != 3 or vs.shape[0] < 1 or vw.shape != vs.shape:
        raise ValueError("transfer: vertex_sources and vertex_weights must be (Vf, 3)")
    if ts.ndim != 1 or ts.shape[0] < 1 or cs.shape != (ts.shape[0], 3):
        raise ValueError("transfer: triangle_source must be (Ff,) and corner_source (Ff, 3)")
    if not all(np.issubdtype(a.dtype, np.integer) for a in (vs, ts, cs)):
        raise ValueError("transfer: integer index arrays expected")
    if not np.issubdtype(vw.dtype, np.floating):
        raise ValueError("transfer: floating-point weights expected")
    vs, ts, cs, vw = vs.astype(np.int64), ts.astype(np.int64), cs.astype(np.int64), vw.astype(np.float64)
    if vs.min() < 0 or vs.max() >= nv or ts.min() < 0 or ts.max() >= nt:
        raise ValueError("transfer: an index outside the source mesh")
    if cs.min() < 0 or cs.max() > 2:
        raise ValueError("transfer: corner_source must be 0, 1 or 2")
    if not (np.all(np.isfinite(vw)) and np.all(vw >= 0.0)):
        raise ValueError("transfer: the weights must be finite and >= 0")
    if n_vertices is not None and nv != int(n_vertices):
        raise ValueError(f"transfer: from a mesh of {nv} vertices, not {int(n_vertices)}")
    if n_triangles is not None and nt != int(n_triangles):
        raise ValueError(f"transfer: from a mesh of {nt} triangles, not {int(n_triangles)}")
    return vs, vw, ts, cs


def transfer_space(array, name, transfer):
    """``array`` (the state array ``name`` on the source mesh of ``transfer``, reference layout) on the destination mesh; the time axis
    is untouched.

    * vertex arrays: ``(w0 * x[..., s0] + w1 * x[..., s1]) + w2 * x[..., s2]`` with the three sources and weights of the vertex, in
      exactly this order of operations and with no special case for a weight of 0 or 1;
    * triangle arrays (``B``, ``E``): a triangle takes the three components of ``triangle_source`` unchanged.  As in
      ``prolong_space`` they are NOT re-projected into the destination triangle's plane: the small normal component is left to the
      first iterations on the destination mesh;
    * corner arrays (``z_mid``, ``beta_mid``): corner ``(f', k)`` takes corner ``(triangle_source[f'], corner_source[f', k])`` for
      both interval ends and every component."""
    a = np.asarray(array, dtype=np.float64)
    if name in VERTEX_ARRAYS:
        if a.ndim != 2:
            raise ValueError(f"{name}: expected (time, V), got shape {a.shape}")
        vs, vw, _, _ = check_transfer(transfer, n_vertices=a.shape[-1])
        return (vw[:, 0] * a[..., vs[:, 0]] + vw[:, 1] * a[..., vs[:, 1]]) + vw[:, 2] * a[..., vs[:, 2]]
    if name in TRIANGLE_ARRAYS:
        if a.ndim != 3 or a.shape[-1] != 3:
            raise ValueError(f"{name}: expected (time, F, 3), got shape {a.shape}")
        _, _, ts, _ = check_transfer(transfer, n_triangles=a.shape[-2])
        return np.ascontiguousarray(a[..., ts, :])
    if name in CORNER_ARRAYS:
        if a.ndim != 5 or a.shape[1:3] != (2, 3) or a.shape[-1] != 3:
            raise ValueError(f"{name}: expected (time, 2, 3, F, 3), got shape {a.shape}")
        _, _, ts, cs = check_transfer(transfer, n_triangles=a.shape[-2])
        return np.ascontiguousarray(a[:, :, cs.T, ts[None, :], :])      # [t][s][k][f'][c] = a[t][s][cs[f'][k]][ts[f']][c]
    raise ValueError(f"unknown state array {name!r}")


def transfer_space_solution(solution, transfer):
    """Every state array of ``solution`` (a dict as ``solver_socp`` returns it) on the destination mesh of ``transfer``: an
    ``init_solution``."""
    names = VERTEX_ARRAYS + TRIANGLE_ARRAYS + CORNER_ARRAYS
    return {k: transfer_space(v, k, transfer) for k, v in solution.items() if k in names and v is not None}


def transfer_row_maps(transfer, perm_vert_dst=None, perm_tri_dst=None, perm_vert_src=None, perm_tri_src=None):
    """The tables of ``dots_transfer_space``: ``vsrc`` (Vf, 3) int32, the three source device rows of every destination device vertex
    row, ``vw`` (Vf, 3) their weights, ``fsrc`` (Ff,) int32, the source device triangle of every destination device triangle, and
    ``csrc`` (Ff, 3) int32.  ``perm[i]`` = caller index of device row i (None = identity), as in ``space_row_maps``.  A renumbering
    permutes the rows of the tables and renames the sources; the order of a vertex's three sources is never changed, so the sums do
    not depend on the numberings.  The plans keep the corner order inside a triangle (as ``space_row_maps`` relies on), so
    ``corner_source`` is carried over as it is."""
    vs, vw, ts, cs = check_transfer(transfer)
    n_src_v, n_src_t = int(transfer["n_source_vertices"]), int(transfer["n_source_triangles"])

    for perm, n in ((perm_vert_dst, vs.shape[0]), (perm_tri_dst, ts.shape[0])):
        if perm is not None and np.asarray(perm).shape != (n,):
            raise ValueError("transfer_row_maps: a permutation of the wrong size")
    if perm_vert_dst is not None:
        pv = np.asarray(perm_vert_dst, dtype=np.int64)
        vs, vw = vs[pv], vw[pv]
    if perm_tri_dst is not None:
        pt = np.asarray(perm_tri_dst, dtype=np.int64)
        ts, cs = ts[pt], cs[pt]
    vsrc = inverse_numbering(perm_vert_src, n_src_v, "transfer_row_maps")[vs]
    fsrc = inverse_numbering(perm_tri_src, n_src_t, "transfer_row_maps")[ts]
    return (np.ascontiguousarray(vsrc, dtype=np.int32), np.ascontiguousarray(vw, dtype=np.float64),
            np.ascontiguousarray(fsrc, dtype=np.int32), np.ascontiguousarray(cs, dtype=np.int32))


# ---- coarse-to-fine in space and time at once ------------------------------------------------------------------------------------
def _one_map(who, parents, transfer):
    if (parents is None) == (transfer is None):
        raise ValueError(f"{who}: exactly one of parents (the source is the parent mesh) and transfer (a located mesh) is needed")


def carry_spacetime(array, name, n_src, n_dst, parents=None, transfer=None):
    """``array`` (the state array ``name`` on the source mesh and the grid of ``n_src`` intervals, reference layout) on the destination
    mesh of ``parents`` (``prolong_space``) or of ``transfer`` (``transfer_space``) -- exactly one of them -- and on the grid of ``n_dst``
    intervals.  Space first, then time: ``prolong_time(prolong_space(array, name, parents), name, n_src, n_dst)``, or the same with
    ``transfer_space``; this order of operations is the definition.  Only for ``n_src != n_dst``: on equal grids ``prolong_time`` is
    ``(1 - w) * a[j] + w * a[j1]`` at ``w = 0``, which differs from a plain carry in the sign of zero and next to non-finite values, so
    equal grids stay with ``prolong_space`` / ``transfer_space`` alone (``ValueError``)."""
    _one_map("carry_spacetime", parents, transfer)
    if int(n_src) == int(n_dst):
        raise ValueError(f"carry_spacetime: both grids have {int(n_dst)} intervals: on one time grid the carriers in space "
                         "(prolong_space / transfer_space) are the definition")
    in_space = prolong_space(array, name, parents) if parents is not None else transfer_space(array, name, transfer)
    return prolong_time(in_space, name, n_src, n_dst)


def carry_spacetime_solution(solution, n_src, n_dst, parents=None, transfer=None):
    """Every state array of ``solution`` (a dict as ``solver_socp`` returns it) on the destination mesh and the grid of ``n_dst``
    intervals: an ``init_solution``."""
    _one_map("carry_spacetime_solution", parents, transfer)
    names = VERTEX_ARRAYS + TRIANGLE_ARRAYS + CORNER_ARRAYS
    return {k: carry_spacetime(v, k, n_src, n_dst, parents=parents, transfer=transfer) for k, v in solution.items() if k in names and v is not None}


def default_spacetime_levels(n_time, n_geometries):
    """The ``n_time`` of every mesh level (coarse to fine) of a cascade in space and time that ends at ``n_time``: from the finest level
    downward ``n_time + 1`` is halved per mesh level while it is even and the half stays >= ``MIN_LEVEL_NODES``, then held
    (127, 3 levels -> 31, 63, 127; 31 -> 15, 15, 31; 20 -> 20, 20)."""
    nodes = int(n_time) + 1
    levels = [nodes - 1]
    for _ in range(int(n_geometries) - 1):
        if nodes % 2 == 0 and nodes // 2 >= MIN_LEVEL_NODES:
            nodes //= 2
        levels.append(nodes - 1)
    return levels[::-1]


def check_spacetime_levels(levels, n_time, n_geometries):
    """The levels as a list of ints: one per geometry, at least one interval each, never decreasing, ending in ``n_time``."""
    if levels is None:
        return default_spacetime_levels(n_time, n_geometries)
    try:
        out = [int(x) for x in levels]
    except (TypeError, ValueError):
        raise ValueError("levels must be a list of n_time values, one per geometry") from None
    if any(int(a) != a for a in levels):
        raise ValueError("levels must be a list of integers")
    if len(out) != int(n_geometries):
        raise ValueError(f"levels: one n_time per geometry ({int(n_geometries)}), got {len(out)}")
    if out[0] < 1:
        raise ValueError("levels: every level needs n_time >= 1")
    if any(b < a for a, b in zip(out, out[1:])):
        raise ValueError(f"levels must not decrease (got {out})")
    if out[-1] != int(n_time):
        raise ValueError(f"the last level must be n_time = {int(n_time)} (got {out[-1]})")
    return out

"""Coarse-to-fine cascades: the transfer of a solution between two time grids, or between two nested meshes, as a specification on
the host.

A solution on a coarse time grid is a good starting point for a finer one (``init_solution``, solver_socp.py:38,70-71).  This
module is the single definition of the interpolation that the device kernel (``dots_prolong_time``, csrc/kernels_alm.hip), the
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

The transfer in space (``prolong_space``; ``dots_prolong_space``, k_prolong_space in csrc/kernels_alm.hip) goes from a mesh to its
nested refinement (``meshes.subdivide``: ``parents``) on one time grid; ``space_row_maps`` turns ``parents`` and the two device
numberings into the row maps the kernel reads.
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


def row_map(perm_dst, perm_src, n):
    """Destination device row -> source device row for two plans of one mesh (``perm[i]`` = caller index of device row i, None =
    identity); None when both numberings agree."""
    if perm_dst is None and perm_src is None:
        return None
    pd = np.arange(n, dtype=np.int64) if perm_dst is None else np.asarray(perm_dst, dtype=np.int64)
    ps = np.arange(n, dtype=np.int64) if perm_src is None else np.asarray(perm_src, dtype=np.int64)
    if np.array_equal(pd, ps):
        return None
    inv_src = np.empty(n, dtype=np.int64)
    inv_src[ps] = np.arange(n)
    return np.ascontiguousarray(inv_src[pd], dtype=np.int32)


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

    def inverse(perm, n):
        if perm is None:
            return np.arange(n, dtype=np.int64)
        perm = np.asarray(perm, dtype=np.int64)
        if perm.shape != (n,):
            raise ValueError("space_row_maps: a permutation of the wrong size")
        inv = np.empty(n, dtype=np.int64)
        inv[perm] = np.arange(n)
        return inv

    for perm, n in ((perm_vert_dst, vp.shape[0]), (perm_tri_dst, tp.shape[0])):
        if perm is not None and np.asarray(perm).shape != (n,):
            raise ValueError("space_row_maps: a permutation of the wrong size")
    vd = vp if perm_vert_dst is None else vp[np.asarray(perm_vert_dst, dtype=np.int64)]
    td = tp if perm_tri_dst is None else tp[np.asarray(perm_tri_dst, dtype=np.int64)]
    vmap = inverse(perm_vert_src, int(n_src_vertices))[vd]
    fmap = inverse(perm_tri_src, int(n_src_triangles))[td]
    return np.ascontiguousarray(vmap, dtype=np.int32), np.ascontiguousarray(fmap, dtype=np.int32)

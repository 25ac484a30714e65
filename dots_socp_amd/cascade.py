"""Coarse-to-fine time cascade: the transfer of a solution between two time grids, as a specification on the host.

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

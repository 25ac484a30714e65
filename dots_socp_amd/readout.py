"""The read-out of a solve: what the solver plug-ins return (``mu`` and ``E`` in DOT units, ``mu`` on the staggered or the
time-centred grid), from the solver's scaled iterate.

``read_out_host`` is the numpy specification of ``dots_readout`` (include/dots_socp_hip.h): the operations of
``AlmSolver.recovered`` (solver_socp.py:397-405), ``socp._socp_to_dot`` (utils/type.py:48-65) and ``socp._to_time_centered``
(socp/solver_decorator.py:29-54), in that order.  The device forms every value with the same operations in the same order, so
the two agree bit for bit.
"""
from __future__ import annotations

import numpy as np


def read_out_host(solution_or_arrays, factor=1.0, w_vertex=None, w_triangle=None, centred=False, mu0=None, mu1=None):
    """``(mu, E)`` from a mapping with ``"mu"`` (T, V) and / or ``"E"`` (T + 1, F, 3) (a missing or None entry gives None):
    every value times ``factor``, then times the weight of its vertex (``w_vertex``, (V,)) / triangle (``w_triangle``, (F,)) where
    given; ``centred``: ``mu`` becomes the T + 1 layers mu0, 0.5 * (a[l - 1] + a[l]), mu1."""
    mu, E = solution_or_arrays.get("mu"), solution_or_arrays.get("E")
    if mu is not None:
        mu = float(factor) * np.asarray(mu, dtype=np.float64)
        if w_vertex is not None:
            mu = mu * np.asarray(w_vertex, dtype=np.float64)[np.newaxis, :]
        if centred:
            if mu0 is None or mu1 is None:
                raise ValueError("read_out_host: the centred output needs mu0 and mu1")
            mu0, mu1 = np.asarray(mu0, dtype=np.float64), np.asarray(mu1, dtype=np.float64)
            mid = 0.5 * (mu[:-1] + mu[1:])
            mu = np.concatenate([mu0[None, :], mid, mu1[None, :]], axis=0)
    if E is not None:
        E = float(factor) * np.asarray(E, dtype=np.float64)
        if w_triangle is not None:
            E = E * np.asarray(w_triangle, dtype=np.float64)[np.newaxis, :, np.newaxis]
    return mu, E


def layer_sums_host(mu):
    """(sum of every layer, sum of its negative entries): what ``dots_readout`` returns as layer_mass / layer_negative, up to the
    order of the additions."""
    mu = np.asarray(mu, dtype=np.float64)
    return mu.sum(axis=1), np.where(mu < 0.0, mu, 0.0).sum(axis=1)

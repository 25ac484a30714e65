"""Wasserstein barycentres of measures on one surface: ``nu`` minimising ``sum_k w_k cost(nu, mu_k)``, by mirror descent on the
simplex -- ``nu <- nu * exp(-eta * sum_k w_k grad_k)``, renormalised, with ``grad_k = -(phi0_k - mean)`` the derivative of the cost of
problem ``(nu -> mu_k)`` in its first end mass (sensitivity.potential_gradients).  For two measures the barycentre with the weights
``(1 - t, t)`` is the displacement interpolation at ``t``.

Host only, numpy and scalar floats: ``update_host`` is the specification of ``dots_barycenter_update`` (include/dots_socp_hip.h), which
forms every element with the same operations in the same order (its sums in another, fixed, order and its ``exp`` by the device's
library: the two agree to rounding, not bit for bit); ``barycenter_host`` is the loop over any solver, the slow twin of
``socp.barycenter``.
"""
from __future__ import annotations

import math

import numpy as np

MAX_MEASURES = 16      # dots_barycenter_desc.n


def _update_arguments(nu, potentials, weights, eta, mass):
    nu = np.asarray(nu, dtype=np.float64)
    potentials = np.asarray(potentials, dtype=np.float64)
    weights = np.asarray(weights, dtype=np.float64)
    if nu.ndim != 1 or nu.shape[0] < 1:
        raise ValueError(f"barycenter update: nu must have shape (V,), got {nu.shape}")
    if potentials.ndim != 2 or potentials.shape[1] != nu.shape[0] or not 1 <= potentials.shape[0] <= MAX_MEASURES:
        raise ValueError(f"barycenter update: potentials must have shape (K, {nu.shape[0]}) with 1 <= K <= {MAX_MEASURES}, got {potentials.shape}")
    if weights.shape != (potentials.shape[0],):
        raise ValueError(f"barycenter update: weights must have shape ({potentials.shape[0]},), got {weights.shape}")
    if not np.all(np.isfinite(weights)):
        raise ValueError("barycenter update: a weight that is not finite")
    if not (math.isfinite(float(eta)) and math.isfinite(float(mass))):
        raise ValueError("barycenter update: eta and mass must be finite")
    if not np.all(nu > 0.0):      # (a NaN is not positive either)
        raise ValueError("barycenter update: nu has an entry that is not positive: a multiplicative update cannot create support")
    return nu, potentials, weights, float(eta), float(mass)


def update_host(nu, potentials, weights, eta, mass):
    """One mirror-descent step: ``(nu_new (V,), {"sum", "change", "gmax", "min"})``.  ``nu`` (V,) positive, ``potentials`` (K, V) the
    ``phi0`` of each problem ``(nu -> mu_k)`` as ``dots_sensitivity`` stores it (no gauge fixed), ``weights`` (K,).  In this order:

        m_k = fsum(potentials[k]) / V
        g[v] = 0.0; for k ascending: g[v] = g[v] + weights[k] * (-(potentials[k][v] - m_k))
        y[v] = nu[v] * exp((-eta) * g[v]);  S = fsum(y);  nu_new[v] = y[v] * (mass / S)
        change = fsum(|nu_new - nu|);  gmax = max |g|;  min = min(nu_new)

    Nothing is fused.  Refused with a ``ValueError``: an entry of ``nu`` that is not positive, wrong shapes, a weight, ``eta`` or
    ``mass`` that is not finite."""
    nu, potentials, weights, eta, mass = _update_arguments(nu, potentials, weights, eta, mass)
    V = nu.shape[0]
    g = np.zeros(V)
    for k in range(potentials.shape[0]):
        m_k = math.fsum(potentials[k]) / V
        g = g + weights[k] * (-(potentials[k] - m_k))
    y = nu * np.exp((-eta) * g)
    S = math.fsum(y)
    nu_new = y * (mass / S)
    return nu_new, {"sum": S, "change": math.fsum(np.abs(nu_new - nu)), "gmax": float(np.max(np.abs(g))), "min": float(np.min(nu_new))}


def check_measures(who, measures, weights, n_vertices=None):
    """``(measures (K, V), weights (K,), mass)`` as the drivers take them: 1 to 16 finite non-negative measures of equal total mass
    (to 1e-9 relative), finite weights (default ``1 / K``).  ``who`` opens the messages."""
    try:
        m = np.asarray([np.asarray(x, dtype=np.float64) for x in measures], dtype=np.float64)
    except ValueError:
        m = None
    if m is None or m.ndim != 2 or not 1 <= m.shape[0] <= MAX_MEASURES or (n_vertices is not None and m.shape[1] != n_vertices):
        raise ValueError(f"{who}: measures must be (K, V) or a list of K arrays of shape (V,), 1 <= K <= {MAX_MEASURES}"
                         + ("" if n_vertices is None else f", V = {n_vertices}"))
    if not np.all(np.isfinite(m)) or np.any(m < 0.0):
        raise ValueError(f"{who}: a measure has entries that are negative or not finite")
    K = m.shape[0]
    w = np.full(K, 1.0 / K) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (K,) or not np.all(np.isfinite(w)):
        raise ValueError(f"{who}: weights must be {K} finite numbers")
    masses = [math.fsum(row) for row in m]
    mass = masses[0]
    if not mass > 0.0 or any(abs(x - mass) > 1e-9 * mass for x in masses):
        raise ValueError(f"{who}: the measures must have one positive total mass, got {masses}")
    return np.ascontiguousarray(m), w, mass


def default_start(measures, weights, area_vertices, mass):
    """``0.5 * sum_k w_k mu_k + 0.5 * mass * area_vertices / sum(area_vertices)``: half the weighted mean, half uniform -- positive
    wherever the surface has area."""
    area = np.asarray(area_vertices, dtype=np.float64)
    mean = np.zeros(measures.shape[1])
    for k in range(measures.shape[0]):
        mean = mean + weights[k] * measures[k]
    return 0.5 * mean + 0.5 * mass * area / math.fsum(area)


def check_start(who, init, n_vertices):
    nu = np.array(init, dtype=np.float64)
    if nu.shape != (n_vertices,):
        raise ValueError(f"{who}: init must have shape ({n_vertices},), got {nu.shape}")
    if not np.all(nu > 0.0) or not np.all(np.isfinite(nu)):
        raise ValueError(f"{who}: the start has an entry that is not positive (or not finite): a multiplicative update cannot create support")
    return nu


class StepRule:
    """The step of the outer loop: ``eta`` is halved for the steps that follow one whose objective exceeds that of the step before;
    nothing is redone.  Shared by ``barycenter_host`` and ``socp.barycenter``."""

    def __init__(self, eta):
        self.eta = float(eta)
        self.last = None

    def take(self, objective):
        """The ``eta`` of the update that follows the solves with this ``objective``."""
        if self.last is not None and objective > self.last:
            self.eta = 0.5 * self.eta
        self.last = objective
        return self.eta


def objective_of(costs, weights):
    """``sum_k w_k cost_k``, k ascending"""
    total = 0.0
    for k in range(len(costs)):
        total = total + float(weights[k]) * float(costs[k])
    return total


def barycenter_host(solve, measures, weights, area_vertices, steps, eta, init=None, tol_change=None):
    """The barycentre loop over any solver.  ``solve(nu, mu_k)`` returns ``(cost, phi0)`` of the transport problem ``(nu -> mu_k)``:
    the cost and the potential at the first end, (V,), as stored.  ``measures`` (K, V) of equal total mass, ``weights`` (K,) or None
    (``1 / K``), ``area_vertices`` (V,) for the default start (``default_start``; ``init`` (V,) positive replaces it).

    Step s = 0, 1, ...: the K problems are solved from the current ``nu`` -- its costs belong to that ``nu`` --, then ``update_host``
    moves it.  If the objective ``sum_k w_k cost_k`` of step s exceeds that of step s - 1, ``eta`` is halved for the updates from
    step s on.  Ends after ``steps`` steps, or when ``change < tol_change * mass``.

    Returns ``{"nu", "objective" [per step], "change" [per step], "costs" (K,) of the last step, "eta" [per step], "scalars" [per
    step: update_host's]}``."""
    who = "barycenter_host"
    m, w, mass = check_measures(who, measures, weights)
    if int(steps) < 1:
        raise ValueError(f"{who}: steps must be at least 1")
    V = m.shape[1]
    nu = default_start(m, w, area_vertices, mass) if init is None else np.asarray(init, dtype=np.float64)
    nu = check_start(who, nu, V)
    rule = StepRule(eta)
    out = {"objective": [], "change": [], "eta": [], "scalars": [], "costs": None}
    for _ in range(int(steps)):
        costs, potentials = [], []
        for k in range(m.shape[0]):
            cost, phi0 = solve(nu, m[k])
            costs.append(float(cost))
            potentials.append(np.asarray(phi0, dtype=np.float64))
        objective = objective_of(costs, w)
        step = rule.take(objective)
        nu, scalars = update_host(nu, np.stack(potentials), w, step, mass)
        out["objective"].append(objective)
        out["change"].append(scalars["change"])
        out["eta"].append(step)
        out["scalars"].append(scalars)
        out["costs"] = np.asarray(costs)
        if tol_change is not None and scalars["change"] < float(tol_change) * mass:
            break
    out["nu"] = nu
    return out

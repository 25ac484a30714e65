"""Linearised optimal transport on one surface: the measures ``mu_i`` seen from one reference measure ``sigma``.  The N problems
``(sigma -> mu_i)`` are solved, the initial velocity fields ``v_i = grad phi_i(0)`` -- the logarithmic map at ``sigma`` -- are kept, and
in the Hilbert space ``L2(sigma)`` the Gram matrix ``G_ij = <v_i, v_j>_sigma`` gives ``|v_i - v_j|^2 = G_ii + G_jj - 2 G_ij`` as an
approximation of ``W2^2(mu_i, mu_j)`` -- and PCA, clustering and kernels -- with no further solve.  ``G_ii / 2`` is the cost of problem
``i`` up to the discretisation.

Host only, numpy and scalar floats: ``velocities_host``, ``weights_host`` and ``gram_host`` are the specifications of
``dots_tangent_velocities``, ``dots_tangent_weights`` and ``dots_tangent_gram`` (include/dots_socp_hip.h), which form every element with
the same operations in the same order (the first two bit for bit; the Gram sums in another, fixed, order carried with error-free
additions: equal to the exactly rounded sum to the last bit or the one before it); ``tangent_embedding_host`` is the loop over any
solver, the slow twin of ``socp.tangent_embedding``.
"""
from __future__ import annotations

import math

import numpy as np

from .barycenter import MAX_MEASURES, check_measures


def _mesh_arguments(who, triangles, n_vertices=None):
    t = np.asarray(triangles)
    if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 1 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"{who}: triangles must be integers of shape (F, 3), got {t.shape} {t.dtype}")
    if n_vertices is not None and (t.min() < 0 or t.max() >= n_vertices):
        raise ValueError(f"{who}: a triangle index outside [0, {n_vertices})")
    return t


def velocities_host(potentials, triangles, hat):
    """``vel`` (n, F, 3): the gradient of every potential on every triangle.  ``potentials`` (n, V) as stored (no gauge is fixed: the
    hat gradients of a triangle sum to zero), ``triangles`` (F, 3), ``hat`` (F, 3, 3) ``[f][corner][xyz]`` -- the plan's hat gradients
    in the caller's numbering, the ones the device holds, not recomputed.  In this order, nothing fused:

        p[c] = potentials[i][triangles[f][c]]
        vel[i][f][d] = (hat[f][0][d] * p[0] + hat[f][1][d] * p[1]) + hat[f][2][d] * p[2]
    """
    who = "velocities_host"
    phi = np.asarray(potentials, dtype=np.float64)
    if phi.ndim != 2 or phi.shape[0] < 1:
        raise ValueError(f"{who}: potentials must have shape (n, V) with n >= 1, got {phi.shape}")
    t = _mesh_arguments(who, triangles, phi.shape[1])
    hat = np.asarray(hat, dtype=np.float64)
    if hat.shape != (t.shape[0], 3, 3):
        raise ValueError(f"{who}: hat must have shape ({t.shape[0]}, 3, 3), got {hat.shape}")
    p = phi[:, t]                                                      # (n, F, 3): [i][f][corner]
    return (hat[None, :, 0, :] * p[:, :, 0, None] + hat[None, :, 1, :] * p[:, :, 1, None]) + hat[None, :, 2, :] * p[:, :, 2, None]


def weights_host(sigma, mass_v, triangles, area_f):
    """``w`` (F,): the mass of ``sigma`` on every triangle; their sum is the mass of ``sigma``.  ``sigma`` (V,) may have zeros,
    ``mass_v`` (V,) the vertex masses (incident area / 3), ``area_f`` (F,).  In this order:

        rho[v] = sigma[v] / mass_v[v]
        w[f] = ((rho[v0] + rho[v1]) + rho[v2]) * (area_f[f] * (1.0 / 3.0))
    """
    who = "weights_host"
    sigma, mass_v, area_f = (np.asarray(a, dtype=np.float64) for a in (sigma, mass_v, area_f))
    if sigma.ndim != 1 or sigma.shape[0] < 1 or mass_v.shape != sigma.shape:
        raise ValueError(f"{who}: sigma and mass_v must have one shape (V,), got {sigma.shape} and {mass_v.shape}")
    t = _mesh_arguments(who, triangles, sigma.shape[0])
    if area_f.shape != (t.shape[0],):
        raise ValueError(f"{who}: area_f must have shape ({t.shape[0]},), got {area_f.shape}")
    rho = sigma / mass_v
    return ((rho[t[:, 0]] + rho[t[:, 1]]) + rho[t[:, 2]]) * (area_f * (1.0 / 3.0))


def gram_terms(a, b, w):
    """``term[f] = w[f] * ((a[f][0] * b[f][0] + a[f][1] * b[f][1]) + a[f][2] * b[f][2])`` of two fields (F, 3)"""
    return w * ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])


def gram_host(A, B, w):
    """``G`` (na, nb), ``G[i][j] = math.fsum(term)`` with ``term`` of ``gram_terms(A[i], B[j], w)``: the exactly rounded sum.  ``A``
    (na, F, 3), ``B`` (nb, F, 3) or None (``B = A``: the result is symmetric bit for bit, because the products commute), ``w`` (F,)."""
    who = "gram_host"
    A = np.asarray(A, dtype=np.float64)
    B = A if B is None else np.asarray(B, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    if A.ndim != 3 or A.shape[2] != 3 or A.shape[0] < 1 or A.shape[1] < 1:
        raise ValueError(f"{who}: A must have shape (na, F, 3), got {A.shape}")
    if B.ndim != 3 or B.shape[0] < 1 or B.shape[1:] != A.shape[1:]:
        raise ValueError(f"{who}: B must have shape (nb, {A.shape[1]}, 3), got {B.shape}")
    if w.shape != (A.shape[1],):
        raise ValueError(f"{who}: w must have shape ({A.shape[1]},), got {w.shape}")
    G = np.empty((A.shape[0], B.shape[0]))
    for i in range(A.shape[0]):
        for j in range(B.shape[0]):
            G[i, j] = math.fsum(gram_terms(A[i], B[j], w))
    return G


def squared_distances(G):
    """``D[i][j] = (G[i][i] + G[j][j]) - 2 G[i][j]``, clipped at 0: ``|v_i - v_j|^2`` in ``L2(sigma)``, the linearised ``W2^2(mu_i,
    mu_j)``.  Half of it is on the scale of the solver's "Transportation cost"."""
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise ValueError(f"squared_distances: G must be square, got {G.shape}")
    d = np.diag(G)
    return np.maximum((d[:, None] + d[None, :]) - 2.0 * G, 0.0)


def check_embedding(who, reference, measures, n_vertices=None):
    """``(reference (V,), measures (N, V), mass)`` as the drivers take them: finite, non-negative, one total mass
    (``barycenter.check_measures``, in groups of its 16 with the reference in each); N >= 1 has no upper limit."""
    try:
        rows = [np.asarray(x, dtype=np.float64) for x in measures]
        ref = np.asarray(reference, dtype=np.float64)
    except (ValueError, TypeError):
        rows = ref = None
    V = n_vertices if n_vertices is not None else (None if ref is None or ref.ndim != 1 else ref.shape[0])
    if not rows or ref is None or ref.ndim != 1 or (V is not None and ref.shape != (V,)) or any(r.shape != ref.shape for r in rows):
        raise ValueError(f"{who}: reference must have shape (V,) and measures must be (N, V) or a list of N arrays of shape (V,), N >= 1"
                         + ("" if n_vertices is None else f", V = {n_vertices}"))
    mass = None
    for at in range(0, len(rows), MAX_MEASURES - 1):
        _, _, mass = check_measures(who, [ref] + rows[at:at + MAX_MEASURES - 1], None, V)
    return np.ascontiguousarray(ref), np.ascontiguousarray(np.stack(rows)), mass


def tangent_embedding_host(solve, reference, measures, geometry, hat=None, area_triangles=None, mass_vertices=None):
    """The embedding over any solver.  ``solve(sigma, mu_i)`` returns ``(cost, phi0)`` of the transport problem ``(sigma -> mu_i)``:
    the cost and the potential at the first end, (V,), as stored.  ``reference`` (V,), ``measures`` (N, V) of its total mass,
    ``geometry`` with ``vertices`` and ``triangles``; ``hat`` (F, 3, 3), ``area_triangles`` (F,), ``mass_vertices`` (V,): the tables
    to use (a device plan's, in the caller's numbering), default ``geometry.hat_gradients`` and the incident areas / 3.

    Returns ``{"gram" (N, N), "costs" (N,), "squared_distances" (N, N), "velocities" (N, F, 3), "weights" (F,), "potentials" (N, V)}``
    with ``v_i = +grad phi0_i``."""
    from .geometry import hat_gradients

    who = "tangent_embedding_host"
    if not isinstance(geometry, dict) or "vertices" not in geometry or "triangles" not in geometry:
        raise ValueError(f"{who}: geometry must be a dict with 'vertices' and 'triangles'")
    vertices = np.asarray(geometry["vertices"], dtype=np.float64)
    V = vertices.shape[0]
    sigma, m, _ = check_embedding(who, reference, measures, V)
    t = _mesh_arguments(who, geometry["triangles"], V)
    if hat is None or area_triangles is None:
        area, own = hat_gradients(vertices, t)
        hat = own if hat is None else hat
        area_triangles = area if area_triangles is None else area_triangles
    if mass_vertices is None:
        mass_vertices = np.zeros(V)
        np.add.at(mass_vertices, t.reshape(-1), np.repeat(np.asarray(area_triangles, dtype=np.float64), 3))
        mass_vertices = mass_vertices / 3.0
    costs, potentials = [], []
    for i in range(m.shape[0]):
        cost, phi0 = solve(sigma, m[i])
        costs.append(float(cost))
        potentials.append(np.asarray(phi0, dtype=np.float64))
    potentials = np.stack(potentials)
    vel = velocities_host(potentials, t, hat)
    w = weights_host(sigma, mass_vertices, t, area_triangles)
    G = gram_host(vel, None, w)
    return {"gram": G, "costs": np.asarray(costs), "squared_distances": squared_distances(G), "velocities": vel, "weights": w,
            "potentials": potentials}

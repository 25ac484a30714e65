"""Gradients of the transport cost, from the converged state: in the end densities the Kantorovich potential at the two ends, in
the vertex positions minus the partial derivative of the discrete kinetic energy with masses and potential held fixed (envelope
theorem).  ``potentials_host`` and ``stress_host`` are the numpy / scalar specification of ``dots_sensitivity``
(include/dots_socp_hip.h): the device forms every value with the same operations in the same order, so the two agree bit for bit.

All quantities are those of the recovered solution (``phi = prim_scale * phi_dev``, ``mu = r * dual_scale * mu_dev``) in the
caller's numbering; ``mass_v = area_vertices / 3``, ``h = 1 / n_time``.

The kinetic energy is linear in a per-triangle tensor, the ``stress`` (F, 3, 6): for corner ``k`` of triangle ``f`` (vertex
``v_k = tri[f][k]``) and the entry ``e`` of ENTRIES = (a, b) = 00, 01, 02, 11, 12, 22, with ``p_t[a] = phi[t][tri[f][a]]``,

    stress[f][k][e] = sum_{t = 0}^{T - 1} (mu[t][v_k] * mass_v[v_k]) * 0.5 * (p_t[a] p_t[b] + p_{t+1}[a] p_{t+1}[b])

and  K(x) = h * sum_f sum_k (area_f / (3 mass_v[v_k])) * 0.5 * sum_{a, b} (hat[f][a] . hat[f][b]) * Psi_{f, k}[a][b]  with Psi the
stress unpacked symmetrically and area_f, mass_v, hat functions of the vertex positions x.  At a converged solve without
congestion K equals the transport cost, and d cost / d x = -dK/dx with the stress held fixed: the MASSES mu * mass_v are held
fixed, not the densities (holding mu fixed gives a wrong derivative: tests/sensitivity_checks.py pins that).
"""
from __future__ import annotations

import numpy as np

ENTRIES = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
# how often an entry occurs in the symmetric 3 x 3 tensor
ENTRY_WEIGHT = (1.0, 2.0, 2.0, 1.0, 2.0, 1.0)
SENSITIVITY_KEYS = ("potentials", "stress", "to_device")


def check_sensitivity(sensitivity, time_slab=None, congestion=0.0):
    """Refuse, before any device call, a ``sensitivity`` request that cannot be served: ``None`` / ``False`` (nothing), ``True`` (the
    potentials and the stress) or the keywords of ``AlmSolver.sensitivity`` as a dict.  Never on a time slab (one context holds every
    time node); the stress only without congestion (the identity K = cost was not established with it).  Returns None or the dict."""
    if sensitivity is None or sensitivity is False:
        return None
    if sensitivity is True:
        sensitivity = {}
    if not isinstance(sensitivity, dict):
        raise ValueError(f"sensitivity must be None, True or a dict with any of {list(SENSITIVITY_KEYS)}")
    unknown = set(sensitivity) - set(SENSITIVITY_KEYS)
    if unknown:
        raise ValueError(f"sensitivity: unknown option(s) {sorted(unknown)}; known: {list(SENSITIVITY_KEYS)}")
    out = {k: sensitivity.get(k, k != "to_device") for k in SENSITIVITY_KEYS}
    for k, v in out.items():
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"sensitivity: {k} must be True or False")
    if not out["potentials"] and not out["stress"]:
        raise ValueError("sensitivity: nothing asked for (potentials and stress are both False)")
    if time_slab is not None:
        raise ValueError("sensitivity is not available on time slabs: one GPU reduces the stress, and it holds every time node")
    if out["stress"] and float(congestion) > 0.0:
        raise ValueError("sensitivity: the stress is defined without congestion only (congestion > 0: ask for potentials alone, stress=False)")
    return {k: bool(v) for k, v in out.items()}


def potentials_host(phi, factor=1.0):
    """``(phi0, phiT)``: the first and the last time node of ``factor * phi`` ((T + 1, V)), as stored: no gauge is fixed here."""
    phi = np.asarray(phi, dtype=np.float64)
    return float(factor) * phi[0], float(factor) * phi[-1]


def potential_gradients(phi0, phiT):
    """``(grad_mu0, grad_mu1)``: the derivative of the cost in the end masses, mean-free: -(phi0 - mean), phiT - mean.  numpy arrays
    or torch tensors."""
    return -(phi0 - phi0.mean()), phiT - phiT.mean()


def stress_host(mu, phi, triangles, mass_v, factor_mu=1.0, factor_phi=1.0):
    """The stress (F, 3, 6) of ``mu`` (T, V) and ``phi`` (T + 1, V), in scalar floats.  Per (triangle f, corner k), with one
    accumulator per entry e = (a, b) that starts at +0.0, for t = 0, 1, ..., T - 1 in this order:

        x = factor_mu * mu[t][v_k];  m = x * mass_v[v_k]
        p_t[c] = factor_phi * phi[t][tri[f][c]]   (one multiplication per value, c = 0, 1, 2; likewise p_{t+1})
        q0 = p_t[a] * p_t[b];  q1 = p_{t+1}[a] * p_{t+1}[b];  s = q0 + q1;  w = 0.5 * s;  c = m * w;  acc[e] = acc[e] + c

    Nothing is fused (the library is built with -ffp-contract=off).  The kernel (csrc/kernels_sensitivity.hip) carries q1 of
    interval t over as q0 of interval t + 1: the same value."""
    mu, phi = np.asarray(mu, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    tri = np.asarray(triangles)
    T, F = mu.shape[0], tri.shape[0]
    if phi.shape != (T + 1, mu.shape[1]):
        raise ValueError(f"stress_host: mu (T, V) and phi (T + 1, V) expected, got {mu.shape} and {phi.shape}")
    fm, fp = float(factor_mu), float(factor_phi)
    mass = [float(x) for x in np.asarray(mass_v, dtype=np.float64)]
    mu_rows = [[fm * float(x) for x in mu[:, v]] for v in range(mu.shape[1])]          # [v][t]: x = factor_mu * mu
    phi_rows = [[fp * float(x) for x in phi[:, v]] for v in range(phi.shape[1])]      # [v][t]: p = factor_phi * phi
    out = np.empty((F, 3, 6))
    for f in range(F):
        vs = [int(v) for v in tri[f]]
        p = [phi_rows[v] for v in vs]
        q = [[p[a][t] * p[b][t] for t in range(T + 1)] for a, b in ENTRIES]            # q[e][t] = p_t[a] * p_t[b]
        for k in range(3):
            x_row, m_v = mu_rows[vs[k]], mass[vs[k]]
            acc = [0.0] * 6
            for t in range(T):
                m = x_row[t] * m_v
                for e in range(6):
                    s = q[e][t] + q[e][t + 1]
                    w = 0.5 * s
                    acc[e] = acc[e] + m * w
            out[f, k] = acc
    return out


def stress_numpy(mu, phi, triangles, mass_v, factor_mu=1.0, factor_phi=1.0):
    """``stress_host`` vectorised over the triangles and corners (the same operations on every element in the same order: the same
    bits), ``t`` ascending in a Python loop: what a caller without ``dots_sensitivity`` computes from the downloaded arrays."""
    mu, phi = float(factor_mu) * np.asarray(mu, dtype=np.float64), float(factor_phi) * np.asarray(phi, dtype=np.float64)
    tri = np.asarray(triangles)
    T = mu.shape[0]
    m = mu[:, tri] * np.asarray(mass_v, dtype=np.float64)[tri][None]                   # (T, F, 3)
    p = phi[:, tri]                                                                    # (T + 1, F, 3)
    ia, ib = [a for a, _ in ENTRIES], [b for _, b in ENTRIES]
    acc = np.zeros((tri.shape[0], 3, 6))
    q0 = p[0][:, ia] * p[0][:, ib]                                                     # (F, 6)
    for t in range(T):
        q1 = p[t + 1][:, ia] * p[t + 1][:, ib]
        w = 0.5 * (q0 + q1)
        acc = acc + m[t][:, :, None] * w[:, None, :]
        q0 = q1
    return acc


def _mesh_terms(vertices, triangles):
    """``(area_f (F,), area_v (V,), gram (F, 6))``: triangle areas, the summed incident areas of the vertices and hat[f][a] . hat[f][b]
    over ENTRIES."""
    from .geometry import hat_gradients

    tri = np.asarray(triangles)
    area, hat = hat_gradients(vertices, tri)
    area_v = np.zeros(np.asarray(vertices).shape[0])
    np.add.at(area_v, tri.reshape(-1), np.repeat(area, 3))
    gram = np.stack([np.einsum("fc,fc->f", hat[:, a], hat[:, b]) for a, b in ENTRIES], axis=1)
    return area, area_v, gram


def kinetic_energy(stress, vertices, triangles, n_time):
    """K(x) of the module docstring, in numpy: with mass_v = area_v / 3 the weight area_f / (3 mass_v[v_k]) is area_f / area_v[v_k]."""
    stress, tri = np.asarray(stress, dtype=np.float64), np.asarray(triangles)
    area, area_v, gram = _mesh_terms(vertices, tri)
    weight = area[:, None] / area_v[tri]                                               # (F, 3)
    form = np.einsum("fke,fe,e->fk", stress, gram, np.asarray(ENTRY_WEIGHT))           # sum over a, b of the symmetric tensor
    return float(np.sum(weight * 0.5 * form)) / float(n_time)


def kinetic_energy_torch(stress, vertices, triangles, n_time):
    """``kinetic_energy`` as a torch scalar (fp64), differentiable in ``vertices``: areas, vertex masses and hat gradients are formed
    from ``vertices`` in torch (the formulas of geometry.hat_gradients); ``stress`` is a constant."""
    import torch

    x = torch.as_tensor(vertices, dtype=torch.float64)
    tri = torch.as_tensor(np.asarray(triangles).astype(np.int64), device=x.device)
    s = torch.as_tensor(stress, dtype=torch.float64, device=x.device)
    p = x[tri]                                                                         # (F, 3, 3)
    area = 0.5 * torch.linalg.norm(torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 1]), dim=1)
    hat = []
    for k in range(3):
        a, b = p[:, (k + 1) % 3], p[:, (k + 2) % 3]
        e, w = b - a, p[:, k] - a
        alt = w - e * ((w * e).sum(1) / (e * e).sum(1))[:, None]
        hat.append(alt / (alt * alt).sum(1)[:, None])
    area_v = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device).index_add(0, tri.reshape(-1), area.repeat_interleave(3))
    gram = torch.stack([(hat[a] * hat[b]).sum(1) for a, b in ENTRIES], dim=1)           # (F, 6)
    weight = area[:, None] / area_v[tri]
    form = torch.einsum("fke,fe,e->fk", s, gram, torch.tensor(ENTRY_WEIGHT, dtype=torch.float64, device=x.device))
    return (weight * 0.5 * form).sum() / float(n_time)


def cost_gradients(sens, vertices, triangles):
    """``(grad_mu0 (V,), grad_mu1 (V,), grad_vertices (V, 3))`` of the transport cost from ``sens``, what ``AlmSolver.sensitivity``
    returns (``phi0``, ``phiT``, ``stress``, ``n_time``; numpy arrays or torch tensors): the mean-free potentials, and -dK/dx with the
    stress held fixed, by torch autograd on ``kinetic_energy_torch``.  A part that ``sens`` does not hold comes back as None.
    Returns numpy arrays."""
    import torch

    def host(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)

    g0 = g1 = gx = None
    if sens.get("phi0") is not None and sens.get("phiT") is not None:
        g0, g1 = potential_gradients(host(sens["phi0"]), host(sens["phiT"]))
    if sens.get("stress") is not None:
        with torch.enable_grad():      # (also inside the backward pass of torch_cost, where recording is off)
            x = torch.tensor(np.asarray(vertices, dtype=np.float64), requires_grad=True)
            K = kinetic_energy_torch(torch.as_tensor(host(sens["stress"])), x, triangles, sens["n_time"])
            gx = -torch.autograd.grad(K, x)[0].numpy()
    return g0, g1, gx

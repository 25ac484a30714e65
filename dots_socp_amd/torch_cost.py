"""The transport cost as a differentiable torch function: a loss in the end densities and in the shape.

``transport_cost`` solves one problem with ``solver_socp`` and returns its cost as a scalar tensor; the backward pass is
``sensitivity.cost_gradients`` on what ``dots_sensitivity`` reduced on the device at the end of the solve: the mean-free Kantorovich
potentials for ``mu0`` / ``mu1`` (the masses per vertex ``solver_socp`` takes) and minus the derivative of the kinetic energy at fixed
stress for ``vertices`` (envelope theorem; without congestion only).  The gradients are those of the converged problem: their error
is the solve's (``tol``) -- DESIGN.md section 9, "Cost gradients", has the measured finite differences.  ``transport_costs`` does
the same for a batch of densities on one surface through ``solver_socp_many``: one factor for all of them.
"""
from __future__ import annotations

import numpy as np
import torch

from . import meshes, sensitivity
from .socp.solver_socp import PER_PROBLEM_KEYS, solver_socp, solver_socp_many


def _host(a):
    return a.detach().cpu().numpy().astype(np.float64) if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)


def _request(needs):
    """The ``sensitivity`` request for the inputs (mu0, mu1, vertices) that need a gradient, or None."""
    if not any(needs[:3]):
        return None
    return {"potentials": bool(needs[0] or needs[1]), "stress": bool(needs[2])}


def _session_mesh(who, session, n_time, x, tri, move):
    """The refusals of a call on a session (``SolveSession``, ``BatchSession``): its time grid and its mesh, by value.  Returns the
    positions its live contexts move to (``move`` and the session's triangles at other positions), or None."""
    if int(n_time) != session.n_time:
        raise ValueError(f"{who}: n_time = {int(n_time)}, the session's {session.n_time}")
    same_tri = np.array_equal(tri, np.asarray(session.geometry["triangles"], dtype=np.int64))
    same_x = np.array_equal(x, np.asarray(session.geometry["vertices"], dtype=np.float64))
    if move and same_tri and not same_x:
        if x.shape != np.asarray(session.geometry["vertices"]).shape:
            raise ValueError(f"{who}: vertices must have the session's shape {np.asarray(session.geometry['vertices']).shape}, got {x.shape}")
        return x
    if not (same_x and same_tri):
        raise ValueError(f"{who}: vertices / triangles are not the session's (a session solves on one mesh; moved "
                         "vertices need a new session)" + (": move=True moves the vertices, the triangles must be the session's" if move else ""))
    return None


def _like(array, ref):
    return torch.as_tensor(np.ascontiguousarray(array), dtype=ref.dtype, device=ref.device)


class _TransportCost(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu0, mu1, vertices, triangles, n_time, options, session=None, move=False):
        x, tri = _host(vertices), np.asarray(_host(triangles), dtype=np.int64)
        if session is not None:      # the session's live context: the masses change, the mesh must be the session's
            moved = _session_mesh("transport_cost", session, n_time, x, tri, move)
            solution, hist = session.solve(mu0.detach(), mu1.detach(), outputs=(), sensitivity=_request(ctx.needs_input_grad), vertices=moved, **options)
        else:
            geom, _ = meshes.make_geometry(x, tri, _host(mu0), _host(mu1), normalize=False)      # the geometry as given
            solution, hist = solver_socp(int(n_time), geom, outputs=(), sensitivity=_request(ctx.needs_input_grad), **options)
        ctx.sens, ctx.mesh = solution.get("sensitivity"), (x, tri)
        ctx.like = (mu0, mu1, vertices)
        return torch.tensor(float(hist.history["Transportation cost"][-1]), dtype=torch.float64, device=mu0.device)

    @staticmethod
    def backward(ctx, g):
        g0, g1, gx = sensitivity.cost_gradients(ctx.sens, *ctx.mesh)
        grads = [None if a is None or not need else g.to(ref.device, ref.dtype) * _like(a, ref)
                 for a, need, ref in zip((g0, g1, gx), ctx.needs_input_grad[:3], ctx.like)]
        return (*grads, None, None, None, None, None)


def _tensor(a):
    return a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))


def transport_cost(mu0, mu1, vertices, triangles, n_time, session=None, move=False, **solver_options):
    """The transport cost between the masses ``mu0`` and ``mu1`` (V,) on the mesh (``vertices`` (V, 3), ``triangles`` (F, 3)) with
    ``n_time`` intervals, as a scalar fp64 tensor on ``mu0``'s device, differentiable in ``mu0``, ``mu1`` and ``vertices``.  Forward:
    one ``solver_socp`` call on the geometry as given (``meshes.make_geometry(..., normalize=False)``) with ``solver_options`` (tol,
    nit, ...); only what an input that requires a gradient needs is reduced.  Backward: ``sensitivity.cost_gradients``.  The
    gradients in the masses are mean-free (the cost is defined for equal total masses); the one in ``vertices`` needs congestion 0.
    ``session``: a ``socp.SolveSession`` on this mesh (``meshes.make_geometry(vertices, triangles, ..., normalize=False)``) and
    ``n_time``: the forward pass is ``session.solve`` on its live context -- no plan, factor or context is built again -- and
    ``solver_options`` are that call's (``warm``, ``tol``, ``nit``, ``time_limit``, ``congestion``); ``vertices`` / ``triangles`` must be
    the session's, by value.  With ``warm=False`` cost and gradients are those of the call without a session, bit for bit; the
    gradient in ``vertices`` is still the stress of the current geometry.
    ``move=True`` (with a session): ``vertices`` that differ from the session's by value move its live context
    (``SolveSession.solve(vertices=)``: tables and factor refreshed on the device; same shape, same triangles); equal positions do not
    move it.  With ``warm=False`` cost and gradients are those of a new solver on ``geometry.plan_with_vertices`` of the session's
    plan, bit for bit.  The default keeps the session on its mesh and refuses other positions."""
    for k in ("outputs", "read_out", "flow_map", "sensitivity"):
        if k in solver_options:
            raise ValueError(f"transport_cost: '{k}' is chosen by the function itself")
    if session is None and "warm" in solver_options:
        raise ValueError("transport_cost: 'warm' needs a session (a call without one starts from zero)")
    if session is None and move:
        raise ValueError("transport_cost: 'move' needs a session (a call without one builds its own solver on the mesh as given)")
    return _TransportCost.apply(_tensor(mu0), _tensor(mu1), _tensor(vertices), triangles, n_time, solver_options, session, bool(move))


class _TransportCosts(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu0, mu1, vertices, triangles, n_time, options, session=None, move=False):
        x, tri = _host(vertices), np.asarray(_host(triangles), dtype=np.int64)
        m0, m1 = _host(mu0), _host(mu1)
        if session is not None:      # the session's live contexts: the masses change, the mesh must be the session's
            moved = _session_mesh("transport_costs", session, n_time, x, tri, move)
            options = dict(options)
            warm = options.pop("warm", False)
            problems = [dict(options, mu0=a, mu1=b) for a, b in zip(m0, m1)]
            results = session.solve_many(problems, warm=warm, vertices=moved, outputs=(), sensitivity=_request(ctx.needs_input_grad))
        else:
            geom, _ = meshes.make_geometry(x, tri, m0[0], m1[0], normalize=False)
            each = {k: v for k, v in options.items() if k in PER_PROBLEM_KEYS}
            common = {k: v for k, v in options.items() if k not in PER_PROBLEM_KEYS}
            problems = [dict(each, mu0=a, mu1=b) for a, b in zip(m0, m1)]
            results = solver_socp_many(int(n_time), geom, problems, outputs=(), sensitivity=_request(ctx.needs_input_grad), **common)
        ctx.sens, ctx.mesh = [sol.get("sensitivity") for sol, _ in results], (x, tri)
        ctx.like = (mu0, mu1, vertices)
        return torch.tensor([float(hist.history["Transportation cost"][-1]) for _, hist in results], dtype=torch.float64, device=mu0.device)

    @staticmethod
    def backward(ctx, g):
        parts = [sensitivity.cost_gradients(s, *ctx.mesh) for s in ctx.sens]
        need, (r0, r1, rx) = ctx.needs_input_grad, ctx.like
        g0 = g.to(r0.device, r0.dtype)[:, None] * _like(np.stack([p[0] for p in parts]), r0) if need[0] else None
        g1 = g.to(r1.device, r1.dtype)[:, None] * _like(np.stack([p[1] for p in parts]), r1) if need[1] else None
        gx = (g.to(rx.device, rx.dtype)[:, None, None] * _like(np.stack([p[2] for p in parts]), rx)).sum(0) if need[2] else None
        return g0, g1, gx, None, None, None, None, None


def transport_costs(mu0, mu1, vertices, triangles, n_time, session=None, move=False, **solver_options):
    """``transport_cost`` for ``B`` pairs of masses on one surface: ``mu0`` and ``mu1`` (B, V); returns the costs (B,).  The problems
    run through ``solver_socp_many``: one factor of the direct solver, batched sweeps.  ``solver_options``: the per-problem options of
    ``solver_socp_many`` (tol, nit, congestion, ...) hold for every problem, the others (eps, device, max_batch, ...) for the batch.
    ``session``: a ``socp.BatchSession`` on this mesh (``meshes.make_geometry(vertices, triangles, ..., normalize=False)``) and
    ``n_time``: the forward pass is ``session.solve_many`` on its live contexts -- no plan, factor or context is built again once
    they exist -- and ``solver_options`` are ``warm`` and what one of its problems may hold (``tol``, ``nit``, ``tol_checkpoints``,
    ``time_limit``, ``congestion``); ``vertices`` / ``triangles`` must be the session's, by value.  With ``warm=False`` (the default)
    costs and gradients are those of the call without a session, bit for bit.  ``move=True`` (with a session): ``vertices`` that
    differ from the session's by value move its live contexts with one refresh of the factor (``BatchSession.solve_many(vertices=)``);
    costs and gradients are then those of the call on the moved mesh in the session's numbering.  The default keeps the session on
    its mesh and refuses other positions."""
    for k in ("outputs", "read_out", "flow_map", "sensitivity"):
        if k in solver_options:
            raise ValueError(f"transport_costs: '{k}' is chosen by the function itself")
    if session is None and "warm" in solver_options:
        raise ValueError("transport_costs: 'warm' needs a session (a call without one starts from zero)")
    if session is None and move:
        raise ValueError("transport_costs: 'move' needs a session (a call without one builds its own solvers on the mesh as given)")
    mu0, mu1 = _tensor(mu0), _tensor(mu1)
    if mu0.ndim != 2 or mu0.shape != mu1.shape or mu0.shape[0] < 1:
        raise ValueError(f"transport_costs: mu0 and mu1 (B, V) expected, got {tuple(mu0.shape)} and {tuple(mu1.shape)}")
    return _TransportCosts.apply(mu0, mu1, _tensor(vertices), triangles, n_time, solver_options, session, bool(move))

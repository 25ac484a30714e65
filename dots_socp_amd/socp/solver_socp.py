"""``solver_socp``: the reference's ALM driver with the numerics on the GPU.

Same signature, return contract and iteration-by-iteration decisions as
``dot_surface_socp/socp/solver_socp.py:25-871``; every array operation of the loop
(steps 1-3, KKT residuals, objective, scaling) runs in HIP kernels behind the C ABI
(``include/dots_socp_hip.h``), the state never leaves HBM between iterations and the host
only sees scalars.  Extra keyword arguments (all optional) select device-side choices:

    lap_solver   how step 1's Laplacian is solved: "modal_direct" (default; time eigen-modes + multifrontal Cholesky
                 sweeps, the reference's eigh + sparse-LU algorithm), "modal_pcg" (batched multigrid-PCG on the
                 modes) or "spacetime_pcg" (Jacobi-PCG on the coupled operator)
    cg_tol       relative PCG tolerance (default 1e-8; see DESIGN.md for the parity budget)
    cg_max_iter  PCG iteration cap
    device       HIP device ordinal
    reorder      locality renumbering of the mesh (default True)

There is no CPU path: without libdotsocp_hip.so and a GPU this raises.
"""
from __future__ import annotations

import logging
import math
import os
import time

import numpy as np

from ..control import (AdaptiveValidator, AdjustAdmmParam, ConditionValidator, ErrorCondition, RunningHistory, SampledStepTimers,
                       KKT_LABELS, KKT_SHORT_LABELS, max_of_list_with_none, safe_rescale_ratio)
from .. import _lib
from .._lib import env_choice
from ..device import DeviceProblem, STATE_NAMES
from ..sensitivity import check_sensitivity

logger = logging.getLogger("dots_socp_amd")

KKT_QUEUE_ORDER = [6, 2, 0, 3, 1, 4, 5]     # solver_socp.py:644
KKT_STOP, KKT_PRIM, KKT_DUAL = [0, 2, 4, 5], [0, 1], [2, 3]   # :299-301
PRIMAL = ("phi", "A", "B", "lambda_c")
Z_VARS = ("z_fst", "z_mid", "z_end")
DUAL_QE = ("mu", "E")
BETAS = ("beta_fst", "beta_mid", "beta_end")
DEFAULT_CG_TOL = 1e-8     # parity study: profiles/studies/cg_tol_parity.txt (cost within 1e-9 of the reference, budget 1e-6)
MODAL_PCG_MAX_NODES = 256     # T + 1 the modal PCG takes in one window, and time slabs at all (per-mode scalar block, slab layouts)
MAX_TIME_NODES = 1024         # T + 1 the library takes at all (modal_direct and spacetime_pcg on one GPU)


PCG_WINDOWS_ONE_SOLVER = ("pcg_windows belongs to solver_socp / AlmSolver on one GPU: {who} does not take it "
                          "(a batch shares the direct solver's factor, the levels of a cascade build theirs)")


def check_time_nodes(n_time, lap_solver="modal_direct", time_slab=None, pcg_windows=False):
    """Refuse, before any device call, what the library cannot run at ``n_time + 1`` time nodes: above 256 only the direct
    solver on one GPU (or spacetime_pcg) runs -- and, with ``pcg_windows=True``, the modal PCG on one GPU, in windows of 256 modes;
    above 1024 nothing does."""
    nodes = int(n_time) + 1
    if nodes > MAX_TIME_NODES:
        raise ValueError(f"n_time + 1 = {nodes} time nodes: at most {MAX_TIME_NODES} are supported")
    if pcg_windows and time_slab is not None:
        raise ValueError("pcg_windows is not available on time slabs: the windowed modal PCG runs on one GPU")
    if nodes > MODAL_PCG_MAX_NODES:
        if time_slab is not None:
            raise ValueError(f"time slabs need n_time + 1 <= {MODAL_PCG_MAX_NODES} (got {nodes}); run on one GPU with lap_solver='modal_direct'")
        if lap_solver == "modal_pcg" and not pcg_windows:
            raise ValueError(f"lap_solver='modal_pcg' needs n_time + 1 <= {MODAL_PCG_MAX_NODES} (got {nodes}); use lap_solver='modal_direct'")


FLOW_MAP_KEYS = ("starts", "floor", "max_crossings", "trajectory", "push", "span", "action", "slide")
FLOW_PUSH_KEYS = ("mass", "attributes", "layers")


def _check_flow_starts(starts):
    """``(kind, level)`` of a named choice of starts -- "vertices", "triangles", ("triangles", level) -- or None for ``(triangle, weights)``."""
    if isinstance(starts, str):
        if starts not in ("vertices", "triangles"):
            raise ValueError("flow_map: starts must be 'vertices', 'triangles', ('triangles', level) or (triangle, weights)")
        return starts, (1 if starts == "triangles" else None)
    if not isinstance(starts, (tuple, list)) or len(starts) != 2:
        raise ValueError("flow_map: starts must be 'vertices', 'triangles', ('triangles', level) or (triangle, weights)")
    if isinstance(starts[0], str):
        level = starts[1]
        if starts[0] != "triangles" or isinstance(level, bool) or not isinstance(level, (int, np.integer)) or level < 1:
            raise ValueError("flow_map: starts by name with a level must be ('triangles', level) with an integer level >= 1")
        return "triangles", int(level)
    return None


def _check_flow_span(span, action, n_time=None):
    """``None`` (today's trace over the whole horizon, no action), or ``(node_from, node_to)`` of a request with a span or the action
    (``action`` alone: ``(0, n_time)``, or ``(0, None)`` while ``n_time`` is not known)."""
    from ..flow import check_span

    if not isinstance(action, (bool, np.bool_)):
        raise ValueError("flow_map: action must be True or False")
    if span is None:
        return (0, None if n_time is None else int(n_time)) if action else None
    return check_span(span, n_time)


def _check_flow_push(push, starts, span=None, n_time=None):
    """``None``, or the request as a dict with all of FLOW_PUSH_KEYS (``True``: the masses of mu0 -- of mu1 where the span starts at the
    last node -- at the starts, the last layer).  ``span``: what ``_check_flow_span`` returned."""
    if push is None or push is False:
        return None
    if push is True:
        push = {}
    if not isinstance(push, dict):
        raise ValueError(f"flow_map: push must be None, True or a dict with any of {list(FLOW_PUSH_KEYS)}")
    unknown = set(push) - set(FLOW_PUSH_KEYS)
    if unknown:
        raise ValueError(f"flow_map: push: unknown option(s) {sorted(unknown)}; known: {list(FLOW_PUSH_KEYS)}")
    out = {"mass": push.get("mass"), "attributes": push.get("attributes"), "layers": push.get("layers", "end")}
    if not isinstance(out["layers"], str) or out["layers"] not in ("end", "all"):
        raise ValueError("flow_map: push: layers must be 'end' or 'all'")
    if out["attributes"] is not None:
        a = np.asarray(out["attributes"])
        if a.ndim != 2 or not 0 <= a.shape[0] <= 4:
            raise ValueError(f"flow_map: push: attributes (A, P) with A <= 4 expected, got {a.shape}")
    if out["mass"] is None and _check_flow_starts(starts) is None:
        raise ValueError("flow_map: push: starts given as (triangle, weights) need a mass per particle")
    if out["mass"] is None and span is not None and span[0] != 0:
        # (without n_time the start of a backward span cannot be told from the last node here: AlmSolver.flow_map checks again)
        if span[0] != int(n_time) if n_time is not None else span[1] > span[0]:
            raise ValueError(f"flow_map: push: a span from the interior node {span[0]} needs a mass per particle (the default is mu0 from "
                             "node 0 and mu1 from node n_time)")
    return out


def check_flow_map(flow_map, time_slab=None, n_time=None):
    """Refuse, before any device call, a ``flow_map`` request that cannot be served: ``None`` or the keywords of ``AlmSolver.flow_map``
    as a dict; never on a time slab (the particles are traced by one context, which holds every time node).  ``n_time``: where it is
    known the span is checked against it here, otherwise ``AlmSolver.flow_map`` does."""
    if flow_map is None:
        return None
    if time_slab is not None:
        raise ValueError("flow_map is not available on time slabs: the particles are traced on one GPU, which holds every time node")
    if not isinstance(flow_map, dict):
        raise ValueError(f"flow_map must be None or a dict with any of {list(FLOW_MAP_KEYS)}")
    unknown = set(flow_map) - set(FLOW_MAP_KEYS)
    if unknown:
        raise ValueError(f"flow_map: unknown option(s) {sorted(unknown)}; known: {list(FLOW_MAP_KEYS)}")
    if "starts" in flow_map:
        _check_flow_starts(flow_map["starts"])
    if not isinstance(flow_map.get("slide", False), (bool, np.bool_)):
        raise ValueError("flow_map: slide must be True or False")
    span = _check_flow_span(flow_map.get("span"), flow_map.get("action", False), n_time)
    _check_flow_push(flow_map.get("push"), flow_map.get("starts", "vertices"), span, n_time)
    return dict(flow_map)


def _validate_checkpoints(tol_checkpoints, tol):
    """solver_socp.py:85-94."""
    if tol_checkpoints is None:
        return None
    if not isinstance(tol_checkpoints, list) or not tol_checkpoints:
        raise ValueError("tol_checkpoints must be a non-empty list")
    for i, cp in enumerate(tol_checkpoints):
        if not (isinstance(cp, (int, float)) and 0 < cp < 1):
            raise ValueError(f"Invalid checkpoint value at index {i}: {cp}. Must be between 0 and 1")
        if cp < tol:
            raise ValueError(f"Checkpoint value must be greater than tol. However, checkpoint ({cp}) < tol ({tol})")
    return sorted(tol_checkpoints, reverse=True)


def _state_carrier(n_time, init_from, init_solution, time_slab, init_parents, init_transfer, init_regrid=False):
    """How a solver's state comes from ``init_from``, validated before any device call: None without ``init_from``, else ``carry(dev)``,
    which fills the DeviceProblem ``dev`` and returns the milliseconds -- in space over ``init_parents`` / ``init_transfer`` (with
    ``init_regrid`` also from another ``n_time``: space and time in one pass), else in time."""
    if init_transfer is not None and init_parents is not None:
        raise ValueError("init_transfer and init_parents are mutually exclusive: the level below is a located mesh or the parent mesh")
    space = None      # (option, which mesh init_from is on, the DeviceProblem method, its map)
    if init_parents is not None:
        space = ("init_parents", "parent", "prolong_space_from", init_parents)
    elif init_transfer is not None:
        space = ("init_transfer", "coarse", "transfer_space_from", init_transfer)
    if init_regrid and space is None:
        raise ValueError("init_regrid needs init_parents or init_transfer: on one mesh init_from alone changes the time grid")
    if init_from is None:
        if space:
            raise ValueError(f"{space[0]} needs init_from (the solver on the {space[1]} mesh)")
        return None
    if init_solution:
        raise ValueError("init_from and init_solution are mutually exclusive: the warm start comes from one of them")
    if time_slab is not None:
        raise ValueError("init_from is not available on time slabs")
    if not getattr(init_from, "finalized", False):
        raise ValueError("init_from must have been finalised (finalize(download=False) is enough)")
    if space is None:
        return lambda dev: dev.prolong_from(init_from.dev, init_from.recovery_factors())
    option, mesh, method, table = space
    if int(init_from.n_time) != int(n_time):
        if init_regrid:      # (the fused carrier; on one time grid the carrier in space below is the definition)
            maps = {"parents": table} if option == "init_parents" else {"transfer": table}
            return lambda dev: dev.carry_spacetime_from(init_from.dev, init_from.recovery_factors(), **maps)
        raise ValueError(f"{option}: the {mesh} mesh's solver has n_time = {int(init_from.n_time)}, this one {int(n_time)}: "
                         "one call changes the mesh or the time grid, not both")
    return lambda dev: getattr(dev, method)(init_from.dev, table, init_from.recovery_factors())


class AlmSolver:
    """The reference's solver as an object: ``__init__`` = setup (solver_socp.py:96-652),
    ``iterate()`` = one pass of the main loop (:656-823), ``finalize()`` = :826-871.

    The scalars the reference keeps in closure variables (r, prim/dual scale, constant_d,
    scale_factor_z, congestion, norm constants) live here on the host and are pushed to the
    device context whenever they change; arrays live on the device only.
    """

    def __init__(self, n_time, geometry, congestion=0.0, nit=1000, eps=0.0, tol=1e-4, tau=1.90, is_z_scaling=True,
                 is_constant_scaling=False, check_kkt_step_by_step=False, init_solution=None, tol_checkpoints=None,
                 time_limit=1000, is_palm=False, lap_solver="modal_direct", cg_tol=DEFAULT_CG_TOL, cg_max_iter=20000, device=0, reorder=True,
                 preconditioner="multigrid", mg_coarsest=256, time_slab=None, nd_leaf=16, plan=None, front_owner=None, init_from=None,
                 release_init_from=False, batched=None, init_parents=None, init_transfer=None, init_regrid=False, pcg_windows=False):
        """``plan``: the device plan to use (geometry.plan_with_densities) instead of building one; ``front_owner``: a DeviceProblem
        whose factor this solver shares (dots_front_share) instead of building its own -- a member of a batch (solver_socp_many), stepped
        by ``step_batch``; the launch ahead of the right-hand side and of the penalty decision are off then.
        ``init_from``: a finalised AlmSolver of the same mesh on the same device at another ``n_time`` (a coarser level of a cascade):
        its recovered solution, interpolated linearly in time on the device (DeviceProblem.prolong_from), is the warm start -- what
        ``init_solution=cascade.prolong_solution(<its solution>, ...)`` does over the host, bit for bit.  The state is transferred before
        this solver's factor is built; ``release_init_from`` closes the coarse solver right after the transfer, so that the two factors
        are never on the device together.  ``init_parents``: ``init_from`` is a solver on the PARENT mesh of this one (``meshes.subdivide``'s
        ``parents``) at the same ``n_time``: its recovered solution is carried to the refinement on the device
        (DeviceProblem.prolong_space_from; ``init_solution=cascade.prolong_space_solution(<its solution>, parents)`` bit for bit).  One call
        changes the mesh or the time grid, not both.  ``init_transfer`` (exclusive with ``init_parents``): ``init_from`` is a solver on ANOTHER
        triangulation of the same surface at the same ``n_time`` and this is ``cascade.mesh_transfer`` from its mesh to this one: its
        recovered solution is carried over barycentrically on the device (DeviceProblem.transfer_space_from;
        ``init_solution=cascade.transfer_space_solution(<its solution>, transfer)`` bit for bit), in the same order: transfer, release,
        factor.  ``init_regrid=True`` (with ``init_parents`` or ``init_transfer``) allows ``init_from`` at ANOTHER ``n_time``: mesh and time
        grid change in one pass on the device (DeviceProblem.carry_spacetime_from; ``init_solution=cascade.carry_spacetime_solution(<its
        solution>, ...)`` bit for bit: space first, then time); at the same ``n_time`` it changes nothing.  ``batched``: whether the solver is stepped by a batch (default: whenever ``plan`` or
        ``front_owner`` is given).  ``pcg_windows``: above 256 time nodes the modal PCG solves the modes in windows of 256
        (DeviceProblem.enable_pcg_windows): ``lap_solver="modal_pcg"`` then takes ``n_time + 1 <= 1024`` on one GPU, and ``modal_direct``
        falls back to it there too when the factor does not fit."""
        check_time_nodes(n_time, lap_solver, time_slab, pcg_windows)
        if pcg_windows and (front_owner is not None or plan is not None):
            raise ValueError(PCG_WINDOWS_ONE_SOLVER.format(who="a member of a batch"))
        carry = _state_carrier(n_time, init_from, init_solution, time_slab, init_parents, init_transfer, init_regrid)
        self.tol_checkpoints = _validate_checkpoints(tol_checkpoints, tol)
        self.geometry = geometry        # (read_out takes the area weights and mu0 / mu1 from it)
        self.checkpoint_solutions = []
        self.move_ms = None             # device milliseconds of the last restart's move of the vertices (restart(vertices=)); None: it moved nothing
        self.n_time, self.nit, self.tol, self.time_limit = int(n_time), int(nit), tol, time_limit
        self.is_z_scaling, self.is_constant_scaling = is_z_scaling, is_constant_scaling
        self.check_kkt_step_by_step = check_kkt_step_by_step
        self.is_palm = bool(is_palm)      # an extra (q, lambda_c) solve opens every iteration (solver_socp.py:668-672)
        self.direct = direct = lap_solver == "modal_direct"
        self.untimed_steps = 0          # iterations whose phases were not timed (run_history.steps_time is estimated from the others)
        self.quiet_steps = 0            # iterations after which nothing was read back
        self._timed_in_flight = []      # kinds of the timed iterations whose events have not been collected yet (one entry per slot)
        # the right-hand side + cone projection of the iteration after a read-back may be enqueued ahead (iterate(); DOTS_RHS_AHEAD=0
        # never).  Round 2 only did so on small problems (the projection then ran apart from the right-hand side: one launch more);
        # the projection now rides in the launch ahead, its results in alternate buffers until the step takes them: the same launch
        # the iteration would start with, only earlier -- on for every size
        ahead = env_choice("DOTS_RHS_AHEAD", ("0", "1", "2"), "1")
        self.batched = (front_owner is not None or plan is not None) if batched is None else bool(batched)
        self._rhs_ahead_ok = (direct and time_slab is None and not self.is_palm and not check_kkt_step_by_step
                              and not is_constant_scaling and ahead != "0" and not self.batched)
        self._rhs_ahead = False
        self._carry = False             # DOTS_STEP_CARRY for the next device step (iterate())
        # (on at every size: where the launches are latency-bound the bytes saved in the right-hand side / projection only balance
        # what the exchange through LDS costs steps 2+3)
        self._carry_ok = direct and not self.is_palm
        self._fused_kkt = False         # the last device step formed the KKT sums it holds in registers (DOTS_STEP_KKT_SUMS)
        if direct and reorder is True:
            reorder = "nd"      # the elimination order of the factor doubles as the locality numbering
        self.dev = dev = DeviceProblem(n_time, geometry, lap_solver="modal_pcg" if direct else lap_solver, device=device,
                                       reorder=reorder, time_slab=time_slab, nd_leaf=nd_leaf, plan=plan, pcg_windows=bool(pcg_windows))

        self.tau, self.eps = float(tau), float(eps)
        self._init_from = init_from is not None      # (a level of a cascade: ``restart`` refuses it)

        def install():
            """What only a new solver does between the first push of the parameters and the start of the run: the state carried from
            ``init_from``, the factor or the hierarchy, the initial state.  Returns the ``init_solution`` the constant scaling reads."""
            nonlocal direct
            if preconditioner not in ("multigrid", "jacobi"):
                raise ValueError("preconditioner must be 'multigrid' or 'jacobi'")
            self.prolong_ms = None          # device milliseconds of the transfer from ``init_from``
            if carry is not None:
                self.prolong_ms = carry(dev)
                if release_init_from:
                    init_from.close()
            self.mg_summary = self.front_summary = None
            self.lap_solver_fallback = None      # why the direct solve was not used although it was asked for
            if direct and front_owner is not None:
                self.front_summary = dev.share_frontal(front_owner)      # (no fall-back: a batch shares the factor or fails)
            elif direct:
                # Memory regime: the factor holds ~70 entries per vertex and time mode (8.9 GB at 500k vertices x 32 modes).  When it
                # does not fit beside the state, step 1 runs the batched multigrid-PCG on the same modes instead -- the reference has
                # no counterpart (laplacian_inverse_socp.py:34-41 just factorises); the choice is logged and reported in solver_stats.
                try:
                    self.front_summary = dev.setup_frontal(eps=self.eps)
                except _lib.HipLibraryError as exc:
                    if exc.status != _lib.ERR_MEMORY or time_slab is not None or (int(n_time) + 1 > MODAL_PCG_MAX_NODES and not pcg_windows):
                        raise      # (above 256 time nodes only the windowed PCG is there to fall back to: without it the error names the sizes)
                    self.lap_solver_fallback = str(exc)
                    logger.warning("modal_direct -> modal_pcg with the multigrid preconditioner: %s", exc)
                    self.direct = direct = False
                    self._rhs_ahead_ok = False
                    if preconditioner == "multigrid":
                        self.mg_summary = dev.setup_multigrid(eps=self.eps, coarsest=mg_coarsest)
            elif preconditioner == "multigrid" and lap_solver == "modal_pcg":
                self.mg_summary = dev.setup_multigrid(eps=self.eps, coarsest=mg_coarsest)
            init = init_solution or {}
            if init_from is None:
                self._upload_initial_state(init)
            elif is_constant_scaling:
                init = {"phi": dev.download("phi")}      # (_initial_constant_scaling borrows phi's storage and puts this back)
            return init

        self._start_run(congestion, cg=(cg_tol, int(cg_max_iter)), install=install)

    def _start_run(self, congestion, cg=None, install=None, keep_phi=False):
        """The start of a run on ``self.dev``, which holds its initial state or receives it from ``install()``: the host scalars of a
        new context (``dev.params``), their push, the history, the timers, the validator, ``prim_gap``, the initial z scaling and the
        constant scaling.  ``__init__`` runs it with ``cg`` (the PCG's tolerance and cap, set once) and ``install``; ``restart`` runs it
        on the context ``dots_restart`` has reset, with ``keep_phi`` where the state is a warm start."""
        dev, is_z_scaling, is_constant_scaling = self.dev, self.is_z_scaling, self.is_constant_scaling
        p = dev.params
        self.r = 1.0
        self.prim_scale = self.dual_scale = self.boundary_scale = 1.0
        self.const_d = self.scale_z = 1.0
        self.norm_d, self.norm_boundary = p.norm_d, p.norm_boundary
        self.congestion0 = float(congestion)
        self.congestion = float(congestion)
        if cg is not None:
            dev.set_params(cg_tol=cg[0], cg_max_iter=cg[1])
        self._push()
        if install is not None:
            init_solution = install()
        else:      # (a warm restart left the recovered iterate in place; the constant scaling borrows phi's storage and puts this back)
            init_solution = {"phi": dev.download("phi")} if is_constant_scaling and keep_phi else {}

        self.run_history = RunningHistory(max_record_numbers=self.nit, kkt_labels=KKT_LABELS,
                                          kkt_short_labels=KKT_SHORT_LABELS, name="SOCP")
        # per-step timers without a host wait in the loop (control.SampledStepTimers); DOTS_TIME_EVERY=1 times every iteration.
        # The five events of a timed iteration cost ~30 us of stream time at knot (measured on the driver's 20-step window:
        # 8 190 it/s without sampling, 7 870 with the first 4 + every 8th of a kind, profiles/tools/driver_window.py): the first 2
        # of a kind and every 32nd are sampled (< 1 % of a 95-us iteration)
        self.step_timers = SampledStepTimers(self.run_history, first=2, every=int(env_choice("DOTS_TIME_EVERY", None, "32", integer=(1, 1 << 20))))
        self.adjust_params = AdjustAdmmParam()
        self.is_org_kkt = False
        self.cg_total = self.cg_fail = 0
        self.counter_main = -1
        self.finished = False
        self.finalized = False

        self.run_history.start()
        self.prim_gap = 1.0 + 1.0 * math.exp(-100 * congestion)      # :568
        if is_z_scaling:
            self.scale_variable_z(2.0, msg="Initially scale z")          # :571-572
        if is_constant_scaling:
            self._initial_constant_scaling(init_solution)                # :574-586

        self._kkt_cache = {}
        conditions = [ErrorCondition((lambda i=i: self._kkt_value(i)), self.tol, KKT_SHORT_LABELS[i]) for i in range(7)]
        self.kkt_validator = AdaptiveValidator(ConditionValidator(conditions, KKT_QUEUE_ORDER))   # :589-645
        self.start_time = time.perf_counter()

    # ---- parameters ------------------------------------------------------------------------
    def _push(self):
        self.dev.set_params(r=self.r, scale_z=self.scale_z, const_d=self.const_d, norm_d=self.norm_d,
                            norm_boundary=self.norm_boundary, congestion=self.congestion, tau=self.tau, eps=self.eps,
                            prim_scale=self.prim_scale, dual_scale=self.dual_scale, boundary_scale=self.boundary_scale)

    def _upload_initial_state(self, init):
        """solver_socp.py:239-250: missing entries default to zero / to the derived expressions."""
        dev, r = self.dev, self.r
        if not init:
            return   # device state is zero-initialised: phi = 0 -> A = B = 0, all multipliers 0
        unknown = set(init) - set(STATE_NAMES) - {"checkpoints"}
        if unknown:
            raise ValueError(f"unknown init_solution entries: {sorted(unknown)}")
        have = {k: np.asarray(v, dtype=np.float64) for k, v in init.items() if k in STATE_NAMES and v is not None}
        phi = have.get("phi", np.zeros(dev.shape("phi")))
        dev.upload("phi", phi)
        dev.upload("A", have["A"] if "A" in have else dev.apply_operator("grad_time", phi))
        dev.upload("B", have["B"] if "B" in have else dev.apply_operator("grad_space", phi))
        for k in ("lambda_c", "z_fst", "z_end", "z_mid"):
            if k in have:
                dev.upload(k, have[k])
        betas = {k: (1.0 / r) * have.get(k, np.zeros(dev.shape(k))) for k in BETAS}
        for k in BETAS:
            dev.upload(k, betas[k])
        mu = (1.0 / r) * (have["mu"] if "mu" in have else r * (betas["beta_fst"] - betas["beta_end"]))
        dev.upload("mu", mu)
        if "E" in have:
            dev.upload("E", (1.0 / r) * have["E"])
        else:
            dev.upload("E", -dev.apply_operator("decouple_adjoint", betas["beta_mid"], 1.0))

    # ---- scaling tools (solver_socp.py:324-412) -------------------------------------------
    def adjust_penalty(self, factor):
        self._kkt_cache = {}
        self.r *= factor
        self.dev.adjust_penalty(factor)
        self._push()

    def scale_variable_z(self, scale_factor, msg="Scale z"):
        logger.log(12, "%s with z factor: %s", msg, scale_factor)
        self._kkt_cache = {}
        self.scale_z *= scale_factor
        self.const_d *= scale_factor
        self.norm_d *= scale_factor
        # the reference multiplies by the *cumulative* factor (:383-384)
        self.dev.scale_z(self.scale_z, 1.0 / self.scale_z, self.scale_z)
        self._push()

    def scale_prim_dual(self, scale_factor=None):
        self._kkt_cache = {}
        dev = self.dev
        if scale_factor is None:
            names = [("phi", 1), ("phi", 2), ("A", 0), ("B", 0), ("z_fst", 0), ("z_mid", 0), ("z_end", 0), ("mu", 0), ("E", 0),
                     ("beta_fst", 0), ("beta_mid", 0), ("beta_end", 0)]
            n2 = dict(zip(names, self._norm_squares(names)))
            prim = [
                math.sqrt(n2["phi", 1] + n2["phi", 2]),
                math.sqrt(n2["A", 0] + n2["B", 0]),
                math.sqrt(n2["z_fst", 0] + n2["z_mid", 0] + n2["z_end", 0]),
            ]
            dual = [
                self.r * math.sqrt(n2["mu", 0] + n2["E", 0]),
                self.r * math.sqrt(n2["beta_fst", 0] + n2["beta_mid", 0] + n2["beta_end", 0]),
            ]
            prim_rescale, dual_rescale = AdjustAdmmParam.compute_scale_factor(prim, dual)
        else:
            prim_rescale, dual_rescale = scale_factor
        if max(prim_rescale, dual_rescale) / min(prim_rescale, dual_rescale) > 2.0:
            self.prim_scale *= prim_rescale
            self.dual_scale *= dual_rescale
            dev.scale_arrays(PRIMAL + Z_VARS, 1.0 / prim_rescale)
            dual_factor = dual_rescale ** 2 / prim_rescale
            dev.scale_arrays(DUAL_QE + BETAS, 1.0 / dual_factor)
            # the boundary term is divided by dual_factor while r is multiplied by dual/prim; the device
            # rebuilds the boundary from r, so only the remaining 1/dual goes into boundary_scale
            self.boundary_scale /= dual_rescale
            self.r *= dual_rescale / prim_rescale
            self.congestion *= dual_rescale / prim_rescale
            self.const_d /= prim_rescale
            self.norm_d /= prim_rescale
            self.norm_boundary /= dual_rescale
            self._push()

    def _initial_constant_scaling(self, init_solution):
        dev, n_time = self.dev, self.n_time
        h = 1.0 / n_time
        plan = dev.plan
        inv = np.arange(dev.V)
        if plan.perm_vert is not None:
            inv = np.empty(dev.V, dtype=np.int64)
            inv[plan.perm_vert] = np.arange(dev.V)
        mass, mu0, mu1 = plan.mass_vert[inv], plan.mu0[inv], plan.mu1[inv]
        bt = np.zeros((n_time + 1, dev.V))        # r * boundary / mass at r = 1
        bt[0], bt[-1] = -mu0 / (h * mass), mu1 / (h * mass)
        norm_c = math.sqrt(float(np.sum(bt ** 2 * mass[None, :])) / (n_time + 1))
        norm_ac = self._boundary_gradient_norm(bt, init_solution.get("phi"))
        self.scale_prim_dual(scale_factor=(self.norm_d, math.sqrt(n_time) * norm_c ** 2 / norm_ac))
        self.adjust_penalty(1.0 / self.r)

    def _boundary_gradient_norm(self, bt, phi0):
        """sqrt(|d_t b|^2 + |d_x b|^2) of the boundary term (:574-586): the device's own operators on an uploaded copy."""
        dev = self.dev
        dev.upload("phi", bt)
        norm_ac = math.sqrt(dev.norm_square("phi", 1) + dev.norm_square("phi", 2))
        dev.upload("phi", np.zeros_like(bt) if phi0 is None else np.asarray(phi0, dtype=np.float64))
        return norm_ac

    def _norm_squares(self, requests):
        """norm_square_* (:875-878) of the listed (array, part) pairs; the multi-GPU solver adds the slabs' shares."""
        return [self.dev.norm_square(name, part) for name, part in requests]

    def recovery_factors(self):
        """The four factors of ``recovered``: (phi, A, B, lambda_c), the z arrays, (mu, E), the beta arrays."""
        return (self.prim_scale, self.prim_scale / self.scale_z, self.r * self.dual_scale, self.r * self.scale_z * self.dual_scale)

    def recovered(self, name, arr):
        """recorver_scaled_solution (:397-405)."""
        if name in PRIMAL:
            return self.prim_scale * arr
        if name in Z_VARS:
            return (self.prim_scale / self.scale_z) * arr
        if name in DUAL_QE:
            return (self.r * self.dual_scale) * arr
        return (self.r * self.scale_z * self.dual_scale) * arr

    # ---- KKT residuals of the current iterate, evaluated at most once each: the conditions an iteration is known to need
    # (the four primal / dual ones before a penalty update, all seven in step-by-step mode and at the end) are fetched in
    # ONE device call (one pass of the KKT kernels, one host round trip) instead of one call per condition
    # After a step with DOTS_STEP_KKT_SUMS the conditions FUSED_KKT cost no pass over the state (their sums were formed by steps
    # 2+3) and Dual(alpha) one vertex pass: whatever of them the lazy validator may ask for next (its queue runs 6, 2, 0, 3, 1)
    # comes with the first round trip.  Which values the validator LOOKS at -- and so the NaN pattern of the history -- is
    # unchanged: the cache only holds more than was asked for.  Conditions 4 and 5 gather over corner lists and keep their own pass.
    FUSED_KKT = (0, 1, 3, 6)

    def _widen(self, conditions):
        want = set(conditions)
        if not self._fused_kkt or want & {4, 5}:
            return list(conditions)
        if want & {2, 6}:      # (6 passes whenever there is no congestion, and 2 follows it in the queue)
            want.add(2)
        want.update(self.FUSED_KKT)
        return sorted(want - set(self._kkt_cache))

    def _kkt_value(self, i):
        if i not in self._kkt_cache:
            self._kkt_cache.update(self._kkt(self._widen([i])))
        return self._kkt_cache[i]

    def _kkt_prefetch(self, conditions):
        missing = [i for i in conditions if i not in self._kkt_cache]
        if missing:
            self._kkt_cache.update(self._kkt(self._widen(missing)))

    # ---- what the multi-GPU solver overrides: everything that reads numbers or arrays back from the device(s)
    def _kkt(self, conditions):
        return self.dev.kkt(conditions)

    def _objective(self):
        return self.dev.objective()

    def _download(self, name):
        """The whole array ``name`` in the reference layout."""
        return self.dev.download(name)

    def _read_out(self, factor, w_vertex=None, w_triangle=None, centred=False, mu0=None, mu1=None, sums=False):
        """``(mu, E, info)`` of the current iterate, formed on the device (DeviceProblem.readout; readout.read_out_host is the
        specification) -- one call, and only these two arrays cross to the host; ``info``: layer sums, device ms and bytes."""
        dev = self.dev
        mu, E, mass, neg = dev.readout(factor, w_vertex, w_triangle, centred, mu0, mu1, sums=sums)
        return mu, E, {"layer_mass": mass, "layer_negative": neg, "ms": dev.readout_ms, "bytes": dev.readout_bytes}

    def _device_step(self, quiet=False):
        """Steps 1-3 on the device; the multi-GPU solver overrides this with begin / all-gather / end.

        ``quiet``: nothing is read back after this iteration (no KKT evaluation, not the last one): z_mid
        need not be stored, and with the direct solver the host does not wait for the device either."""
        # is_palm's step 0 reads z_mid of the previous iteration: it is stored every iteration then
        # With the direct solver an iteration needs no host round trip: it is only enqueued, and on iterations that read
        # back the KKT kernels follow it on the stream (one wait, at the read-back).  The phase timers of the history
        # (Step 1-1 ...) come from SAMPLED iterations whose phases are bracketed by events on the stream, collected at the
        # next read-back and scaled to all iterations of their kind (control.SampledStepTimers).
        kind = "quiet" if quiet else "read-back"
        sample = self.step_timers.begin(kind)
        if quiet:
            self.quiet_steps += 1
        if self.direct:
            timed = sample and len(self._timed_in_flight) < 60       # (the ring of the library holds 64 slots)
            self.dev.step_flags(skip_z_mid=quiet and not self.is_palm, palm=self.is_palm, rhs_ahead=self._rhs_ahead and not quiet, timed=timed,
                                carry=self._carry, kkt_sums=not quiet)
            self._fused_kkt = not quiet
            try:
                self.dev.step(1, wait=False)
            except Exception:
                # the library gave the timing slot of a failed step back: what this side still expects of the ring can no longer
                # be matched to kinds -- drop it, so that the error that surfaces is the step's own
                self._timed_in_flight.clear()
                raise
            if timed:
                self._timed_in_flight.append(kind)
            else:
                self.untimed_steps += 1
        else:       # the PCG waits for its convergence flags anyway: every iteration is timed
            self.dev.step_flags(skip_z_mid=quiet and not self.is_palm, palm=self.is_palm)
            self._account(self.dev.step(1), kind)

    def batch_step_prepare(self, quiet):
        """A batch member's share of ``_device_step``: its step flags (the batch enqueues the step itself, step_batch); returns
        (kind, sampled)."""
        kind = "quiet" if quiet else "read-back"
        sample = self.step_timers.begin(kind)
        if quiet:
            self.quiet_steps += 1
        self.dev.step_flags(skip_z_mid=quiet and not self.is_palm, palm=self.is_palm, carry=self._carry, kkt_sums=not quiet)
        self._fused_kkt = not quiet
        return kind, sample

    def _collect_step_times(self, wait=False):
        """Phase times of the timed iterations that have finished (at a read-back: all of them), into the history."""
        fresh = False
        if self._timed_in_flight:
            for st in self.dev.step_times(wait=wait):
                self._account(st, self._timed_in_flight.pop(0))
                fresh = True
        if fresh or wait:       # (the estimate also scales with the iteration counts: brought up to date whenever it is asked for with wait=True)
            self.step_timers.publish()

    def _time_is_up(self, reads_back=True):
        """``reads_back``: this iteration synchronises with the host anyway (the multi-GPU driver only shares the
        clock decision on those iterations)."""
        return (time.perf_counter() - self.start_time) > self.time_limit

    def _account(self, st, kind):
        """One dots_step_stats (a whole iteration, or one stage of a time slab: the iteration is complete with the record that
        carries alm_iterations = 1) of an iteration of ``kind`` into the sampled timers."""
        tm = self.step_timers
        self.cg_total += st.cg_iterations
        self.cg_fail += st.cg_not_converged
        done = int(st.alm_iterations)
        tm.add(kind, "Step 1-1 (Laplacian)", 1e-3 * (st.ms_rhs + st.ms_laplacian), done)
        tm.add(kind, "Step 1-2 (SOC-Projection)", 1e-3 * st.ms_soc, done)
        tm.add(kind, "Step 2+3 (Q & Lambda, Multiplier)", 1e-3 * st.ms_q_lambda_multiplier, done)

    # ---- one pass of the main loop (:656-823); returns True when the loop must stop ------------
    def iterate(self):
        quiet = self.iterate_begin()
        if quiet is None:
            return True
        self._device_step(quiet)                                                # steps 1-3 (:674-722)
        return self.iterate_end()

    def iterate_begin(self):
        """The part of ``iterate()`` before the device step: returns whether the step is quiet (nothing read back after it), or
        None when the solver has finished."""
        if self.finished:
            return None
        self.counter_main += 1
        it, dev, hist, params = self.counter_main, self.dev, self.run_history, self.adjust_params
        if self.is_constant_scaling and params.is_to_scale(it):
            self.scale_prim_dual()
        if self.is_z_scaling and params.is_to_scale_matrix(it, hist.get_current_kkt_errors()):
            rescale_z = safe_rescale_ratio(self.prim_gap, hist.get_current_kkt_errors())
            if rescale_z > 1.25:
                self.scale_variable_z(rescale_z, msg=f"Rescale z at iteration {it}")

        # The reference looks at the clock after the step (:725); here before it, so that it is known in advance whether
        # this iteration's results are read back (a wall-clock limit has no parity to keep).
        validator = self.kkt_validator
        reads_back = (self.check_kkt_step_by_step or it + 1 >= self.nit or params.peek_adjust(it) or validator.will_validate_next()
                      or (self.is_constant_scaling and params.is_to_scale(it + 1)))   # the next iteration opens with norms of z
        is_time_used_up = self._time_is_up(reads_back)
        quiet = not (is_time_used_up or reads_back)
        self._kkt_cache = {}
        # An iteration that reads residuals back but changes nothing afterwards (no penalty update: that is known from the
        # schedule) is followed by an iteration that starts from the state it leaves, unless the run stops or z is rescaled:
        # the device starts on that iteration's right-hand side while the host waits for the residuals (DOTS_STEP_RHS_AHEAD;
        # dropped by the library if anything changes in between).
        self._rhs_ahead = (self._rhs_ahead_ok and reads_back and not is_time_used_up and it + 1 < self.nit
                           and not params.peek_adjust(it))
        # The next iteration starts from the state this one leaves unless the penalty is updated in between (known from the schedule;
        # a z rescaling or a stop simply drop what was carried): steps 2+3 then also store the per-corner sums that iteration's
        # right-hand side and cone projection would gather from B, E and beta_mid (DOTS_STEP_CARRY: one pass over beta_mid less).
        self._carry = self._carry_ok and it + 1 < self.nit and not params.peek_adjust(it)
        self._pass = (it, is_time_used_up, quiet)
        self._last_quiet = quiet        # (a quiet step stores no z_mid: ``restart(warm=True)`` needs the iterate of a read-back)
        return quiet

    def iterate_end(self):
        """The part of ``iterate()`` after the device step; returns True when the loop must stop."""
        (it, is_time_used_up, quiet), self._pass = self._pass, None
        hist, params = self.run_history, self.adjust_params
        adjust = params.is_to_adjust(it) or is_time_used_up
        required = KKT_PRIM + KKT_DUAL if adjust else None
        validator = self.kkt_validator

        history = None
        if not self.check_kkt_step_by_step:
            if adjust:
                validator.reset_counter()
                if self._rhs_ahead_ok and not is_time_used_up and it + 1 < self.nit:
                    # the library takes the decision below itself as soon as the residuals have arrived and starts the next iteration's
                    # first launch with it, while this side is still on its way there (dots_penalty_ahead; confirmed -- or dropped -- by the
                    # adjust_penalty / set_params calls further down: results never depend on it)
                    self.dev.penalty_ahead(self.tol, self.is_org_kkt, params._sigma_lower_bound, params._sigma_upper_bound, params.FACTOR_STEPS)
                self._kkt_prefetch(required)
            passed, _info = validator.validate(required)
            org, scaled = validator.collect()
            if adjust:
                validator.reset_counter()
        else:
            self._kkt_prefetch(range(7))
            passed, _info = validator.validator.validate(list(range(7)))
            org, scaled = validator.collect()
            cost, lagr = self._objective()
            history = {"Transportation cost": cost, "Objective value": lagr}
        error = max_of_list_with_none([org[i] for i in KKT_STOP])

        cps = self.tol_checkpoints
        if cps and error is not None and error <= cps[0]:                      # :790-801
            cp_mu, cp_E, _ = self._read_out(self.r * self.dual_scale)
            self.checkpoint_solutions.append({
                "mu": cp_mu,
                "E": cp_E,
                "iteration": it, "time": hist.get_running_time(), "kkt": np.array(org, dtype=object),
            })
            cps.pop(0)

        stop = passed or is_time_used_up
        if stop or it + 1 >= self.nit:
            self.finished = True
        if not stop:
            max_scaled = max_of_list_with_none(scaled)
            if max_scaled is not None and max_scaled < 5 * self.tol:
                self.is_org_kkt = True
            if adjust:                                                         # :813-823
                # enqueued BEFORE the records below are written (the reference records first, :776-789): nothing the records
                # hold depends on it, and the device divides its arrays while the host does its bookkeeping
                src = org if self.is_org_kkt else scaled
                prim_error = max_of_list_with_none([src[i] for i in KKT_PRIM])
                dual_error = max_of_list_with_none([src[i] for i in KKT_DUAL])
                self.adjust_penalty(params.get_updated_value(self.r, prim_error / dual_error) / self.r)
        hist.record(current_it=it, kkt_errors=org, history=history)
        if not quiet:
            self._collect_step_times()      # (the read-back above waited for the stream: every timed iteration so far is complete)
        if not self.check_kkt_step_by_step and error is not None:
            validator.set_error_and_tolerance(error, self.tol)
        return self.finished

    # ---- final record and solution (:826-871) ------------------------------------------------
    def read_out(self, dot_units=True, centred=True):
        """``({"mu", "E"}, info)``: the recovered ``mu`` and ``E`` (solver_socp.py:397-405) through the read-out --
        ``dot_units``: as masses and fluxes (times area_v / 3 and area_t of ``geometry``: socp._socp_to_dot); ``centred``: ``mu`` on
        the time-centred grid with ``geometry``'s mu0 / mu1 as end points (socp._to_time_centered).  ``info``: the sum of every
        layer of that ``mu`` and of its negative entries, device milliseconds and bytes copied."""
        w_vertex = w_triangle = mu0 = mu1 = None
        if dot_units:
            from . import _geometry_with_areas

            g = _geometry_with_areas(self.geometry)
            w_vertex = np.asarray(g["area_vertices"], dtype=np.float64) / 3.0
            w_triangle = np.asarray(g["area_triangles"], dtype=np.float64)
        if centred:
            mu0 = np.asarray(self.geometry["mu0"], dtype=np.float64)
            mu1 = np.asarray(self.geometry["mu1"], dtype=np.float64)
        mu, E, info = self._read_out(self.r * self.dual_scale, w_vertex, w_triangle, centred, mu0, mu1, sums=True)
        return {"mu": mu, "E": E}, info

    def flow_map(self, starts="vertices", floor=None, max_crossings=16, trajectory=False, push=None, span=None, action=False, slide=False):
        """The transport map of the current iterate, traced on the device (DeviceProblem.flow_map; flow.flow_map_host is the
        specification): where the mass at a point ends up, and with ``trajectory`` where it is after every interval.
        ``starts``: "vertices" (one particle on every vertex: flow.vertex_starts), "triangles" or ``("triangles", level)`` (one on
        every one of the ``level^2`` sub-triangles of every triangle: flow.triangle_starts) or ``(triangle (P,), weights (P, 3))`` in
        the numbering of ``geometry`` -- arbitrary points of the surface come from ``cascade.locate_device``, which returns exactly
        these two arrays.  ``floor``: densities up to it carry no velocity, in the units of the recovered ``mu`` (default
        ``1e-3 * max(mu0 / (area_vertices / 3))``); it is divided by the recovery factor before the call, since the device holds
        the iterate.  Returns the dict of ``flow_map_host`` plus ``positions`` (P, 3), and with ``trajectory`` ``positions_at``
        (T + 1, P, 3); ``ms`` and ``bytes``: device milliseconds of the launch and bytes copied to the host.
        ``push``: None, ``True`` or ``{"mass" (P,), "attributes" (A <= 4, P), "layers": "end" | "all"}``: what the particles carry is
        summed onto the vertices on the device (DeviceProblem.flow_push; flow.push_forward_host is the specification).  The
        default mass is that of ``mu0`` at the named starts (flow.start_masses), the default layer the last.  The result gains
        ``pushed``: ``{"mass" (L, V), "attributes" (A, L, V) or None, "dropped", "exponents" (flow.push_scales), "rested_mass" and
        "stopped_mass" (the mass of the particles that rested / stopped), "to_mu1":
        evaluate.compare_with_exact_transportation(mass[-1], mu1, geometry)}``.
        ``span = (node_from, node_to)`` and ``action``: the trace between two time nodes, backward where ``node_to < node_from`` (the
        inverse map: ``flow.pull_back`` then pulls a vertex field onto the starts), and the kinetic action of every particle
        (DeviceProblem.flow_trace; ``action`` alone means ``span=(0, n_time)``).  With neither, the call is the one above.  The result
        gains ``"span"``, ``"nodes"`` (n + 1,): the time node of every layer, and ``"action"`` (P,) on request; the trajectory has
        n + 1 layers.  The default mass of a push is that of ``mu0`` where ``node_from == 0`` and of ``mu1`` where
        ``node_from == n_time`` (a ``ValueError`` asks for ``mass`` otherwise); ``pushed["to_mu1"]`` is given only where
        ``node_to == n_time``, and ``pushed["to_mu0"]``, the same comparison against ``mu0``, where ``node_to == 0``.
        ``slide``: the sliding mode (DeviceProblem.flow_trace with ``slide=True``: dots_flow_slide; ``flow_map_host(..., slide=True,
        areas)`` is the specification): where two triangles push a particle at each other across their edge it moves along the edge
        instead of resting there.  Without a span the trace is ``(0, n_time)``.  The result gains ``"slides"`` and ``"steps"`` (P,),
        and ``pushed`` ``"slid_mass"``, the mass of the particles that slid at least once, beside the rested and the stopped mass.
        With ``slide=False`` the calls are the ones above."""
        from .. import evaluate, flow
        from . import _geometry_with_areas

        if self.dev.slab:
            raise ValueError("flow_map is not available on time slabs: the particles are traced on one GPU, which holds every time node")
        n_time = self.dev.T
        if not isinstance(slide, (bool, np.bool_)):
            raise ValueError("flow_map: slide must be True or False")
        span = _check_flow_span(span, action, n_time)
        if slide and span is None:
            span = (0, n_time)
        push = _check_flow_push(push, starts, span, n_time)
        vertices, triangles = np.asarray(self.geometry["vertices"], dtype=np.float64), np.asarray(self.geometry["triangles"])
        named = _check_flow_starts(starts)
        if named is None:
            start_triangle, start_weights = starts
        elif named[0] == "vertices":
            start_triangle, start_weights = flow.vertex_starts(triangles, vertices.shape[0])
        else:
            start_triangle, start_weights = flow.triangle_starts(triangles, named[1])
        g = _geometry_with_areas(self.geometry) if floor is None or push is not None else None
        if floor is None:
            floor = 1e-3 * float(np.max(np.asarray(g["mu0"], dtype=np.float64) / (np.asarray(g["area_vertices"], dtype=np.float64) / 3.0)))
        if getattr(self, "_neighbours", None) is None:
            self._neighbours = flow.triangle_neighbours(triangles)
        dev, floor = self.dev, float(floor) / (self.r * self.dual_scale)
        node_from, node_to = (0, n_time) if span is None else span
        mass = None
        if push is not None:      # (the default: mu0 from node 0, mu1 from node n_time; _check_flow_push refused an interior start)
            mass = push["mass"]
            if mass is None:
                mass = flow.start_masses(g["mu0" if node_from == 0 else "mu1"], g["area_vertices"], g["area_triangles"], triangles, start_triangle,
                                         start_weights, named[1])
            mass = np.asarray(mass, dtype=np.float64)
        common = dict(max_crossings=max_crossings, trajectory=trajectory)
        if span is not None:
            call, who = dev.flow_trace, "flow_trace"
            common.update(span=span, action=bool(action), slide=bool(slide))
        else:
            call, who = (dev.flow_map, "flow_map") if push is None else (dev.flow_push, "flow_push")
        if push is not None:
            common.update(mass=mass, attributes=push["attributes"], layers=push["layers"])
        out = call(start_triangle, start_weights, self._neighbours, floor, **common)
        out["ms"], out["bytes"] = getattr(dev, who + "_ms"), getattr(dev, who + "_bytes")
        if span is not None:
            step = 1 if node_to > node_from else -1
            out["span"], out["nodes"] = span, np.arange(node_from, node_to + step, step)
        if push is not None:
            pushed = {"mass": out.pop("mass_at"), "attributes": out.pop("attr_at"), "dropped": out.pop("dropped"), "exponents": out.pop("exponents"),
                      "rested_mass": float(np.sum(mass[out["rested"] > 0])), "stopped_mass": float(np.sum(mass[out["status"] == 1]))}
            if slide:
                pushed["slid_mass"] = float(np.sum(mass[out["slides"] > 0]))
            for end, key in ((n_time, "mu1"), (0, "mu0")):
                if node_to == end:
                    pushed["to_" + key] = evaluate.compare_with_exact_transportation(pushed["mass"][-1], np.asarray(g[key], dtype=np.float64), g)
            out["pushed"] = pushed
        out["positions"] = flow.positions(vertices, triangles, out["triangle"], out["weights"])
        if trajectory:
            out["positions_at"] = flow.positions(vertices, triangles, out["triangles_at"], out["weights_at"])
        return out

    def sensitivity(self, potentials=True, stress=True, to_device=False):
        """What the derivative of the transport cost of the current iterate is made of, reduced on the device
        (DeviceProblem.sensitivity: dots_sensitivity; sensitivity.potentials_host and stress_host on the recovered ``phi`` and ``mu``
        are the specification and return the same bits).  ``potentials``: ``phi0`` and ``phiT`` (V,), the recovered potential at the
        two ends as stored, and ``grad_mu0 = -(phi0 - mean)``, ``grad_mu1 = phiT - mean``, the derivative of the cost in the masses
        ``mu0`` / ``mu1`` of ``geometry``.  ``stress`` (F, 3, 6): the tensor the kinetic energy is linear in, with the vertex masses
        ``area_vertices / 3`` of ``geometry``; ``sensitivity.cost_gradients`` turns it into the derivative in the vertex positions.
        Refused with congestion > 0 (a ``ValueError``; the potentials are still to be had with ``stress=False``).  ``to_device``:
        torch tensors on the context's device instead of numpy arrays, nothing crosses to the host.  Also ``n_time``, and ``ms`` /
        ``bytes``: device milliseconds of the launches and bytes copied to the host."""
        from .. import sensitivity as sens
        from . import _geometry_with_areas

        spec = sens.check_sensitivity({"potentials": potentials, "stress": stress, "to_device": to_device}, getattr(self.dev, "slab", None),
                                      self.congestion0)
        mass = None
        if spec["stress"]:
            mass = np.asarray(_geometry_with_areas(self.geometry)["area_vertices"], dtype=np.float64) / 3.0
        dev = self.dev
        out = dev.sensitivity(self.prim_scale, self.r * self.dual_scale, mass, spec["potentials"], spec["stress"], spec["to_device"])
        if spec["potentials"]:
            out["grad_mu0"], out["grad_mu1"] = sens.potential_gradients(out["phi0"], out["phiT"])
        out["n_time"], out["ms"], out["bytes"] = dev.T, dev.sensitivity_ms, dev.sensitivity_bytes
        return out

    def finalize(self, download=True, outputs=None, read_out=None, flow_map=None, sensitivity=None):
        """``outputs``: None = the twelve arrays, or a tuple of names: only those are downloaded.  ``read_out``: None, or the
        keywords of ``read_out`` (dot_units, centred): the solution is then its ``{"mu", "E"}`` -- nothing else is downloaded --
        and ``run_history.solver_stats["readout"]`` its info.  ``flow_map``: None, or the keywords of ``flow_map`` as a dict:
        ``solution["flow_map"]`` then holds what it returns.  ``sensitivity``: None, True or the keywords of ``sensitivity`` as a
        dict: ``solution["sensitivity"]`` then holds what it returns."""
        if read_out is not None and outputs is not None:
            raise ValueError("finalize: outputs and read_out are mutually exclusive (read_out returns mu and E only)")
        flow_map = check_flow_map(flow_map, getattr(self.dev, "slab", None), self.dev.T)
        sensitivity = check_sensitivity(sensitivity, getattr(self.dev, "slab", None), self.congestion0)
        dev, hist, validator = self.dev, self.run_history, self.kkt_validator
        self._kkt_prefetch(range(7))
        validator.validator.validate(list(range(7)))
        org, _ = validator.collect()
        cost, lagr = self._objective()
        hist.record(current_it=self.counter_main, kkt_errors=org,
                    history={"Transportation cost": cost, "Objective value": lagr})
        self._collect_step_times(wait=True)
        hist.end()
        self.finalized = True
        hist.solver_stats = {
            "cg_iterations": int(self.cg_total), "cg_not_converged": int(self.cg_fail), "lap_solver": dev.lap_solver,
            "device_bytes": dev.device_bytes(), "final_r": self.r, "final_scale_z": self.scale_z,
        }
        if self.lap_solver_fallback:
            hist.solver_stats.update(lap_solver="modal_pcg (asked for modal_direct)", lap_solver_fallback=self.lap_solver_fallback)
        if self.cg_fail:
            logger.warning("PCG hit its iteration cap in %d solves", self.cg_fail)
        solution = {}
        if read_out is not None:
            solution, hist.solver_stats["readout"] = self.read_out(**read_out)
        elif download:
            names = STATE_NAMES if outputs is None else tuple(outputs)
            unknown = set(names) - set(STATE_NAMES)
            if unknown:
                raise ValueError(f"finalize: unknown outputs {sorted(unknown)}")
            solution = {name: self.recovered(name, self._download(name)) for name in names}
        if flow_map is not None:
            solution["flow_map"] = self.flow_map(**flow_map)
        if sensitivity is not None:
            solution["sensitivity"] = self.sensitivity(**sensitivity)
        solution["checkpoints"] = self.checkpoint_solutions if self.checkpoint_solutions else None
        logger.info("Number of iterations: %d   Iteration time: %.2f", self.counter_main, hist.running_time)
        return solution, hist

    def close(self):
        self.closed = True
        self.dev.close()

    def _warm_refusal(self):
        """Why this solver's iterate cannot be a warm start, or None."""
        if self.counter_main >= 0 and getattr(self, "_last_quiet", False) and not self.is_palm:
            return ("restart: the last iteration stored no z_mid (nothing was read back after it): a warm restart needs the "
                    "whole iterate; iterate to a read-back or restart cold")
        return None

    def _geometry_moved(self, moved):
        """``self.geometry`` after the context's vertices moved to ``moved`` (V, 3), a host array: positions and areas follow."""
        self.geometry = _moved_geometry(self.geometry, moved)

    def restart(self, mu0, mu1, warm=True, nit=None, tol=None, tol_checkpoints=None, time_limit=None, congestion=None, vertices=None, *,
                batch_member=False):
        """The next problem of a solve session on the live context: other end masses ``mu0`` / ``mu1`` (V,) on the same surface
        (DeviceProblem.restart: dots_restart).  The factor, the hierarchy and the plan are kept; the run starts as a new solver's does
        (r = 1, the initial z scaling, a fresh penalty schedule, validator and history).  ``warm=True``: from the recovered iterate
        the solver holds, rescaled in place on the device -- the state a new solver with ``init_solution=`` all twelve arrays of
        ``finalize()`` starts from, bit for bit, without the arrays crossing to the host; ``warm=False``: from zero, as a new solver.
        May be called mid-run, after the run has finished or after ``finalize``, not after ``close``; the caller's arrays and
        ``geometry`` dict are not written to (``self.geometry`` becomes a shallow copy with the new masses).  ``nit``, ``tol``,
        ``tol_checkpoints``, ``time_limit``, ``congestion``: None keeps the solver's.  Torch tensors on the context's device are read
        there (their finiteness is then the caller's business).  Returns the device milliseconds of the call.
        ``vertices`` (V, 3): the surface moves first (DeviceProblem.move_vertices: dots_move_vertices) -- same triangles, other
        positions; the geometry tables are assembled and the factor is computed again on the device, the tree and the plan stay --
        and the run then starts on the moved surface: what a new solver on ``geometry.plan_with_vertices(plan, vertices)`` computes,
        bit for bit.  ``self.geometry`` follows (vertices, areas); ``self.move_ms``: the three times of the move, or None.
        ``batch_member``: the route of ``BatchSession`` to a solver that is stepped by a batch (dots_restart takes a sharer of a
        factor: only this context's state changes); such a solver is moved by its session, with all holders of the factor
        (``device.move_vertices_many``), never through ``vertices``."""
        tol = self.tol if tol is None else tol
        checkpoints = _validate_checkpoints(tol_checkpoints, tol)
        if getattr(self, "closed", False):
            raise ValueError("restart: the solver is closed")
        if getattr(self.dev, "slab", None):
            raise ValueError("restart: not available on time slabs")
        if getattr(self, "_init_from", False):
            raise ValueError("restart: the solver was started from init_from (a level of a cascade); sessions over the cascades are not supported")
        if self.batched and not batch_member:
            raise ValueError("restart: the solver is stepped by a batch (solver_socp_many); sessions over batches are not supported")
        if batch_member and vertices is not None:
            raise ValueError("restart: a member of a batch moves with all holders of its factor (BatchSession.solve_many(vertices=))")
        V = int(np.asarray(self.geometry["vertices"]).shape[0])
        ordered = isinstance(mu0, DeviceOrdered) or isinstance(mu1, DeviceOrdered)      # (in the context's numbering: read as they lie)
        on_device = ordered or (_is_device_tensor(mu0) and _is_device_tensor(mu1))      # (one of each: both are read on the host)
        masses = _end_masses("restart", mu0, mu1, V, to_host=not on_device)
        if ordered and self.is_constant_scaling:
            raise ValueError("restart: is_constant_scaling reads the end masses on the host: not with masses in the context's numbering (DeviceOrdered)")
        if warm and self._warm_refusal():
            raise ValueError(self._warm_refusal())
        factors = self.recovery_factors() if warm else None
        if not batch_member:      # (a member's session has moved it, or not, and booked the times)
            self.move_ms = None
            if vertices is not None:
                given = vertices if _is_device_tensor(vertices) else _host_array(vertices)
                self.move_ms = self.dev.move_vertices(given, device_pointers=_is_device_tensor(given))
                self._geometry_moved(np.array(_host_array(given)))
        if ordered:      # (nothing crosses to the host: the solver holds no copy of these masses)
            ms = self.dev.restart(masses[0].tensor, masses[1].tensor, "warm" if warm else "cold", factors, device_pointers=True, device_order=True)
            self.geometry = _without_masses(self.geometry)
        else:
            ms = self.dev.restart(masses[0], masses[1], "warm" if warm else "cold", factors, device_pointers=on_device)
            if on_device:      # (the plan's host copies, back in the caller's numbering: read_out and flow_map take the end masses from the geometry)
                order = self._caller_order()
                masses = [self.dev.plan.mu0[order], self.dev.plan.mu1[order]]
            self.geometry = {**self.geometry, "mu0": np.array(masses[0]), "mu1": np.array(masses[1])}
        if nit is not None:
            self.nit = int(nit)
        if time_limit is not None:
            self.time_limit = time_limit
        self.tol, self.tol_checkpoints = tol, checkpoints
        self.checkpoint_solutions = []
        self.untimed_steps = self.quiet_steps = 0
        self._timed_in_flight = []      # (dots_restart emptied the library's ring)
        self._rhs_ahead = self._carry = self._fused_kkt = False
        self._pass, self._last_quiet = None, False
        self._start_run(self.congestion0 if congestion is None else congestion, keep_phi=bool(warm))
        self.restart_ms = ms
        return ms

    def _caller_order(self):
        """Index array that takes a per-vertex array of the plan (device numbering) to the caller's numbering."""
        perm = self.dev.plan.perm_vert
        inv = np.arange(self.dev.V)
        if perm is not None:
            inv = np.empty(self.dev.V, dtype=np.int64)
            inv[perm] = np.arange(self.dev.V)
        return inv


def solver_socp(
        n_time,
        geometry,
        congestion=0.0,
        nit=1000,
        eps=0.0,
        tol=1e-4,
        tau=1.90,
        is_palm=False,
        is_multi_threads=True,
        is_z_scaling=True,
        is_constant_scaling=False,
        check_kkt_step_by_step=False,
        init_solution=None,
        tol_checkpoints=None,
        time_limit=1000,
        *,
        lap_solver="modal_direct",
        cg_tol=DEFAULT_CG_TOL,
        cg_max_iter=20000,
        device=0,
        reorder=True,
        preconditioner="multigrid",
        mg_coarsest=256,
        nd_leaf=16,
        outputs=None,
        read_out=None,
        pcg_windows=False,
        flow_map=None,
        sensitivity=None,
):
    """SOCP for dynamical optimal transport on a discrete surface, on the GPU.

    Returns ``(solution, run_history)``: ``solution`` is a dict with the twelve arrays of
    ``SolutionSocpData`` (reference layouts, un-scaled as at solver_socp.py:397-405) plus
    ``checkpoints``; ``run_history`` is a :class:`RunningHistory`.
    ``is_multi_threads`` is accepted and ignored (the GPU path has no host threads to split).
    ``outputs``: a tuple of array names: ``solution`` holds only those (and ``checkpoints``), and only those are downloaded.
    ``read_out``: the keywords of ``AlmSolver.read_out`` (dot_units, centred): ``solution`` is ``mu`` and ``E`` as the solver
    plug-ins return them, formed on the device (``checkpoints`` stay in the solver's units).
    ``pcg_windows``: above 256 time nodes the modal PCG runs in windows of 256 modes: ``lap_solver="modal_pcg"`` takes
    ``n_time + 1 <= 1024`` with either preconditioner, and ``modal_direct`` falls back to it when its factor does not fit.
    ``flow_map``: the keywords of ``AlmSolver.flow_map`` as a dict (``{"starts": "vertices"}``): ``solution["flow_map"]`` is the
    transport map of the solution, traced on the device; None (the default) changes nothing.
    ``sensitivity``: True, or the keywords of ``AlmSolver.sensitivity`` as a dict: ``solution["sensitivity"]`` holds the potentials at
    the two ends and the stress of the kinetic energy, reduced on the device (``dots_socp_amd.sensitivity.cost_gradients`` makes the
    derivatives of the cost in mu0, mu1 and the vertex positions of them); None (the default) changes nothing.
    """
    flow_map, sensitivity = _requests("solver_socp", n_time, outputs, read_out, flow_map, sensitivity, [congestion])
    alm = AlmSolver(n_time, geometry, congestion=congestion, nit=nit, eps=eps, tol=tol, tau=tau, is_z_scaling=is_z_scaling,
                    is_constant_scaling=is_constant_scaling, check_kkt_step_by_step=check_kkt_step_by_step,
                    init_solution=init_solution, tol_checkpoints=tol_checkpoints, time_limit=time_limit, is_palm=is_palm,
                    lap_solver=lap_solver, cg_tol=cg_tol, cg_max_iter=cg_max_iter, device=device, reorder=reorder,
                    preconditioner=preconditioner, mg_coarsest=mg_coarsest, nd_leaf=nd_leaf, pcg_windows=pcg_windows)
    try:
        for _ in range(nit):
            if alm.iterate():
                break
        return alm.finalize(outputs=outputs, read_out=read_out, flow_map=flow_map, sensitivity=sensitivity)
    finally:
        alm.close()


# ---- a sequence of problems on one surface, one live context -----------------------------------------------------------------
SESSION_KEYS = ("congestion", "nit", "eps", "tol", "tau", "is_palm", "is_multi_threads", "is_z_scaling", "is_constant_scaling",
                "check_kkt_step_by_step", "tol_checkpoints", "time_limit", "lap_solver", "cg_tol", "cg_max_iter", "device", "reorder",
                "preconditioner", "mg_coarsest", "nd_leaf", "pcg_windows")
SESSION_SOLVE_KEYS = ("nit", "tol", "tol_checkpoints", "time_limit", "congestion")      # what one solve of a session may change


def _is_device_tensor(a):
    return type(a).__module__.startswith("torch") and bool(getattr(a, "is_cuda", False))


class DeviceOrdered:
    """An end mass that lies on the context's device in the CONTEXT's vertex numbering (``plan.perm_vert`` applied): ``tensor``, a
    float64 tensor of shape (V,), as ``DeviceProblem.barycenter_update`` writes ``nu_device_order``.  ``AlmSolver.restart`` and
    ``BatchSession.solve_many`` read such masses where they lie -- no permutation, no copy to the host --, so the solver then holds
    no host copy of its end masses: ``geometry`` has none, and what needs one (``read_out``, ``flow_map``, ``is_constant_scaling``) is
    not available for that solve.  Only a live context takes them (a restart), and both masses of a problem must be of this kind."""

    def __init__(self, tensor):
        self.tensor = tensor


def _host_array(a):
    """``a``, an array or a torch tensor wherever it lives, as a float64 array on the host"""
    return np.asarray(a.detach().cpu().numpy() if type(a).__module__.startswith("torch") else a, dtype=np.float64)


def _without_masses(geometry):
    return {k: v for k, v in geometry.items() if k not in ("mu0", "mu1")}


# ---- what the drivers over live contexts share: intake, admission, the slot loop ------------------------------------------------------
def _end_masses(who, mu0, mu1, V, to_host):
    """The end masses as a driver takes them: float64 host arrays of shape (V,) with finite entries; a tensor on a device passes as it
    is, checked for its shape alone (its entries are the caller's business), unless ``to_host``.  ``who`` opens the messages."""
    out = []
    if isinstance(mu0, DeviceOrdered) or isinstance(mu1, DeviceOrdered):
        if to_host or not (isinstance(mu0, DeviceOrdered) and isinstance(mu1, DeviceOrdered)):
            raise ValueError(f"{who}: masses in the context's numbering (DeviceOrdered) are for a restart of a live context, both of them")
        for name, a in (("mu0", mu0), ("mu1", mu1)):
            if not _is_device_tensor(a.tensor) or tuple(a.tensor.shape) != (V,):
                raise ValueError(f"{who}: {name} must hold a tensor of shape ({V},) on the context's device")
        return [mu0, mu1]
    for name, a in (("mu0", mu0), ("mu1", mu1)):
        if to_host or not _is_device_tensor(a):
            a = _host_array(a)
            if a.shape == (V,) and not np.all(np.isfinite(a)):
                raise ValueError(f"{who}: {name} has entries that are not finite")
        if tuple(a.shape) != (V,):
            raise ValueError(f"{who}: {name} must have shape ({V},), got {tuple(a.shape)}")
        out.append(a)
    return out


def _moved_vertices(who, vertices, V):
    """Moved vertices as a session takes them: ``(what the device call reads, the host array)`` -- a tensor on a device as it is,
    anything else as the host array; the host array is a finite (V, 3) float64 copy either way."""
    on_device = _is_device_tensor(vertices)
    host = _host_array(vertices)
    if host.shape != (V, 3):
        raise ValueError(f"{who}: vertices must have shape ({V}, 3), got {host.shape}")
    if not np.all(np.isfinite(host)):
        raise ValueError(f"{who}: vertices has entries that are not finite")
    return (vertices if on_device else host), np.array(host)


def _moved_geometry(geometry, host_vertices):
    """``geometry`` with its vertices at ``host_vertices`` (V, 3): the same triangles, positions and areas follow."""
    from .. import meshes

    t = np.asarray(geometry["triangles"])
    area_t = meshes.triangle_areas(host_vertices, t)
    return {**geometry, "vertices": host_vertices, "area_triangles": area_t,
            "area_vertices": meshes.vertex_areas(host_vertices.shape[0], t, area_t)}


def _requests(who, n_time, outputs, read_out, flow_map, sensitivity, congestions):
    """What every driver checks of the results it is asked for, before a device is touched; ``congestions``: of every problem.
    Returns the checked ``flow_map`` and ``sensitivity``."""
    if read_out is not None and outputs is not None:
        raise ValueError(f"{who}: outputs and read_out are mutually exclusive (read_out returns mu and E only)")
    flow_map = check_flow_map(flow_map, n_time=n_time)
    for congestion in congestions:
        sensitivity = check_sensitivity(sensitivity, congestion=congestion)
    return flow_map, sensitivity


class _Session:
    """What the two sessions share: the mesh, the counters, the context manager and the record ``solver_stats["session"]``."""

    def __init__(self, who, geometry):
        if not isinstance(geometry, dict) or "vertices" not in geometry or "triangles" not in geometry:
            raise ValueError(f"{who}: geometry must be a dict with 'vertices' and 'triangles'")
        self.geometry = _without_masses(geometry)
        self.n_vertices = int(np.asarray(geometry["vertices"]).shape[0])
        self.index = 0                  # problems admitted (SolveSession: solved) so far
        self.setup_seconds = None       # of the first context -- plan, factor, context --: what every later admission saves
        self.closed = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        self.closed = True
        for alm in self._live():
            alm.close()

    def _admitted(self, built, warm, restart_ms, setup, moved, move_ms):
        """``solver_stats["session"]`` of the problem just admitted; ``built``: its context was built for it (else restarted)."""
        if self.setup_seconds is None:
            self.setup_seconds = setup
        return {"index": self.index, "warm": bool(warm) and not built, "restart_ms": restart_ms, "setup_seconds": setup,
                "setup_seconds_saved": 0.0 if built else self.setup_seconds, "moved": bool(moved), "move_ms": move_ms}


class SolveSession(_Session):
    """One device context and one factor for a sequence of transport problems on one surface, whose end masses change from solve to
    solve: ``with SolveSession(n_time, geometry, **solver_options) as s: solution, hist = s.solve(mu0, mu1)``.

    ``geometry``: the mesh (``vertices``, ``triangles``; ``mu0`` / ``mu1`` in it are ignored); ``solver_options``: the keywords of
    ``solver_socp`` that shape the solver (``SESSION_KEYS``; no ``init_solution``: a session starts from zero or from its own last
    iterate).  The first ``solve`` builds the solver -- plan, factor, context --, every later one restarts it on the device
    (``AlmSolver.restart``: dots_restart): nothing is rebuilt, and nothing but what the caller asks for crosses to the host.
    ``close()`` (or leaving the ``with`` block) releases the context.  Moved vertices -- the same triangles at other positions -- are
    taken by ``solve(..., vertices=)``: the geometry tables and the factor are refreshed on the live context (dots_move_vertices), the
    tree and the plan stay.  Batches (``solver_socp_many``) have ``BatchSession``; not over the cascades, time slabs or changed
    connectivity."""

    def __init__(self, n_time, geometry, **solver_options):
        unknown = set(solver_options) - set(SESSION_KEYS)
        if unknown:
            raise ValueError(f"SolveSession: unknown option(s) {sorted(unknown)}; known: {list(SESSION_KEYS)}")
        _Session.__init__(self, "SolveSession", geometry)
        options = dict(solver_options)
        options.pop("is_multi_threads", None)
        check_time_nodes(n_time, options.get("lap_solver", "modal_direct"), None, options.get("pcg_windows", False))
        _validate_checkpoints(options.get("tol_checkpoints"), options.get("tol", 1e-4))
        if int(options.get("nit", 1000)) < 1:
            raise ValueError("SolveSession: nit must be at least 1")
        self.n_time, self.options = int(n_time), options
        self.alm = None

    def _live(self):
        return [] if self.alm is None else [self.alm]

    def solve(self, mu0, mu1, warm=True, outputs=None, read_out=None, flow_map=None, sensitivity=None, vertices=None, **per_solve):
        """Solve the problem with the end masses ``mu0`` / ``mu1`` (V,): returns ``(solution, run_history)`` as ``solver_socp(n_time,
        {**geometry, "mu0": mu0, "mu1": mu1}, **solver_options)`` does -- with ``warm=False`` bit for bit.  ``warm=True`` (the default)
        starts from the session's last iterate, rescaled on the device: what ``init_solution=`` the whole previous solution does over
        the host, bit for bit; on the first solve it is a cold start.  ``outputs``, ``read_out``, ``flow_map``, ``sensitivity``: as for
        ``solver_socp``.  ``per_solve``: ``nit``, ``tol``, ``tol_checkpoints``, ``time_limit``, ``congestion`` for this and the later
        solves.  The masses may be torch tensors on the context's device: from the second solve on they are read there.
        ``run_history.solver_stats["session"]`` = {"index", "warm", "restart_ms" (device milliseconds of the restart; None on the first
        solve), "setup_seconds" (wall time before the first iteration of this solve), "setup_seconds_saved" (the first solve's
        set-up: what this one did not repeat; 0 on the first), "moved", "move_ms"}.
        ``vertices`` (V, 3): the surface moves before this solve (same triangles): on the first solve they replace the session's, later
        the live context is moved (``AlmSolver.restart(vertices=)``: tables and factor are refreshed on the device, nothing is planned
        again); ``session.geometry`` follows.  ``"moved"``: whether this solve moved the surface; ``"move_ms"``: the device
        milliseconds of the assembly launches, the factor refresh and the whole move, or None."""
        if self.closed:
            raise ValueError("SolveSession.solve: the session is closed")
        unknown = set(per_solve) - set(SESSION_SOLVE_KEYS)
        if unknown:
            raise ValueError(f"SolveSession.solve: unknown option(s) {sorted(unknown)}; known: {list(SESSION_SOLVE_KEYS)}")
        who = "SolveSession.solve"
        first = self.alm is None
        congestion = per_solve.get("congestion", self.options.get("congestion", 0.0) if first else self.alm.congestion0)
        flow_map, sensitivity = _requests(who, self.n_time, outputs, read_out, flow_map, sensitivity, [congestion])
        m0, m1 = _end_masses(who, mu0, mu1, self.n_vertices, to_host=first)
        given, host = (None, None) if vertices is None else _moved_vertices(who, vertices, self.n_vertices)
        t0 = time.perf_counter()
        restart_ms = move_ms = None
        if first:
            self.options.update(per_solve)
            if host is not None:
                self.geometry = _moved_geometry(self.geometry, host)
            self.alm = AlmSolver(self.n_time, {**self.geometry, "mu0": m0.copy(), "mu1": m1.copy()}, **self.options)
        else:
            more = {} if given is None else {"vertices": given}      # (without vertices the call is the one a session always made)
            restart_ms = self.alm.restart(m0, m1, warm=bool(warm), **more, **per_solve)
            if given is not None:
                move_ms = self.alm.move_ms
                self.geometry = _without_masses(self.alm.geometry)
        record = self._admitted(first, warm, restart_ms, time.perf_counter() - t0, host is not None, move_ms)
        alm = self.alm
        for _ in range(alm.nit):
            if alm.iterate():
                break
        solution, hist = alm.finalize(outputs=outputs, read_out=read_out, flow_map=flow_map, sensitivity=sensitivity)
        hist.solver_stats["session"] = record
        self.index += 1
        return solution, hist



# ---- several problems on one surface, one factor ---------------------------------------------------------------------------
PER_PROBLEM_KEYS = ("mu0", "mu1", "congestion", "nit", "tol", "tau", "is_palm", "is_z_scaling", "is_constant_scaling", "check_kkt_step_by_step",
                    "init_solution", "tol_checkpoints", "time_limit")
COMMON_KEYS = ("eps", "lap_solver", "reorder", "nd_leaf", "device", "cg_tol", "cg_max_iter", "is_multi_threads")
BATCH_TIME_NOTE = ("phase times of a batched iteration are the batch's, booked to each active member as 1/n of them "
                   "(n = members in that iteration)")


def _batch_solver_options(common):
    """The keywords every solver of a batch is built with, from the options given once (``COMMON_KEYS``)."""
    reorder = common.get("reorder", True)
    return dict(eps=common.get("eps", 0.0), lap_solver="modal_direct", device=common.get("device", 0), reorder="nd" if reorder is True else reorder,
                cg_tol=common.get("cg_tol", DEFAULT_CG_TOL), cg_max_iter=common.get("cg_max_iter", 20000), nd_leaf=common.get("nd_leaf", 16))


def _needs_shared_factor(who, alm):
    """The first solver of a batch must hold the direct solver's factor: one that fell back to the PCG is closed and the memory error raised."""
    if alm.direct:
        return
    reason = alm.lap_solver_fallback
    alm.close()
    err = _lib.HipLibraryError(f"{who}: the shared factor does not fit (no batched PCG): {reason}")
    err.status = _lib.ERR_MEMORY
    raise err


def _batch_problems(geometry, problems, common):
    """The checks of solver_socp_many, before any device is touched."""
    if "pcg_windows" in common:
        raise ValueError(PCG_WINDOWS_ONE_SOLVER.format(who="solver_socp_many"))
    unknown = set(common) - set(COMMON_KEYS)
    if unknown:
        raise ValueError(f"solver_socp_many: unknown option(s) {sorted(unknown)}")
    if common.get("lap_solver", "modal_direct") != "modal_direct":
        raise ValueError("solver_socp_many: the batch shares the factor of the direct solver: lap_solver must be 'modal_direct'")
    if not problems:
        raise ValueError("solver_socp_many: no problems")
    verts, tris = np.asarray(geometry["vertices"]), np.asarray(geometry["triangles"])
    out = []
    for i, p in enumerate(problems):
        p = dict(p)
        for k in ("vertices", "triangles"):
            if k in p:
                if not np.array_equal(np.asarray(p.pop(k)), verts if k == "vertices" else tris):
                    raise ValueError(f"solver_socp_many: problem {i} is on another mesh: a batch shares one surface")
        for k in p:
            if k in COMMON_KEYS:
                raise ValueError(f"solver_socp_many: '{k}' shapes the factor or the solver: give it once for the batch, not per problem ({i})")
            if k not in PER_PROBLEM_KEYS:
                raise ValueError(f"solver_socp_many: unknown per-problem option '{k}' (problem {i})")
        for k in ("mu0", "mu1"):
            if p.get(k) is None:
                if k not in geometry:
                    raise ValueError(f"solver_socp_many: problem {i} has no {k}")
                p[k] = geometry[k]
            if np.asarray(p[k]).shape != (verts.shape[0],):
                raise ValueError(f"solver_socp_many: problem {i}: {k} must have one entry per vertex")
        _validate_checkpoints(p.get("tol_checkpoints"), p.get("tol", 1e-4))
        out.append(p)
    return out


def solver_socp_many(n_time, geometry, problems, *, max_batch=4, read_out=None, flow_map=None, sensitivity=None, outputs=None, plan=None, **common):
    """Solve several transport problems on ONE surface with one factor of the direct solver.

    ``geometry`` holds the mesh (``vertices``, ``triangles``; ``mu0`` / ``mu1`` are defaults for problems without their own);
    ``problems`` is a list of dicts with ``mu0``, ``mu1`` and any of the per-problem options of ``solver_socp`` (congestion, nit, tol,
    tau, is_palm, is_z_scaling, is_constant_scaling, check_kkt_step_by_step, init_solution, tol_checkpoints, time_limit).  The options that
    shape the factor or the solver (eps, lap_solver -- only "modal_direct" --, reorder, nd_leaf, device, cg_tol, cg_max_iter) are given
    once, as keywords.  At most ``max_batch`` problems are active at a time and advance in lockstep, one ALM iteration each with ONE batched
    pair of sweeps (dots_step_many); when one stops the next pending problem takes its slot, sharing the same factor (built once).

    Returns ``[(solution, run_history), ...]`` in input order, each what ``solver_socp(n_time, {**geometry, "mu0": ..., "mu1": ...},
    **common, **problem)`` returns, bit for bit; ``run_history.solver_stats["batch"]`` = {"size", "index", "max_batch", "steps_time_note"}.
    Each problem's running time and time limit start when it is admitted.  A factor that does not fit raises the library's memory error
    (there is no batched PCG).  ``read_out``, ``flow_map`` and ``sensitivity``: as for ``solver_socp``, for every problem (with its own
    mu0 / mu1 and congestion); so is ``outputs`` (the arrays that are downloaded; exclusive with ``read_out``).  ``plan``: the device
    plan of this mesh to number it by (``geometry.build_plan``, ``geometry.plan_with_vertices``) instead of building one: the nested
    dissection reads the positions, so a mesh that moved keeps the numbering of a live context only through its plan."""
    who = "solver_socp_many"
    probs = _batch_problems(geometry, problems, common)
    flow_map, sensitivity = _requests(who, n_time, outputs, read_out, flow_map, sensitivity, [p.get("congestion", 0.0) for p in probs])
    if int(max_batch) < 1:
        raise ValueError("solver_socp_many: max_batch >= 1")
    solver_kw = _batch_solver_options(common)
    if plan is not None and (plan.n_time != int(n_time) or plan.n_vertices != np.asarray(geometry["vertices"]).shape[0]
                             or plan.n_triangles != np.asarray(geometry["triangles"]).shape[0]):
        raise ValueError("solver_socp_many: plan is not a plan of this mesh and n_time")
    mesh = _without_masses(geometry)
    base = plan if plan is not None else _base_plan(n_time, mesh, probs[0], solver_kw)

    def admit(slot, i, owner):
        p = probs[i]
        return _new_member(who, n_time, mesh, base, p["mu0"], p["mu1"], owner, solver_kw, **_without_masses(p))

    # a slot per problem, at most max_batch of them running: the members step in the order they were admitted in
    return _run_slots(len(probs), int(max_batch), lambda i, running: i if len(running) < int(max_batch) else None, admit,
                      dict(outputs=outputs, read_out=read_out, flow_map=flow_map, sensitivity=sensitivity))


def _base_plan(n_time, mesh, p, solver_kw):
    """The plan every solver of a batch on ``mesh`` is built on, up to its densities (here those of problem ``p``)"""
    from .. import geometry as geo

    return geo.build_plan(n_time, {**mesh, "mu0": p["mu0"], "mu1": p["mu1"]}, reorder=solver_kw["reorder"], nd_leaf=solver_kw["nd_leaf"])


def _new_member(who, n_time, mesh, base, mu0, mu1, owner, solver_kw, **run):
    """A new solver of a batch on ``mesh`` with the end masses ``mu0`` / ``mu1``: ``base`` with these densities, and the factor of
    ``owner``, a solver that holds it -- None: this one builds it, and must not fall back to the PCG."""
    from .. import geometry as geo

    alm = AlmSolver(n_time, {**mesh, "mu0": mu0, "mu1": mu1}, plan=geo.plan_with_densities(base, mu0, mu1),
                    front_owner=None if owner is None else owner.dev, **solver_kw, **run)
    if owner is None:
        _needs_shared_factor(who, alm)
    return alm


def _run_slots(n_problems, max_batch, slot_for, admit, requests, harvested=None, keep=False, live=()):
    """The loop of the batch drivers: while problems are pending or running, admit into free slots, step every running solver once
    (``_lockstep``: in slot order, in groups of ``max_batch``), finalize those that finished and write their ``solver_stats["batch"]``.
    Returns ``[(solution, run_history), ...]`` in input order.
    ``slot_for(i, running)``: the slot the first pending problem ``i`` may take now (``running``: the slots in use), or None: it waits.
    ``admit(slot, i, owner)``: returns the solver, new or restarted, that now runs problem ``i``; ``owner``: a live holder of the factor
    -- the first that runs as the round begins, else that the last round harvested, else of ``live`` (the caller's idle solvers) --,
    or None: the first admitted builds the factor and is the owner from then on.  ``requests``: the keywords of ``finalize``;
    ``harvested(slot, i, run_history)``: the caller's hook after it.  ``keep``: the solvers stay the caller's; else a harvested one is
    closed after the next admissions, so that a holder of the factor store is alive throughout, and all of them however the loop ends."""
    results = [None] * n_problems
    pending = list(range(n_problems))
    running, retired = {}, []      # slot -> (problem, solver); the harvested solvers that are still to be closed
    try:
        while pending or running:
            owner = next(iter([running[slot][1] for slot in sorted(running)] + retired + list(live)), None)      # (one for the whole round)
            while pending:
                slot = slot_for(pending[0], running)
                if slot is None:
                    break
                i = pending.pop(0)
                running[slot] = (i, admit(slot, i, owner))
                owner = owner or running[slot][1]
            for alm in retired:
                alm.close()
            retired = []
            _lockstep([running[slot][1] for slot in sorted(running)], max_batch)
            for slot in sorted(running):
                i, alm = running[slot]
                if alm.finished:
                    sol, hist = alm.finalize(**requests)
                    hist.solver_stats["batch"] = {"size": n_problems, "index": i, "max_batch": max_batch, "steps_time_note": BATCH_TIME_NOTE}
                    if harvested is not None:
                        harvested(slot, i, hist)
                    results[i] = (sol, hist)
                    del running[slot]
                    if not keep:
                        retired.append(alm)
    finally:
        if not keep:
            for alm in [alm for _, alm in running.values()] + retired:
                alm.close()
    return results



def _lockstep(solvers, max_batch):
    """One ALM iteration of every solver of ``solvers`` (holders of one factor) that still runs: those that step, in groups of at most
    ``max_batch`` in the order given, each group with ONE batched pair of sweeps (device.step_many)."""
    from ..device import step_many

    members = []
    for alm in solvers:
        quiet = alm.iterate_begin()
        if quiet is not None:
            members.append((alm, quiet))
    for at in range(0, len(members), max_batch):
        group = members[at:at + max_batch]
        booked = [(alm, alm.batch_step_prepare(quiet)) for alm, quiet in group]
        sampled = any(s for _, (_, s) in booked)
        st = step_many([alm.dev for alm, _ in group], stats=sampled)
        n = len(group)
        for alm, (kind, sample) in booked:
            if sample and st is not None:
                alm._account(_BatchShare(st, n), kind)
            else:
                alm.untimed_steps += 1
        for alm, _ in group:
            alm.iterate_end()


class _BatchShare:
    """1/n of a batch's phase times, in the form AlmSolver._account reads"""

    def __init__(self, st, n):
        self.cg_iterations = self.cg_not_converged = 0
        self.alm_iterations = 1
        self.ms_rhs = st.ms_rhs / n
        self.ms_laplacian = st.ms_laplacian / n
        self.ms_soc = st.ms_soc / n
        self.ms_q_lambda_multiplier = st.ms_q_lambda_multiplier / n


# ---- a sequence of batches on one surface: live contexts on one shared factor ------------------------------------------------------
BATCH_SESSION_FIXED = ("tau", "is_palm", "is_z_scaling", "is_constant_scaling", "check_kkt_step_by_step")      # per problem in solver_socp_many; a restart cannot change them
BATCH_SOLVE_DEFAULTS = {"nit": 1000, "tol": 1e-4, "tol_checkpoints": None, "time_limit": 1000, "congestion": 0.0}      # SESSION_SOLVE_KEYS as a new AlmSolver has them


class BatchSession(_Session):
    """Live device contexts on ONE shared factor for a sequence of batches of transport problems on one surface, whose end masses --
    and vertex positions -- change from call to call: ``with BatchSession(n_time, geometry, max_batch=4) as bs: results =
    bs.solve_many(problems)``.  What ``solver_socp_many`` is to ``solver_socp``, this is to ``SolveSession``.

    ``geometry``: the mesh (``vertices``, ``triangles``; ``mu0`` / ``mu1`` in it are defaults for problems without their own).
    ``options``: the keywords ``solver_socp_many`` takes once (``COMMON_KEYS``) and the solver options a restart cannot change
    (``BATCH_SESSION_FIXED``: tau, is_palm, is_z_scaling, is_constant_scaling, check_kkt_step_by_step), fixed for the session.
    ``slots`` (default ``max_batch``, at least ``max_batch``): the live contexts the session keeps, created when first needed; each
    holds the state of the problem it solved last.  At most ``max_batch`` of them share one ``device.step_many`` call; with more slots
    the running members are stepped in groups of ``max_batch``, in slot order.  Memory: ``slots`` times the state of one context
    plus ONE factor.  ``close()`` (or leaving the ``with`` block) releases every context; the factor goes with the last."""

    def __init__(self, n_time, geometry, max_batch=4, slots=None, **options):
        if "pcg_windows" in options:
            raise ValueError(PCG_WINDOWS_ONE_SOLVER.format(who="BatchSession"))
        unknown = set(options) - set(COMMON_KEYS) - set(BATCH_SESSION_FIXED)
        if unknown:
            raise ValueError(f"BatchSession: unknown option(s) {sorted(unknown)}; known: {list(COMMON_KEYS + BATCH_SESSION_FIXED)}")
        if options.get("lap_solver", "modal_direct") != "modal_direct":
            raise ValueError("BatchSession: the batch shares the factor of the direct solver: lap_solver must be 'modal_direct'")
        _Session.__init__(self, "BatchSession", geometry)
        if int(max_batch) < 1:
            raise ValueError("BatchSession: max_batch >= 1")
        slots = int(max_batch) if slots is None else int(slots)
        if slots < int(max_batch):
            raise ValueError(f"BatchSession: slots = {slots} < max_batch = {int(max_batch)}: a lockstep group needs a context per member")
        check_time_nodes(n_time, "modal_direct")
        self.n_time, self.max_batch = int(n_time), int(max_batch)
        self.solver_kw = {**_batch_solver_options(options), **{k: options[k] for k in BATCH_SESSION_FIXED if k in options}}
        self.default_masses = {k: geometry[k] for k in ("mu0", "mu1") if k in geometry}
        self.solvers = [None] * slots   # AlmSolver per slot, or None: not created yet
        self.solved = [False] * slots   # the slot's context holds the iterate of a finished solve
        self.base = None                # the plan every context is built on, up to the densities; follows the moves

    def _live(self):
        return [alm for alm in self.solvers if alm is not None]

    def _problems(self, problems):
        """The checks of ``solve_many`` on its problems, before any device is touched: dicts with host masses and every key of
        ``SESSION_SOLVE_KEYS`` (a problem describes its run completely: what it leaves out is a new solver's default)."""
        if not problems:
            raise ValueError("BatchSession.solve_many: no problems")
        out = []
        for i, p in enumerate(problems):
            p = dict(p)
            for k in p:
                if k in BATCH_SESSION_FIXED or k in COMMON_KEYS:
                    raise ValueError(f"BatchSession.solve_many: '{k}' is fixed for the session: give it to BatchSession, not per problem ({i})")
                if k == "init_solution":
                    raise ValueError(f"BatchSession.solve_many: problem {i}: no init_solution: a slot starts from zero or, with warm=True, from its own last iterate")
                if k not in ("mu0", "mu1") + SESSION_SOLVE_KEYS:
                    raise ValueError(f"BatchSession.solve_many: unknown per-problem option '{k}' (problem {i}); known: {list(('mu0', 'mu1') + SESSION_SOLVE_KEYS)}")
            for k in ("mu0", "mu1"):
                if p.get(k) is None:
                    if k not in self.default_masses:
                        raise ValueError(f"BatchSession.solve_many: problem {i} has no {k}")
                    p[k] = self.default_masses[k]
            ordered = isinstance(p["mu0"], DeviceOrdered) or isinstance(p["mu1"], DeviceOrdered)      # (read where they lie, by a restart)
            p["mu0"], p["mu1"] = _end_masses(f"BatchSession.solve_many: problem {i}", p["mu0"], p["mu1"], self.n_vertices, to_host=not ordered)
            p = {**BATCH_SOLVE_DEFAULTS, **p}
            _validate_checkpoints(p["tol_checkpoints"], p["tol"])
            if int(p["nit"]) < 1:
                raise ValueError(f"BatchSession.solve_many: problem {i}: nit must be at least 1")
            out.append(p)
        return out

    def _move(self, given, host):
        """All live contexts to other positions with ONE refresh of the factor (device.move_vertices_many); the session's geometry and
        plan, and every solver's geometry, follow.  Without a live context the positions replace the session's.  Returns the times."""
        from ..device import move_vertices_many

        live = self._live()
        if not live:
            self.geometry = _moved_geometry(self.geometry, host)
            return None
        ms = move_vertices_many([alm.dev for alm in live], given, device_pointers=_is_device_tensor(given))
        for alm in live:
            alm._geometry_moved(host)
            alm.move_ms = ms
        self.base = live[0].dev.plan
        self.geometry = _without_masses(live[0].geometry)
        return ms

    def _admit(self, slot, p, warm, owner, moved, move_ms):
        """Problem ``p`` into ``slot``: a new solver on the session's plan where the slot has no context yet, else a restart of the
        one it has.  Returns the solver and its ``solver_stats["session"]`` (``moved``, ``move_ms``: this call's move, for the record)."""
        t0 = time.perf_counter()
        run = {k: p[k] for k in SESSION_SOLVE_KEYS}
        alm, restart_ms = self.solvers[slot], None
        built = alm is None
        if built and isinstance(p["mu0"], DeviceOrdered):
            raise ValueError("BatchSession.solve_many: masses in the context's numbering (DeviceOrdered) need a slot that holds a context: solve with host masses first")
        if built:
            if self.base is None:
                self.base = _base_plan(self.n_time, self.geometry, p, self.solver_kw)
            alm = _new_member("BatchSession", self.n_time, self.geometry, self.base, p["mu0"].copy(), p["mu1"].copy(), owner, self.solver_kw, **run)
            self.solvers[slot] = alm
        else:
            restart_ms = alm.restart(p["mu0"], p["mu1"], warm=warm, batch_member=True, **run)
        self.solved[slot] = False
        record = self._admitted(built, warm, restart_ms, time.perf_counter() - t0, moved, move_ms)
        self.index += 1
        return alm, record

    def solve_many(self, problems, warm=False, vertices=None, outputs=None, read_out=None, flow_map=None, sensitivity=None):
        """Solve ``problems`` -- dicts with ``mu0``, ``mu1`` (V,) and any of ``nit``, ``tol``, ``tol_checkpoints``, ``time_limit``,
        ``congestion`` (what a problem leaves out is a new solver's default, not the slot's last value) -- on the session's contexts.
        Returns ``[(solution, run_history), ...]`` in input order.
        ``warm=False``: the problems are admitted into free slots in input order and a slot that finishes takes the next one, as
        ``solver_socp_many`` does, and with its results bit for bit; a slot that holds a context takes its problem by a cold restart
        on the device (``AlmSolver.restart``: dots_restart), so from the second call on nothing is built.
        ``warm=True``: problem ``i`` runs in slot ``i`` from that slot's last iterate -- per problem what
        ``SolveSession.solve(..., warm=True)`` computes, bit for bit, under ``AlmSolver.restart``'s rules; at most ``slots`` problems, each
        on a slot that has solved before.
        ``vertices`` (V, 3; an array or a tensor on the contexts' device): the surface moves before the solves, same triangles: every
        live context takes the positions and the shared factor is refreshed once (``device.move_vertices_many``); contexts created
        later are built on the moved plan; ``self.geometry`` follows.  On the first call they replace the session's positions.
        A problem whose ``mu0`` and ``mu1`` are both ``DeviceOrdered`` (tensors on the device in the contexts' vertex numbering) is
        taken by its slot's restart where the masses lie, with no copy to the host; its slot must hold a context already.
        ``outputs``, ``read_out``, ``flow_map``, ``sensitivity``: as for ``solver_socp_many``.
        ``run_history.solver_stats["batch"]`` as ``solver_socp_many`` writes it; ``solver_stats["session"]`` = {"index" (problems the
        session admitted before this one), "warm", "restart_ms" (None where the context was built for this problem), "setup_seconds",
        "setup_seconds_saved" (the first context's set-up, 0 where one was built), "moved", "move_ms" (of this call's one move, the
        same in every problem's record)}."""
        if self.closed:
            raise ValueError("BatchSession.solve_many: the session is closed")
        who = "BatchSession.solve_many"
        probs = self._problems(problems)
        flow_map, sensitivity = _requests(who, self.n_time, outputs, read_out, flow_map, sensitivity, [p["congestion"] for p in probs])
        slots = len(self.solvers)
        if warm:
            if len(probs) > slots:
                raise ValueError(f"BatchSession.solve_many: warm=True runs problem i in slot i: {len(probs)} problems, {slots} slots (problem {slots} has none)")
            for i in range(len(probs)):
                if not self.solved[i]:
                    raise ValueError(f"BatchSession.solve_many: warm=True: slot {i} has not solved a problem yet: problem {i} has no iterate to start from")
                refusal = self.solvers[i]._warm_refusal()
                if refusal:
                    raise ValueError(f"BatchSession.solve_many: problem {i}: {refusal}")
        given, host = (None, None) if vertices is None else _moved_vertices(who, vertices, self.n_vertices)
        for alm in self._live():
            alm.move_ms = None
        move_ms = None if host is None else self._move(given, host)
        records = {}        # problem -> its session record

        def slot_for(i, running):      # (warm: problem i runs in slot i; else the first free slot takes the first pending problem)
            return next((slot for slot in ([i] if warm else range(slots)) if slot not in running), None)

        def admit(slot, i, owner):
            alm, records[i] = self._admit(slot, probs[i], bool(warm), owner, host is not None, move_ms)
            return alm

        def harvested(slot, i, hist):
            hist.solver_stats["session"] = records[i]
            self.solved[slot] = True

        return _run_slots(len(probs), self.max_batch, slot_for, admit, dict(outputs=outputs, read_out=read_out, flow_map=flow_map, sensitivity=sensitivity),
                          harvested, keep=True, live=self._live())


# ---- coarse-to-fine cascades: what the drivers share ---------------------------------------------------------------------------------
CASCADE_KEYS = ("congestion", "nit", "eps", "tol", "tau", "is_palm", "is_multi_threads", "is_z_scaling", "is_constant_scaling",
                "check_kkt_step_by_step", "init_solution", "tol_checkpoints", "time_limit", "lap_solver", "cg_tol", "cg_max_iter", "device",
                "reorder", "preconditioner", "mg_coarsest", "nd_leaf")


def _check_option_names(who, kwargs):
    if "pcg_windows" in kwargs:
        raise ValueError(PCG_WINDOWS_ONE_SOLVER.format(who=who))
    unknown = set(kwargs) - set(CASCADE_KEYS)
    if unknown:
        raise ValueError(f"{who}: unknown option(s) {sorted(unknown)}")


def _check_lap_solver(kwargs, time_grids):
    """The solver's name, then every time grid against it.  ``time_grids``: a list, or a callable that makes it once the name is good."""
    lap_solver = kwargs.get("lap_solver", "modal_direct")
    if lap_solver != "modal_direct" and lap_solver not in _lib.LAP_SOLVERS:
        raise ValueError(f"lap_solver must be one of {['modal_direct'] + list(_lib.LAP_SOLVERS)}")
    time_grids = time_grids() if callable(time_grids) else time_grids
    for T in time_grids:
        check_time_nodes(T, lap_solver)
    return time_grids


def _check_preconditioner(kwargs):
    if kwargs.get("preconditioner", "multigrid") not in ("multigrid", "jacobi"):
        raise ValueError("preconditioner must be 'multigrid' or 'jacobi'")


def _common_cascade_checks(kwargs, level_tol, time_grids=None, level_tol_optional=False):
    """The option checks the cascade drivers repeat, in the order their callers see: with ``time_grids`` the Laplacian solver and the
    preconditioner are checked here too (the cascade in space leaves them to AlmSolver).  ``level_tol``: None is ``tol``, or with
    ``level_tol_optional`` left to the driver that will run.  Returns ``(level_tol, time_grids)``."""
    if time_grids is not None:
        time_grids = _check_lap_solver(kwargs, time_grids)
    tol = kwargs.get("tol", 1e-4)
    if level_tol is None and not level_tol_optional:
        level_tol = tol
    if (level_tol is not None or not level_tol_optional) and not (isinstance(level_tol, (int, float)) and level_tol > 0):
        raise ValueError("level_tol must be a positive number")
    _validate_checkpoints(kwargs.get("tol_checkpoints"), tol)
    if time_grids is not None:
        _check_preconditioner(kwargs)
    if int(kwargs.get("nit", 1000)) < 1:
        raise ValueError("nit must be at least 1")
    return level_tol, time_grids


def _max_distance(geom):
    d = (geom.get("transfer") or {}).get("max_distance")
    return None if d is None else float(d)


def _time_record(alm, hist, setup, n_time):
    return {"n_time": int(n_time), "tol": float(alm.tol), "iterations": int(alm.counter_main) + 1, "running_time": float(hist.running_time),
            "setup_seconds": float(setup), "prolong_ms": alm.prolong_ms, "cost": float(hist.history["Transportation cost"][-1]),
            "kkt_max": float(np.nanmax(np.asarray(hist.kkt_errors[-1], dtype=np.float64)))}


def _mesh_record(alm, hist, setup, geom, first):
    return {"n_vertices": int(alm.dev.V), "n_triangles": int(alm.dev.F), "tol": float(alm.tol), "iterations": int(alm.counter_main) + 1,
            "running_time": float(hist.running_time), "setup_seconds": float(setup), "prolong_ms": alm.prolong_ms,
            "prolong_bytes": getattr(alm.dev, "prolong_bytes", None), "cost": float(hist.history["Transportation cost"][-1]),
            "kkt_max": float(np.nanmax(np.asarray(hist.kkt_errors[-1], dtype=np.float64))),
            "device_bytes": int(hist.solver_stats["device_bytes"]),
            "transfer": None if first else ("nested" if geom.get("parents") is not None else "located"),
            "max_distance": None if first else _max_distance(geom)}


def _carried(geom, i, **more):
    """The AlmSolver keywords of mesh level ``i``: how the state of the level below reaches it."""
    return dict(geometry=geom, init_parents=geom.get("parents") if i else None, init_transfer=geom.get("transfer") if i else None, **more)


def _run_levels(levels, stats_key, record, level_tol, opts, read_out, flow_map, sensitivity=None):
    """The level loop of the cascade drivers.  ``levels``: per level, the AlmSolver keywords that vary (``n_time``, ``geometry``, a ``plan``,
    ``init_parents`` / ``init_transfer`` / ``init_regrid``, ...), or a callable that makes them when the level starts (its time is set-up
    time).  Each level is warm-started from the one before (``init_from``, released before the finer factor is built), runs ``nit``
    iterations at most within what is left of ``time_limit``, and adds ``record(alm, hist, setup, i)`` to ``solver_stats[stats_key]``;
    only the last one is downloaded, read out, traced (``flow_map``) and asked for its ``sensitivity``.  ``opts``: the driver's checked
    options."""
    tol, nit = opts.pop("tol", 1e-4), int(opts.pop("nit", 1000))
    time_limit = opts.pop("time_limit", 1000)
    init_solution, checkpoints = opts.pop("init_solution", None), opts.pop("tol_checkpoints", None)
    t_start = time.perf_counter()
    records = []
    coarse = alm = None
    try:
        for i, level in enumerate(levels):
            last = i + 1 == len(levels)
            t0 = time.perf_counter()
            level = level() if callable(level) else level
            alm = AlmSolver(nit=nit, tol=tol if last else level_tol, tol_checkpoints=checkpoints if last else None,
                            init_solution=init_solution if i == 0 else None, init_from=coarse, release_init_from=True,
                            time_limit=max(time_limit - (t0 - t_start), 0.0), **level, **opts)
            coarse = None      # (closed by the constructor as soon as the finer state was filled)
            setup = time.perf_counter() - t0
            for _ in range(nit):
                if alm.iterate():
                    break
            solution, hist = alm.finalize(download=last, read_out=read_out if last else None, flow_map=flow_map if last else None,
                                          sensitivity=sensitivity if last else None)
            records.append(record(alm, hist, setup, i))
            coarse, alm = alm, None
        coarse.dev.sync()
        hist.solver_stats[stats_key] = {"levels": records, "total_seconds": time.perf_counter() - t_start}
        return solution, hist
    finally:
        for a in (alm, coarse):
            if a is not None:
                a.close()


# ---- coarse-to-fine time cascade ---------------------------------------------------------------------------------------------
def _cascade_options(n_time, levels, level_tol, kwargs):
    """The checks of solver_socp_cascade, before any device is touched: (levels, level_tol, options)."""
    from .. import cascade

    if "time_slab" in kwargs:
        raise ValueError("solver_socp_cascade: time slabs are not supported (a cascade runs on one GPU)")
    if "init_from" in kwargs:
        raise ValueError("solver_socp_cascade: init_from belongs to the levels of the cascade; start the coarsest level with init_solution")
    _check_option_names("solver_socp_cascade", kwargs)
    level_tol, levels = _common_cascade_checks(kwargs, level_tol, cascade.check_levels(levels, n_time))
    opts = dict(kwargs)
    opts.pop("is_multi_threads", None)
    return levels, level_tol, opts


def solver_socp_cascade(n_time, geometry, levels=None, level_tol=None, read_out=None, flow_map=None, sensitivity=None, **kwargs):
    """``solver_socp`` through a coarse-to-fine cascade in time: the problem is solved on the time grids ``levels`` (``n_time`` values,
    increasing, the last one ``n_time``) one after the other, each level warm-started from the recovered solution of the one before,
    interpolated linearly in time on the device (AlmSolver ``init_from``; cascade.prolong_time is the specification).  The number of
    iterations hardly depends on the time grid and an iteration on half the grid moves half the bytes, so most of the way to the
    solution is covered where iterations are cheap.

    ``levels=None``: ``n_time + 1`` halved while it is even and stays >= 16 nodes (1023 -> 15, 31, ..., 1023; 31 -> 15, 31; 20 -> 20
    alone).  ``level_tol``: the tolerance of the levels below the finest (default ``tol``).  The other keywords are ``solver_socp``'s:
    ``nit`` holds per level, ``time_limit`` for the whole cascade (a level gets the time that is left), ``init_solution`` starts the
    coarsest level, ``tol_checkpoints`` belong to the finest level.  Every level starts as a warm start through ``init_solution`` does
    (r = 1, the initial z scaling, a fresh penalty schedule, validator and history).

    Returns ``(solution, run_history)`` of the finest level; ``run_history.running_time`` is that level's own, and
    ``run_history.solver_stats["cascade"]`` = {"levels": [one record per level: n_time, tol, iterations, running_time, setup_seconds,
    prolong_ms (device events; None on the coarsest level), cost, kkt_max], "total_seconds"} has the whole cascade.
    ``read_out``, ``flow_map`` and ``sensitivity``: as for ``solver_socp``, for the finest level.  The mesh is the same on every level;
    ``solver_socp_spacetime_cascade`` coarsens the mesh along with the time grid."""
    from .. import geometry as geo

    flow_map = check_flow_map(flow_map, kwargs.get("time_slab"), n_time)
    sensitivity = check_sensitivity(sensitivity, kwargs.get("time_slab"), kwargs.get("congestion", 0.0))
    levels, level_tol, opts = _cascade_options(n_time, levels, level_tol, kwargs)
    reorder = opts.pop("reorder", True)
    if opts.get("lap_solver", "modal_direct") == "modal_direct" and reorder is True:
        reorder = "nd"      # (as AlmSolver chooses it)
    nd_leaf = opts.get("nd_leaf", 16)
    shared, plans = {}, []

    def level(T):      # the levels' plans share what does not depend on the time grid
        plans.append(geo.build_plan(T, geometry, reorder=reorder, nd_leaf=nd_leaf, _shared=shared, _earlier=tuple(plans)))
        return dict(n_time=T, geometry=geometry, plan=plans[-1], batched=False, reorder=reorder)

    return _run_levels([lambda T=T: level(T) for T in levels], "cascade", lambda alm, hist, setup, i: _time_record(alm, hist, setup, levels[i]),
                       level_tol, opts, read_out, flow_map, sensitivity)


# ---- coarse-to-fine cascade in space ---------------------------------------------------------------------------------------------
def _mesh_cascade_options(geometries, level_tol, kwargs, who="solver_socp_mesh_cascade"):
    """The checks of solver_socp_mesh_cascade (and, as ``who``, of the cascade in space and time), before any device is touched:
    (geometries, level_tol, options)."""
    from .. import cascade

    try:
        geometries = list(geometries)
    except TypeError:
        raise ValueError(f"{who}: geometries must be a list of geometries, coarse to fine") from None
    if len(geometries) < 2:
        raise ValueError(f"{who}: at least two geometries (a coarse level and its refinement); one level is solver_socp")
    for key in ("time_slab", "init_from", "init_parents", "init_transfer", "levels"):
        if key in kwargs:
            raise ValueError(f"{who}: {key} is not an option of the cascade in space" +
                             (" (a cascade in time and in space in one call is not supported)" if key == "levels" else ""))
    _check_option_names(who, kwargs)
    for i, (coarse, fine) in enumerate(zip(geometries, geometries[1:])):
        nested, located = isinstance(fine, dict) and fine.get("parents") is not None, isinstance(fine, dict) and fine.get("transfer") is not None
        if nested and located:
            raise ValueError(f"{who}: geometry {i + 1} has both 'parents' and 'transfer': the level below is its parent mesh "
                             "or a located mesh, not both")
        if not nested and not located:
            raise ValueError(f"{who}: geometry {i + 1} has neither 'parents' (meshes.refine_levels / meshes.subdivide) nor "
                             "'transfer' (meshes.link_levels / cascade.mesh_transfer)")
        size_c = dict(n_vertices=np.asarray(coarse["vertices"]).shape[0], n_triangles=np.asarray(coarse["triangles"]).shape[0])
        size_f = (np.asarray(fine["vertices"]).shape[0], np.asarray(fine["triangles"]).shape[0])
        if nested:
            vp, tp = cascade.check_parents(fine["parents"], **size_c)
            if (vp.shape[0], tp.shape[0]) != size_f:
                raise ValueError(f"{who}: the parents of geometry {i + 1} do not have its size")
        else:
            vs, _, ts, _ = cascade.check_transfer(fine["transfer"], **size_c)
            if (vs.shape[0], ts.shape[0]) != size_f:
                raise ValueError(f"{who}: the transfer of geometry {i + 1} does not have its size")
    level_tol, _ = _common_cascade_checks(kwargs, level_tol)
    opts = dict(kwargs)
    opts.pop("is_multi_threads", None)
    return geometries, level_tol, opts


def solver_socp_mesh_cascade(n_time, geometries, level_tol=None, read_out=None, flow_map=None, sensitivity=None, **kwargs):
    """``solver_socp`` through a coarse-to-fine cascade in space: the problem is solved on the meshes ``geometries`` (coarse to fine,
    every one after the first the nested refinement of the one before with its ``parents``: ``meshes.refine_levels``), all at
    ``n_time``, each level warm-started from the recovered solution of the one before, carried to the refinement on the device
    (AlmSolver ``init_from`` with ``init_parents``; cascade.prolong_space is the specification).  A level down has a quarter of the
    vertices and triangles: state, factor, set-up and every launch shrink with them.  A level may instead carry ``transfer``
    (``meshes.link_levels`` / ``cascade.mesh_transfer``): the level below is then an independent triangulation of the same surface and
    the state is carried over barycentrically (``init_transfer``; cascade.transfer_space is the specification).  Nested and located
    levels may be mixed; a level with both keys or with neither raises ``ValueError``.

    ``level_tol``: the tolerance of the levels below the finest (default ``tol``).  The other keywords are ``solver_socp``'s: ``nit``
    holds per level, ``time_limit`` for the whole call (a level gets the time that is left), ``init_solution`` starts the coarsest
    level, ``tol_checkpoints`` belong to the finest level.  Every level starts as a warm start through ``init_solution`` does (r = 1,
    the initial z scaling, a fresh penalty schedule, validator and history); the coarse solver is released before the finer factor
    is built.  All levels have one time grid here; ``solver_socp_spacetime_cascade`` coarsens the time grid along with the mesh.

    Returns ``(solution, run_history)`` of the finest level; ``run_history.solver_stats["mesh_cascade"]`` = {"levels": [one record
    per level: n_vertices, n_triangles, tol, iterations, running_time, setup_seconds, prolong_ms and prolong_bytes (None on the coarsest
    level), cost, kkt_max, device_bytes, transfer ("nested" | "located", None on the coarsest level), max_distance (of a located
    level, else None)], "total_seconds"}.  ``read_out``, ``flow_map`` and ``sensitivity``: as for ``solver_socp``, for the finest level."""
    flow_map = check_flow_map(flow_map, kwargs.get("time_slab"), n_time)
    sensitivity = check_sensitivity(sensitivity, kwargs.get("time_slab"), kwargs.get("congestion", 0.0))
    geometries, level_tol, opts = _mesh_cascade_options(geometries, level_tol, kwargs)
    return _run_levels([_carried(geom, i, n_time=n_time) for i, geom in enumerate(geometries)], "mesh_cascade",
                       lambda alm, hist, setup, i: _mesh_record(alm, hist, setup, geometries[i], i == 0), level_tol, opts, read_out, flow_map, sensitivity)


# ---- coarse-to-fine cascade in space and time at once ----------------------------------------------------------------------------
def _spacetime_cascade_options(n_time, geometries, levels, level_tol, kwargs):
    """The checks of solver_socp_spacetime_cascade, before any device is touched: (geometries, levels, level_tol, options)."""
    from .. import cascade

    geometries, level_tol, opts = _mesh_cascade_options(geometries, level_tol, kwargs, who="solver_socp_spacetime_cascade")
    levels = _check_lap_solver(opts, cascade.check_spacetime_levels(levels, n_time, len(geometries)))
    _check_preconditioner(opts)
    return geometries, levels, level_tol, opts


def solver_socp_spacetime_cascade(n_time, geometries, levels=None, level_tol=None, read_out=None, flow_map=None, sensitivity=None, **kwargs):
    """``solver_socp`` through a coarse-to-fine cascade in space AND time: the meshes ``geometries`` (coarse to fine, each level above the
    first with ``parents`` or ``transfer``, as for ``solver_socp_mesh_cascade``) are solved on the time grids ``levels`` (one ``n_time`` per
    geometry, never decreasing, the last one ``n_time``, each one valid for the Laplacian solver).  A level that is coarser in both
    directions costs about an eighth of the one above it.  Where two neighbouring levels have one ``n_time`` the state is carried as
    ``solver_socp_mesh_cascade`` carries it, so ``levels=[n_time] * len(geometries)`` is that driver bit for bit; where they differ,
    mesh and time grid change in one pass on the device (AlmSolver ``init_regrid``; cascade.carry_spacetime is the specification: space
    first, then time).  A step that changes the time grid alone, on one mesh, is ``solver_socp_cascade``'s.

    ``levels=None``: from the finest level downward ``n_time + 1`` is halved per mesh level while it is even and the half stays >= 16
    nodes, then held (127 with three meshes -> 31, 63, 127; 31 -> 15, 15, 31; 20 -> 20, 20).  Everything else is as for
    ``solver_socp_mesh_cascade``: ``level_tol``, ``nit`` per level, ``time_limit`` for the whole call, ``init_solution`` for the coarsest
    level, the coarse solver released before the finer factor is built.

    Returns ``(solution, run_history)`` of the finest level; ``run_history.solver_stats["spacetime_cascade"]`` = {"levels": [the records of
    ``solver_socp_mesh_cascade`` plus ``n_time``], "total_seconds"}.  ``read_out``, ``flow_map`` and ``sensitivity``: as for
    ``solver_socp``, for the finest level."""
    flow_map = check_flow_map(flow_map, kwargs.get("time_slab"), n_time)
    sensitivity = check_sensitivity(sensitivity, kwargs.get("time_slab"), kwargs.get("congestion", 0.0))
    geometries, levels, level_tol, opts = _spacetime_cascade_options(n_time, geometries, levels, level_tol, kwargs)
    return _run_levels([_carried(geom, i, n_time=T, init_regrid=bool(i) and T != levels[i - 1]) for i, (T, geom) in enumerate(zip(levels, geometries))],
                       "spacetime_cascade",
                       lambda alm, hist, setup, i: {"n_time": int(levels[i]), **_mesh_record(alm, hist, setup, geometries[i], i == 0)},
                       level_tol, opts, read_out, flow_map, sensitivity)


# ---- a cascade in space from ONE geometry: the levels are made here ----------------------------------------------------------------
def _auto_cascade_options(n_time, coarse_levels, ratio, locate, spacetime, levels, level_tol, kwargs):
    """The checks of solver_socp_auto_cascade, before the levels are built and any device is touched: the number of coarse levels."""
    from .. import cascade

    who = "solver_socp_auto_cascade"
    if isinstance(coarse_levels, bool) or not isinstance(coarse_levels, (int, np.integer)) or coarse_levels < 0:
        raise ValueError(f"{who}: coarse_levels must be an integer >= 0")
    if not (isinstance(ratio, (int, float)) and ratio > 1):
        raise ValueError(f"{who}: ratio must be a number > 1")
    cascade.check_locate(locate, who)
    for key in ("time_slab", "init_from", "init_parents", "init_transfer"):
        if key in kwargs:
            raise ValueError(f"{who}: {key} is not an option of the cascade in space")
    _check_option_names(who, kwargs)
    if levels is not None and not spacetime:
        raise ValueError(f"{who}: levels (one n_time per mesh level) needs spacetime=True")
    _common_cascade_checks(kwargs, level_tol, lambda: cascade.check_spacetime_levels(levels, n_time, int(coarse_levels) + 1) if spacetime else [n_time],
                           level_tol_optional=True)
    return int(coarse_levels)


def solver_socp_auto_cascade(n_time, geometry, coarse_levels=2, ratio=4.0, locate="device", spacetime=False, levels=None, level_tol=None,
                             read_out=None, flow_map=None, sensitivity=None, **kwargs):
    """``solver_socp`` through a cascade in space for a caller with ONE geometry: ``coarse_levels`` coarser meshes are made of it
    (``meshes.coarsen_levels``: half-edge-collapse decimation by ``ratio`` per level on the host, every level located on the one below
    with ``locate`` -- "device": ``dots_mesh_locate`` on the solver's GPU --, ``mu0`` / ``mu1`` restricted), then the levels are handed
    to ``solver_socp_mesh_cascade``, or with ``spacetime=True`` to ``solver_socp_spacetime_cascade`` (``levels``: its ``n_time`` per mesh
    level).  ``coarse_levels=0`` is ``solver_socp``.  The other keywords are those drivers'; ``time_limit`` covers the build (the
    cascade gets the time that is left).

    Returns ``(solution, run_history)`` of ``geometry``; ``run_history.solver_stats["auto_cascade"]`` = {"levels": [one record per
    coarse level, coarse to fine: n_vertices, n_triangles, coarsen_seconds, locate_seconds, locate, max_distance (of the level above
    from it)], "build_seconds"} next to the record of the driver that ran.  ``ValueError`` where ``meshes.coarsen_levels`` raises (a
    mesh that does not coarsen); every option is checked before the levels are built."""
    from .. import meshes

    flow_map = check_flow_map(flow_map, kwargs.get("time_slab"), n_time)
    sensitivity = check_sensitivity(sensitivity, kwargs.get("time_slab"), kwargs.get("congestion", 0.0))
    n_coarse = _auto_cascade_options(n_time, coarse_levels, ratio, locate, spacetime, levels, level_tol, kwargs)
    if n_coarse == 0:
        return solver_socp(n_time, geometry, read_out=read_out, flow_map=flow_map, sensitivity=sensitivity, **kwargs)
    t_start = time.perf_counter()
    geometries = meshes.coarsen_levels(geometry, n_coarse + 1, ratio=ratio, locate=locate, device=kwargs.get("device", 0))
    build = time.perf_counter() - t_start
    records = [dict(g["build"], n_vertices=int(np.asarray(g["vertices"]).shape[0]), n_triangles=int(np.asarray(g["triangles"]).shape[0]),
                    max_distance=_max_distance(above)) for g, above in zip(geometries, geometries[1:])]
    opts = dict(kwargs)
    opts["time_limit"] = max(opts.get("time_limit", 1000) - build, 0.0)
    if spacetime:
        solution, hist = solver_socp_spacetime_cascade(n_time, geometries, levels=levels, level_tol=level_tol, read_out=read_out, flow_map=flow_map, sensitivity=sensitivity, **opts)
    else:
        solution, hist = solver_socp_mesh_cascade(n_time, geometries, level_tol=level_tol, read_out=read_out, flow_map=flow_map, sensitivity=sensitivity, **opts)
    hist.solver_stats["auto_cascade"] = {"levels": records, "build_seconds": build}
    return solution, hist


# ---- Wasserstein barycentres: mirror descent over one batch session, iterated on the device -------------------------------------------
BARYCENTER_SOLVE_KEYS = ("tol", "nit", "congestion")      # per problem, the same for all K


def barycenter(n_time, geometry, measures, weights=None, steps=20, eta=100.0, tol_change=None, init=None, to_device=False, **options):
    """The Wasserstein barycentre ``nu`` of ``measures`` on the surface of ``geometry``: the minimiser of ``sum_k w_k cost(nu, mu_k)``,
    by mirror descent on the simplex (``dots_socp_amd.barycenter``: ``barycenter_host`` is this loop on the host, ``update_host`` the
    specification of the update).  ``measures``: (K, V) or a list of K arrays (V,) of one total mass, 1 <= K <= 16; ``weights`` (K,),
    default ``1 / K`` -- with two measures and the weights ``(1 - t, t)`` the displacement interpolation at ``t``.

    One ``BatchSession`` carries the loop.  Per outer step the K problems ``(nu -> mu_k)`` are solved together (``solve_many``: cold
    in step 0, from their last iterates afterwards), their potentials at the first end are read out on the device
    (``sensitivity(to_device=True)``), ``DeviceProblem.barycenter_update`` (dots_barycenter_update, a call without a context) moves ``nu`` where it lies, and
    the next solves restart from it there (``DeviceOrdered``).  From step 1 on only scalars cross to the host: the residuals and
    costs of the solves, the four scalars of the update.  The costs of step s belong to the ``nu`` before its update; if the
    objective of step s exceeds that of step s - 1, ``eta`` is halved for the updates from step s on.  Ends after ``steps`` steps or
    when ``change < tol_change * mass``.

    ``init`` (V,): the start, every entry positive (a multiplicative update cannot create support); default ``0.5 * sum_k w_k mu_k +
    0.5 * mass * area_vertices / sum(area_vertices)``.  ``eta`` = 100 suits masses of total 1 on a surface of diameter about 1: the
    potentials scale with the squared distances, and ``eta * gmax`` (``solver_stats["updates"]``) of order 1 is the working range.
    ``options``: those of ``BatchSession`` (``max_batch`` and ``slots`` default to K) and ``tol``, ``nit``, ``congestion`` of every solve.

    Returns ``{"nu" (V,) (a torch tensor on the device with ``to_device``), "objective" [per step], "change" [per step], "costs" (K,)
    of the last step, "eta" [per step], "iterations" [per step, summed over the K problems], "solver_stats": {"updates" [per step:
    sum, change, gmax, min], "update_ms" [per step], "solve_seconds" and "step_seconds" [per step], "bytes_to_host" [per step:
    dots_debug_counter 9 of the session's contexts and the 32 bytes of the update's scalars], "session" (of the last solves)}}``."""
    import torch

    from .. import barycenter as bary
    from . import _geometry_with_areas

    who = "barycenter"
    if not isinstance(geometry, dict) or "vertices" not in geometry or "triangles" not in geometry:
        raise ValueError(f"{who}: geometry must be a dict with 'vertices' and 'triangles'")
    V = int(np.asarray(geometry["vertices"]).shape[0])
    m, w, mass = bary.check_measures(who, measures, weights, V)
    K = m.shape[0]
    if int(steps) < 1:
        raise ValueError(f"{who}: steps must be at least 1")
    if not (math.isfinite(float(eta)) and float(eta) >= 0.0):
        raise ValueError(f"{who}: eta must be finite and not negative")
    if options.get("is_constant_scaling"):
        raise ValueError(f"{who}: is_constant_scaling reads the end masses on the host: not available")
    per_solve = {k: options.pop(k) for k in BARYCENTER_SOLVE_KEYS if k in options}
    session_kw = {"max_batch": K, "slots": K, **options}
    g = _geometry_with_areas(geometry)
    nu0 = bary.default_start(m, w, g["area_vertices"], mass) if init is None else _host_array(init)
    nu0 = bary.check_start(who, nu0, V)
    request = {"potentials": True, "stress": False, "to_device": True}
    rule = bary.StepRule(eta)
    out = {"objective": [], "change": [], "eta": [], "iterations": [], "costs": None}
    stats = {"updates": [], "update_ms": [], "solve_seconds": [], "step_seconds": [], "bytes_to_host": []}
    with BatchSession(n_time, _without_masses(g), **session_kw) as bs:
        nu = nu_ordered = targets = dev = None
        for step in range(int(steps)):
            t0 = time.perf_counter()
            copied = sum(alm.dev.debug_counter(9) for alm in bs._live())
            if step == 0:
                problems = [{"mu0": nu0, "mu1": m[k], **per_solve} for k in range(K)]
            else:
                problems = [{"mu0": DeviceOrdered(nu_ordered), "mu1": DeviceOrdered(targets[k]), **per_solve} for k in range(K)]
            results = bs.solve_many(problems, warm=step > 0, outputs=(), sensitivity=request)
            stats["solve_seconds"].append(time.perf_counter() - t0)
            if step == 0:      # the masses move to the device once: nu in the caller's numbering, the targets in the contexts'
                dev = bs.solvers[0].dev
                where = torch.device("cuda", dev.device)
                perm = dev.plan.perm_vert
                nu = torch.as_tensor(nu0, dtype=torch.float64, device=where).contiguous()
                nu_ordered = torch.empty_like(nu)
                targets = [torch.as_tensor(np.ascontiguousarray(m[k] if perm is None else m[k][perm]), dtype=torch.float64, device=where) for k in range(K)]
            costs = [float(hist.history["Transportation cost"][-1]) for _, hist in results]
            potentials = [sol["sensitivity"]["phi0"] for sol, _ in results]
            objective = bary.objective_of(costs, w)
            step_eta = rule.take(objective)
            scalars = dev.barycenter_update(potentials, w, step_eta, mass, nu, nu_ordered)
            out["objective"].append(objective)
            out["change"].append(scalars["change"])
            out["eta"].append(step_eta)
            out["iterations"].append(int(sum(int(hist.kkt_iteration[-1]) + 1 for _, hist in results)))
            out["costs"] = np.asarray(costs)
            stats["updates"].append(scalars)
            stats["update_ms"].append(dev.barycenter_ms)
            stats["session"] = [hist.solver_stats.get("session") for _, hist in results]
            stats["step_seconds"].append(time.perf_counter() - t0)
            stats["bytes_to_host"].append(int(sum(alm.dev.debug_counter(9) for alm in bs._live()) - copied) + 32)      # (+ the update's four scalars)
            if tol_change is not None and scalars["change"] < float(tol_change) * mass:
                break
        out["nu"] = nu.clone() if to_device else nu.cpu().numpy()
    out["solver_stats"] = stats
    return out


# ---- linearised transport: tangent vectors at one reference measure and their Gram matrix, formed on the device ------------------------
TANGENT_SOLVE_KEYS = BARYCENTER_SOLVE_KEYS      # per problem, the same for all N


def _tangent_arguments(who, geometry, options):
    """The checks the two drivers share, before the library loads: the mesh's vertex count, the options split into those of every
    solve and those of the session."""
    if not isinstance(geometry, dict) or "vertices" not in geometry or "triangles" not in geometry:
        raise ValueError(f"{who}: geometry must be a dict with 'vertices' and 'triangles'")
    if options.get("time_slab") is not None:
        raise ValueError(f"{who}: not available on time slabs")
    if options.get("is_constant_scaling"):
        raise ValueError(f"{who}: is_constant_scaling is not available: the problems share one session whose contexts are restarted")
    options = {k: v for k, v in options.items() if k != "time_slab"}
    per_solve = {k: options.pop(k) for k in TANGENT_SOLVE_KEYS if k in options}
    unknown = set(options) - set(COMMON_KEYS) - set(BATCH_SESSION_FIXED) - {"max_batch"}
    if unknown:
        raise ValueError(f"{who}: unknown option(s) {sorted(unknown)}")
    return int(np.asarray(geometry["vertices"]).shape[0]), per_solve, options


def _tangent_session(n_problems, slots, session_kw):
    """``max_batch`` and ``slots`` of a session for ``n_problems`` cold problems: at most 8 run at a time unless asked otherwise; a
    slot that finishes takes the next problem, so the problems are not limited to the slots."""
    max_batch = int(session_kw.pop("max_batch", min(n_problems, 8)))
    return {"max_batch": max_batch, "slots": max(max_batch, min(n_problems, int(slots))) if slots is not None else max_batch, **session_kw}


def tangent_embedding(n_time, geometry, reference, measures, velocities=False, to_device=False, slots=None, **options):
    """The linearised-transport embedding of ``measures`` at the measure ``reference`` on the surface of ``geometry``
    (``dots_socp_amd.tangent``: ``tangent_embedding_host`` is this driver on the host, ``velocities_host``, ``weights_host`` and
    ``gram_host`` the specifications of the device calls).  The N problems ``(reference -> mu_i)`` are solved, their initial velocities
    ``v_i = +grad phi0_i`` -- the logarithmic map at the reference -- are formed per triangle, and ``G_ij = sum_f w_f v_i[f] . v_j[f]``
    with ``w_f`` the reference's mass on triangle ``f`` is their Gram matrix in L2(reference): ``G_ii + G_jj - 2 G_ij`` approximates
    ``W2^2(mu_i, mu_j)`` (half of it is on the scale of "Transportation cost"; ``G_ii / 2`` is the cost of problem i up to the
    discretisation), and PCA, clustering and kernels need no further solve.

    ``reference`` (V,) and ``measures`` ((N, V) or a list of N arrays (V,)): finite, non-negative, of one total mass; N >= 1 has no
    upper limit.  One ``BatchSession`` solves the N problems cold (``solve_many``: ``max_batch`` of them at a time, default min(N, 8);
    ``slots`` contexts, default ``max_batch``; a slot that finishes takes the next problem) with their potentials read out on the
    device (``sensitivity(to_device=True)``); then the velocities, the weights and the Gram matrix are formed there
    (``DeviceProblem.tangent_velocities`` / ``tangent_weights`` / ``tangent_gram``: dots_tangent_*, calls without a context).
    Besides the residuals and costs of the solves only ``G`` crosses to the host, 8 N^2 bytes -- and the weights (8 F) and, if asked
    for, the velocities (24 N F), unless ``to_device``.  Device memory: N F 3 doubles for the velocities and N V for the potentials,
    besides the session's.  ``options``: those of ``BatchSession`` and ``tol``, ``nit``, ``congestion`` of every solve.  Not on time
    slabs, not with ``is_constant_scaling``.

    Returns ``{"gram" (N, N), "costs" (N,), "squared_distances" (N, N), "iterations" (N,), "weights" (F,), "velocities" (N, F, 3) with
    ``velocities=True`` (else None) -- ``weights`` and ``velocities`` are torch tensors on the device with ``to_device`` --,
    "solver_stats": {"solve_seconds", "seconds", "tangent_ms" {"velocities", "weights", "gram"}, "bytes_to_host" (after the solves:
    dots_debug_counter 9 of the session's contexts and the bytes of G, the weights and the velocities that crossed), "session"}}``."""
    import torch

    from .. import tangent as tg

    who = "tangent_embedding"
    t0 = time.perf_counter()
    V, per_solve, session_kw = _tangent_arguments(who, geometry, dict(options))
    sigma, m, _ = tg.check_embedding(who, reference, measures, V)
    N = m.shape[0]
    request = {"potentials": True, "stress": False, "to_device": True}
    with BatchSession(n_time, _without_masses(geometry), **_tangent_session(N, slots, session_kw)) as bs:
        results = bs.solve_many([{"mu0": sigma, "mu1": m[i], **per_solve} for i in range(N)], outputs=(), sensitivity=request)
        solved = time.perf_counter()
        copied = sum(alm.dev.debug_counter(9) for alm in bs._live())
        dev = bs.solvers[0].dev
        potentials = [sol["sensitivity"]["phi0"] for sol, _ in results]
        vel = dev.tangent_velocities(potentials)
        w = dev.tangent_weights(torch.as_tensor(sigma, dtype=torch.float64, device=vel.device))
        G = dev.tangent_gram(vel, None, w)
        crossed = int(sum(alm.dev.debug_counter(9) for alm in bs._live()) - copied) + G.nbytes
        tangent_ms = dict(dev.tangent_ms)
        if not to_device:
            crossed += 8 * w.numel() + (8 * vel.numel() if velocities else 0)
            w, vel = w.cpu().numpy(), vel.cpu().numpy() if velocities else None
    return {"gram": G, "costs": np.array([float(hist.history["Transportation cost"][-1]) for _, hist in results]),
            "squared_distances": tg.squared_distances(G), "iterations": np.array([int(hist.kkt_iteration[-1]) + 1 for _, hist in results]),
            "weights": w, "velocities": vel if velocities else None,
            "solver_stats": {"solve_seconds": solved - t0, "seconds": time.perf_counter() - t0, "tangent_ms": tangent_ms, "bytes_to_host": crossed,
                             "session": [hist.solver_stats.get("session") for _, hist in results]}}


def distance_matrix(n_time, geometry, measures, method="tangent", reference=None, slots=None, **options):
    """The transport costs between every two of ``measures`` ((N, V), one total mass) on the surface of ``geometry``: (N, N), symmetric,
    zero on the diagonal, on the scale of "Transportation cost" (``W2^2 / 2``).
    ``method="tangent"``: ``squared_distances / 2`` of ``tangent_embedding`` at ``reference`` (default: the mean of the measures, summed
    in their order) -- N solves; an approximation, good where the measures lie near the reference in the transport's sense.
    ``method="pairs"``: the N (N - 1) / 2 problems ``(mu_i -> mu_j)``, i < j, solved exactly and cold through one ``BatchSession`` -- the
    yardstick the linearisation is judged by.  ``options``: as for ``tangent_embedding``."""
    from .. import tangent as tg

    who = "distance_matrix"
    if method not in ("tangent", "pairs"):
        raise ValueError(f"{who}: method must be 'tangent' or 'pairs'")
    V, per_solve, session_kw = _tangent_arguments(who, geometry, dict(options))
    rows = list(measures)
    if not rows:
        raise ValueError(f"{who}: no measures")
    _, m, _ = tg.check_embedding(who, rows[0], rows, V)
    N = m.shape[0]
    if method == "tangent":
        if reference is None:
            reference = np.zeros(V)
            for i in range(N):
                reference = reference + m[i]
            reference = reference / N
        return 0.5 * tangent_embedding(n_time, geometry, reference, m, slots=slots, **options)["squared_distances"]
    if reference is not None:
        raise ValueError(f"{who}: method='pairs' takes no reference")
    D = np.zeros((N, N))
    pairs = [(i, j) for i in range(N) for j in range(i + 1, N)]
    if not pairs:
        return D
    with BatchSession(n_time, _without_masses(geometry), **_tangent_session(len(pairs), slots, session_kw)) as bs:
        results = bs.solve_many([{"mu0": m[i], "mu1": m[j], **per_solve} for i, j in pairs], outputs=())
    for (i, j), (_, hist) in zip(pairs, results):
        D[i, j] = D[j, i] = float(hist.history["Transportation cost"][-1])
    return D

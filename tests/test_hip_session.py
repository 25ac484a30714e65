"""GPU tests of the solve session: dots_restart, AlmSolver.restart, socp.SolveSession and transport_cost(session=).  A solver that is
restarted on its live context must compute what a new solver computes, bit for bit: cold against a new solver from zero, warm against
a new solver with ``init_solution=`` the twelve arrays of the first one's solution.  Every comparison is np.array_equal with NaN
positions equal, over the iteration count, the whole KKT history, the cost, every downloaded state array and the dots_get_params
record.  Cases, caps and the bar of the warm torch function: session_checks.py."""
import ctypes as C

import numpy as np
import pytest

import session_checks as sc
from conftest import has_gpu
from dots_socp_amd import _lib, meshes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

STATE = tuple(_lib.ARRAY_IDS)
NAMES = tuple(sc.CASES)


def AlmSolver(*a, **kw):
    from dots_socp_amd.socp.solver_socp import AlmSolver as cls

    return cls(*a, **kw)


def params_record(dev):
    p = _lib.Params()
    _lib.check(dev.lib.dots_get_params(dev._h, C.byref(p)), "dots_get_params")
    return {name: getattr(p, name) for name, _ in _lib.Params._fields_}


def run(alm, steps=None):
    for _ in range(alm.nit if steps is None else steps):
        if alm.iterate():
            break
    return alm


def record(alm, **finalize):
    """What a run leaves, after ``finalize``: everything the identities compare."""
    solution, hist = alm.finalize(**finalize)
    out = {"iterations": np.array(alm.counter_main), "kkt_errors": np.array(hist.kkt_errors, dtype=np.float64),
           "kkt_iteration": np.array(hist.kkt_iteration), "cost": np.array(hist.history["Transportation cost"]),
           "objective": np.array(hist.history["Objective value"]), "scalars": np.array([alm.r, alm.scale_z, alm.prim_scale, alm.dual_scale]),
           "params": np.array(list(params_record(alm.dev).values()), dtype=np.float64)}
    for name in STATE:
        out["raw " + name] = alm.dev.download(name)
        if name in solution:
            out["solution " + name] = solution[name]
    return out, solution


def assert_same(got, want, skip=()):
    assert set(got) == set(want)
    for k in want:
        if k not in skip:
            assert np.array_equal(got[k], want[k], equal_nan=True), f"{k} differs"


def options_of(name, **more):
    n_time, cap = sc.CASES[name]
    return n_time, dict(tol=sc.TOL, nit=cap, **more)


def fresh(name, which=2, init_solution=None, **more):
    n_time, opts = options_of(name, **more)
    alm = AlmSolver(n_time, sc.geometry(name, which), init_solution=init_solution, **opts)
    try:
        return record(run(alm))
    finally:
        alm.close()


_shared = {}


def fresh_p2(name):
    """The new solver's solve of P2, computed once per case and left unchanged."""
    if name not in _shared:
        _shared[name] = fresh(name)[0]
    return _shared[name]


def whole(solution):
    return {k: solution[k] for k in STATE}


# ---- premise -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_premise_two_new_solves_are_bit_identical(name):
    """If this fails the factor build is not reproducible and no identity below can hold against a solver with its own factor."""
    assert_same(fresh(name)[0], fresh_p2(name))
    if name == "torus":      # the device numbering differs from the caller's
        from dots_socp_amd.geometry import build_plan

        plan = build_plan(sc.CASES[name][0], sc.geometry(name), reorder="nd")
        assert not np.array_equal(plan.perm_vert, np.arange(plan.n_vertices))
    if name == "icosphere1":      # 17 nodes: a padded time pitch
        assert sc.CASES[name][0] + 1 == 17


def test_one_case_converges_before_its_cap():
    assert int(fresh_p2("plane")["iterations"]) + 1 < sc.CASES["plane"][1]


# ---- cold and warm identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_cold_restart_equals_a_new_solver(name):
    n_time, opts = options_of(name)
    _, p1, p2 = sc.problems(name)
    alm = AlmSolver(n_time, sc.geometry(name, 1), **opts)
    try:
        run(alm).finalize(download=False)
        alm.restart(*p2, warm=False)
        assert_same(record(run(alm))[0], fresh_p2(name))
        # three restarts in a row, from a finalised solver, a fresh one and one that has not run
        alm.restart(*p1, warm=False)
        alm.restart(*p2, warm=True)
        alm.restart(*p2, warm=False)
        assert_same(record(run(alm))[0], fresh_p2(name))
    finally:
        alm.close()


@pytest.mark.parametrize("name", NAMES)
def test_warm_restart_equals_a_new_solver_with_init_solution(name):
    n_time, opts = options_of(name)
    _, _, p2 = sc.problems(name)
    alm = AlmSolver(n_time, sc.geometry(name, 1), **opts)
    try:
        _, first = record(run(alm))
        alm.restart(*p2, warm=True)
        got = record(run(alm))[0]
    finally:
        alm.close()
    want = fresh(name, init_solution=whole(first))[0]
    assert_same(got, want)
    assert not np.array_equal(got["kkt_errors"], fresh_p2(name)["kkt_errors"], equal_nan=True)      # (it is another run than the cold one)


# ---- live flags: a restart in the middle of a run, without finalize or any download ----------------------------------------------------
def live_solver(name):
    """A solver of P1 stopped after sc.LIVE_STOP iterations of a run that goes on (tight tolerance, far cap).  37 iterations end on a
    quiet one (no penalty update is due at iteration 36 and the validator is not; z_mid is then not stored, so neither a warm restart
    nor the twin's finalize is possible); iteration 38 is a penalty update of the schedule (control.AdjustAdmmParam: 24, 31, 38):
    it reads back (z_mid deferred), leaves the division pending and arms the decision ahead, whose launch is on the stream."""
    n_time, _ = sc.CASES[name]
    alm = AlmSolver(n_time, sc.geometry(name, 1), tol=1e-12, nit=4000)
    run(alm, sc.LIVE_STOP - 1)
    before, ahead = alm.r, alm.dev.debug_counter(2)      # (penalty decisions the library has taken ahead of the host so far)
    run(alm, 1)
    assert alm.counter_main == sc.LIVE_STOP - 1 and not alm.finished
    live = {"update": alm.adjust_params.last_it == sc.LIVE_STOP - 1, "read_back": bool(alm._fused_kkt) and not alm._last_quiet,
            "division": alm.r != before, "ahead": alm.dev.debug_counter(2) > ahead}
    return alm, live


@pytest.mark.parametrize("name", NAMES)
def test_live_flags_warm(name):
    _, _, p2 = sc.problems(name)
    n_time, opts = options_of(name)
    twin, live = live_solver(name)
    try:
        first, _ = twin.finalize()      # the host path: flushes the division, materialises z_mid, downloads
    finally:
        twin.close()
    assert live["update"] and live["read_back"], live
    assert live["division"] or live["ahead"], live      # a pending division (r moved) or a launch ahead is live at the restart
    want = fresh(name, init_solution=whole(first))[0]
    alm, live2 = live_solver(name)
    try:
        assert live2 == live
        alm.restart(*p2, warm=True, **opts)      # no finalize, no download
        assert_same(record(run(alm))[0], want)
    finally:
        alm.close()


@pytest.mark.parametrize("name", NAMES)
def test_live_flags_cold(name):
    """The leftovers (stale z_mid storage, pending division, launch ahead) must not leak into a zeroed state."""
    _, _, p2 = sc.problems(name)
    _, opts = options_of(name)
    alm, live = live_solver(name)
    try:
        assert live["update"] and live["read_back"], live
        alm.restart(*p2, warm=False, **opts)
        assert_same(record(run(alm))[0], fresh_p2(name))
    finally:
        alm.close()


def test_a_quiet_last_iteration_refuses_a_warm_restart_and_takes_a_cold_one():
    name = "plane"
    _, _, p2 = sc.problems(name)
    n_time, opts = options_of(name)
    alm = AlmSolver(n_time, sc.geometry(name, 1), tol=1e-12, nit=4000)
    try:
        run(alm, 37)
        assert alm._last_quiet
        with pytest.raises(ValueError, match="stored no z_mid"):
            alm.restart(*p2, warm=True)
        d = _lib.RestartDesc()      # the library refuses the same, and leaves the context alone
        m0, m1 = (np.ascontiguousarray(a) for a in p2)
        d.mu0, d.mu1, d.mode = m0.ctypes.data, m1.ctypes.data, _lib.RESTART_WARM
        for i in range(4):
            d.factors[i] = 1.0
        assert alm.dev.lib.dots_restart(alm.dev._h, C.byref(d)) == _lib.ERR_STATE
        alm.restart(*p2, warm=False, **opts)
        assert_same(record(run(alm))[0], fresh_p2(name))
    finally:
        alm.close()


# ---- option variants -----------------------------------------------------------------------------------------------------------------
VARIANTS = {
    "congestion": dict(congestion=0.01),
    "constant_scaling": dict(is_constant_scaling=True),
    "palm": dict(is_palm=True),
    "pcg_jacobi": dict(lap_solver="modal_pcg", preconditioner="jacobi"),
    "pcg_multigrid": dict(lap_solver="modal_pcg", preconditioner="multigrid", mg_coarsest=32),
    "step_by_step": dict(check_kkt_step_by_step=True),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_option_variants_cold_and_warm(variant):
    name, more = "torus", VARIANTS[variant]
    n_time, opts = options_of(name, **more)
    _, _, p2 = sc.problems(name)
    cold = fresh(name, **more)[0]
    alm = AlmSolver(n_time, sc.geometry(name, 1), **opts)
    try:
        _, first = record(run(alm))
        alm.restart(*p2, warm=False)
        assert_same(record(run(alm))[0], cold)
        alm.restart(*sc.problems(name)[1], warm=False)
        _, again = record(run(alm))
        assert_same(whole(again), whole(first))
        alm.restart(*p2, warm=True)
        got = record(run(alm))[0]
    finally:
        alm.close()
    assert_same(got, fresh(name, init_solution=whole(first), **more)[0])


# ---- derived outputs after a session solve ---------------------------------------------------------------------------------------------
def same_tree(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            if k not in ("ms", "bytes"):
                same_tree(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same_tree(x, y, f"{path}/{i}")
    elif a is None or isinstance(a, (str, bool)):
        assert a == b, path
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), path


@pytest.mark.parametrize("request_", ({"read_out": {"dot_units": True, "centred": True}}, {"sensitivity": True, "outputs": ("phi", "mu")},
                                      {"flow_map": {"starts": "vertices", "push": True}, "outputs": ()}), ids=("read_out", "sensitivity", "flow_map"))
def test_derived_outputs_after_a_session_solve(request_):
    from dots_socp_amd.socp import SolveSession, solver_socp

    name = "torus"
    n_time, opts = options_of(name)
    mesh, p1, p2 = sc.problems(name)
    want, hist_w = solver_socp(n_time, sc.geometry(name), **opts, **request_)
    with SolveSession(n_time, mesh, **opts) as s:
        s.solve(*p1, outputs=())
        got, hist = s.solve(*p2, warm=False, **request_)
        stats = hist.solver_stats["session"]
        assert stats["index"] == 1 and stats["warm"] is False and stats["restart_ms"] > 0.0 and stats["setup_seconds_saved"] == s.setup_seconds
        got2, _ = s.solve(*p2, warm=False, **request_)      # ... and finalize is repeatable on one solver
    same_tree(got, want)
    same_tree(got2, want)
    assert np.array_equal(hist.kkt_errors, hist_w.kkt_errors, equal_nan=True)
    if "read_out" in request_:
        same_tree(hist.solver_stats["readout"], hist_w.solver_stats["readout"])


# ---- nothing rebuilt -----------------------------------------------------------------------------------------------------------------
def test_nothing_is_rebuilt_across_restarts(monkeypatch):
    from dots_socp_amd.device import DeviceProblem
    from dots_socp_amd.socp import SolveSession

    calls = []
    original = DeviceProblem.setup_frontal
    monkeypatch.setattr(DeviceProblem, "setup_frontal", lambda self, *a, **kw: (calls.append(1), original(self, *a, **kw))[1])
    name = "torus"
    n_time, opts = options_of(name)
    mesh, p1, p2 = sc.problems(name)

    def front_info(dev):
        info = (C.c_double * 4)()
        _lib.check(dev.lib.dots_front_info(dev._h, info), "dots_front_info")
        return list(info), dev.debug_counter(10), dev.front_launches()

    with SolveSession(n_time, mesh, **opts) as s:
        s.solve(*p1, outputs=(), nit=40)
        dev, plan = s.alm.dev, s.alm.dev.plan
        nbytes, info = dev.device_bytes(), front_info(dev)
        for i in range(5):
            s.solve(*(p2 if i % 2 == 0 else p1), warm=bool(i % 3), outputs=())
            assert s.alm.dev is dev and dev.device_bytes() == nbytes and front_info(dev) == info
            assert dev.plan.dissection is plan.dissection and dev.plan.lap_val is plan.lap_val
        assert s.index == 6
    assert calls == [1]


# ---- device pointers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("warm", (False, True))
def test_device_pointers_equal_host_arrays_up_to_norm_boundary(name, warm):
    import torch

    n_time, opts = options_of(name)
    _, _, p2 = sc.problems(name)
    out = []
    for on_device in (False, True):
        alm = AlmSolver(n_time, sc.geometry(name, 1), **opts)
        try:
            run(alm, sc.LIVE_STOP)      # (ends on a read-back: the iterate is whole)
            masses = [torch.tensor(a, dtype=torch.float64, device="cuda") for a in p2] if on_device else p2
            alm.restart(*masses, warm=warm)
            perm = alm.dev.plan.perm_vert
            assert np.array_equal(alm.geometry["mu1"], p2[1]) and np.array_equal(alm.dev.plan.mu0, p2[0] if perm is None else p2[0][perm])
            out.append(({"raw " + k: alm.dev.download(k) for k in STATE}, params_record(alm.dev), alm.norm_boundary))
        finally:
            alm.close()
    (state_h, params_h, nb_h), (state_d, params_d, nb_d) = out
    assert_same(state_d, state_h)
    for k in params_h:
        if k != "norm_boundary":
            assert params_d[k] == params_h[k], k
    V = p2[0].shape[0]
    assert abs(params_d["norm_boundary"] - params_h["norm_boundary"]) <= V * 2.0 ** -53 * params_h["norm_boundary"]
    assert abs(nb_d - nb_h) <= V * 2.0 ** -53 * nb_h


def test_host_arrays_give_the_norm_boundary_of_a_new_context():
    from dots_socp_amd.device import DeviceProblem

    for name in NAMES:
        n_time, _ = sc.CASES[name]
        _, _, p2 = sc.problems(name)
        with DeviceProblem(n_time, sc.geometry(name, 1), lap_solver="modal_pcg", reorder="nd") as a, \
                DeviceProblem(n_time, sc.geometry(name, 2), lap_solver="modal_pcg", reorder="nd") as b:
            a.set_params(r=3.0, congestion=0.5, scale_z=2.0, tau=1.5, cg_tol=1e-6)
            ms = a.restart(*p2, mode="cold")
            assert ms >= 0.0
            got, want = params_record(a), params_record(b)
            assert got.pop("tau") == 1.5 and got.pop("cg_tol") == 1e-6      # kept
            want.pop("tau"), want.pop("cg_tol")
            assert got == want


def test_the_rescaling_launch_can_be_timed_alone_and_keeps_the_state():
    name = "icosphere1"
    n_time, opts = options_of(name)
    alm = AlmSolver(n_time, sc.geometry(name, 1), **opts)
    try:
        run(alm, sc.LIVE_STOP)
        before = {k: alm.dev.download(k) for k in STATE}
        ms, nbytes = alm.dev.bench_kernel(_lib.BENCH_RESTART_SCALE, reps=3)
        pitch = 32
        assert ms > 0.0 and nbytes == 2 * 8 * pitch * (8 * alm.dev.V + 42 * alm.dev.F)
        assert_same({k: alm.dev.download(k) for k in STATE}, before)
    finally:
        alm.close()


# ---- the torch function ----------------------------------------------------------------------------------------------------------------
def cost_and_gradients(name, masses, **kw):
    import torch

    from dots_socp_amd import torch_cost

    mesh = sc.problems(name)[0]
    n_time, opts = options_of(name)
    m0, m1 = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in masses)
    x = torch.tensor(mesh["vertices"], dtype=torch.float64, requires_grad=True)
    c = torch_cost.transport_cost(m0, m1, x, mesh["triangles"], n_time, **opts, **kw)
    c.backward()
    return {"cost": np.array(float(c.detach())), "mu0": m0.grad.numpy(), "mu1": m1.grad.numpy(), "vertices": x.grad.numpy()}


@pytest.mark.parametrize("name", NAMES)
def test_torch_function_with_a_session(name):
    from dots_socp_amd.socp import SolveSession

    mesh, p1, p2 = sc.problems(name)
    n_time, _ = sc.CASES[name]
    want = cost_and_gradients(name, p2)
    geom, _ = meshes.make_geometry(mesh["vertices"], mesh["triangles"], normalize=False)
    with SolveSession(n_time, geom) as s:
        cost_and_gradients(name, p1, session=s)
        cold = cost_and_gradients(name, p2, session=s, warm=False)
        assert_same(cold, want)      # bit for bit
        cost_and_gradients(name, p1, session=s, warm=False)
        warm = cost_and_gradients(name, p2, session=s, warm=True)
    ref = sc.WARM_REFERENCE[name]
    for k in ("cost", "mu0", "mu1", "vertices"):
        diff = float(np.max(np.abs(warm[k] - want[k])))
        print(f"{name}: warm against cold, {k}: {diff:.3e} (reference {ref[k]:.3e})")
        assert diff <= sc.WARM_MARGIN * ref[k], k

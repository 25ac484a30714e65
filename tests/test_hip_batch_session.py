"""GPU tests of the batch session: dots_move_vertices_many, device.move_vertices_many, socp.BatchSession and
transport_costs(session=).  The contract is bit identity: a cold ``solve_many`` with ``solver_socp_many`` on the same list, a warm
one with ``SolveSession.solve(..., warm=True)`` per problem, a moved one with the same on the moved mesh.  "Bit for bit" is
np.array_equal (NaN positions equal) over the twelve state arrays, the KKT, cost and objective histories and the stopping iteration.
Meshes, masses, caps and LIVE_STOP: session_checks.py; the displacement: move_checks.py, as test_hip_move.py uses it.

A moved mesh is compared in the session's numbering: the nested dissection of ``geometry.build_plan`` reads the positions, so the
reference on the moved mesh -- ``solver_socp_many`` or ``transport_costs`` -- is given ``plan=geometry.plan_with_vertices(<the
session's plan>, moved)``, the same mesh assembled from scratch, as the twin of test_hip_move.py is."""
import ctypes as C
import importlib

import numpy as np
import pytest

import move_checks as mc
import session_checks as sc
import test_hip_move as thm
import test_hip_session as ths
from conftest import has_gpu
from dots_socp_amd import _lib, geometry, meshes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

ss = importlib.import_module("dots_socp_amd.socp.solver_socp")
NAMES = tuple(sc.CASES)
STATE = tuple(_lib.ARRAY_IDS)


def rec(result):
    solution, hist = result
    out = {"iterations": np.array(hist.kkt_iteration[-1]), "kkt_errors": np.array(hist.kkt_errors, dtype=np.float64),
           "kkt_iteration": np.array(hist.kkt_iteration), "cost": np.array(hist.history["Transportation cost"]),
           "objective": np.array(hist.history["Objective value"])}
    for name in STATE:
        out[name] = solution[name]
    return out


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        ths.assert_same(rec(g), rec(w))


def swapped(p):
    return (p[1], p[0])


def run_options(name, **more):
    return dict(tol=sc.TOL, nit=sc.CASES[name][1], **more)


def three(name, **more):
    """P1, P2 and P1 with mu0 / mu1 swapped, each with the case's tolerance and cap"""
    _, p1, p2 = sc.problems(name)
    return [dict(mu0=m[0], mu1=m[1], **run_options(name, **more)) for m in (p1, p2, swapped(p1))]


_many = {}


def many_cold(name):
    """``solver_socp_many`` on the three problems with two at a time, computed once per case and left unchanged."""
    if name not in _many:
        from dots_socp_amd.socp import solver_socp_many

        _many[name] = solver_socp_many(sc.CASES[name][0], sc.problems(name)[0], three(name), max_batch=2)
    return _many[name]


def many_moved(mesh, plan, moved, problems):
    """``solver_socp_many`` on ``mesh`` moved to ``moved``, numbered as ``plan`` numbers it"""
    from dots_socp_amd.socp import solver_socp_many

    return solver_socp_many(plan.n_time, mc.moved_mesh(mesh, moved), problems, max_batch=2, plan=geometry.plan_with_vertices(plan, moved))


@pytest.fixture
def contexts(monkeypatch):
    """Counts the device contexts the driver creates."""
    made = []

    class Counted(ss.DeviceProblem):
        def __init__(self, *a, **kw):
            made.append(1)
            super().__init__(*a, **kw)

    monkeypatch.setattr(ss, "DeviceProblem", Counted)
    return made


# ---- 1 cold ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_cold_equals_the_batch_driver_refill_included(name, contexts):
    from dots_socp_amd.socp import BatchSession

    want = many_cold(name)
    del contexts[:]
    with BatchSession(sc.CASES[name][0], sc.problems(name)[0], max_batch=2) as bs:
        first = bs.solve_many(three(name))
        assert len(contexts) == 2
        second = bs.solve_many(three(name))
        assert len(contexts) == 2      # restarts, no new context
    same(first, want)
    same(second, want)
    for i, (_, hist) in enumerate(second):
        assert hist.solver_stats["batch"] == {**want[i][1].solver_stats["batch"]}
        s = hist.solver_stats["session"]
        assert s["index"] == 3 + i and s["warm"] is False and s["restart_ms"] > 0.0 and s["moved"] is False and s["move_ms"] is None
        assert s["setup_seconds_saved"] == first[0][1].solver_stats["session"]["setup_seconds"]
    assert [h.solver_stats["session"]["restart_ms"] is None for _, h in first] == [True, True, False]


# ---- 2 warm ---------------------------------------------------------------------------------------------------------------------------------
def single_session(name, first, then, fixed, moved=None):
    """``SolveSession.solve(first)`` followed by ``.solve(then, warm=True)`` (with ``vertices=moved``): the second result"""
    from dots_socp_amd.socp import SolveSession

    with SolveSession(sc.CASES[name][0], sc.problems(name)[0], **fixed) as s:
        s.solve(first["mu0"], first["mu1"], outputs=(), **{k: first[k] for k in first if k not in ("mu0", "mu1")})
        more = {} if moved is None else {"vertices": moved}
        return s.solve(then["mu0"], then["mu1"], warm=True, **more, **{k: then[k] for k in then if k not in ("mu0", "mu1")})


@pytest.mark.parametrize("name,variant", (("plane", "congestion"), ("torus", "constant_scaling"), ("icosphere1", "default")))
def test_warm_equals_the_single_session_per_problem(name, variant):
    from dots_socp_amd.socp import BatchSession

    _, p1, p2 = sc.problems(name)
    fixed = {k: v for k, v in sc.VARIANTS[variant].items() if k in ss.BATCH_SESSION_FIXED}
    each = run_options(name, **{k: v for k, v in sc.VARIANTS[variant].items() if k not in ss.BATCH_SESSION_FIXED})
    firsts = [dict(mu0=m[0], mu1=m[1], **each) for m in (p1, swapped(p1))]
    thens = [dict(mu0=m[0], mu1=m[1], **each) for m in (p2, swapped(p2))]
    with BatchSession(sc.CASES[name][0], sc.problems(name)[0], max_batch=2, **fixed) as bs:
        bs.solve_many(firsts, outputs=())
        got = bs.solve_many(thens, warm=True)
    assert all(h.solver_stats["session"]["warm"] is True for _, h in got)
    same(got, [single_session(name, a, b, fixed) for a, b in zip(firsts, thens)])


# ---- 3 moved --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_moved_cold_there_and_back(name, contexts):
    from dots_socp_amd.socp import BatchSession

    mesh = sc.problems(name)[0]
    moved = thm.moved_of(name)
    short = [dict(p, nit=sc.LIVE_STOP) for p in three(name)]
    with BatchSession(sc.CASES[name][0], mesh, max_batch=2) as bs:
        bs.solve_many(short, outputs=())
        plan = bs.base
        there = bs.solve_many(three(name), vertices=moved)
        s = there[0][1].solver_stats["session"]
        assert s["moved"] is True and len(s["move_ms"]) == 3 and s["move_ms"][2] >= s["move_ms"][1] > 0.0
        assert all(h.solver_stats["session"]["move_ms"] == s["move_ms"] for _, h in there)
        assert np.array_equal(bs.geometry["vertices"], moved) and np.array_equal(bs.base.lap_val, geometry.plan_with_vertices(plan, moved).lap_val)
        back = bs.solve_many(three(name), vertices=mesh["vertices"])
        assert len(contexts) == 2
    same(there, many_moved(mesh, plan, moved, three(name)))
    same(back, many_cold(name))
    assert not np.array_equal(rec(there[0])["kkt_errors"], rec(back[0])["kkt_errors"], equal_nan=True)      # (another surface, another run)


@pytest.mark.parametrize("name", NAMES)
def test_moved_warm_equals_the_single_session_per_problem(name):
    from dots_socp_amd.socp import BatchSession

    _, p1, p2 = sc.problems(name)
    moved = thm.moved_of(name)
    firsts = [dict(mu0=m[0], mu1=m[1], **run_options(name)) for m in (p1, swapped(p1))]
    thens = [dict(mu0=m[0], mu1=m[1], **run_options(name)) for m in (p2, swapped(p2))]
    with BatchSession(sc.CASES[name][0], sc.problems(name)[0], max_batch=2) as bs:
        bs.solve_many(firsts, outputs=())
        got = bs.solve_many(thens, warm=True, vertices=moved)
    same(got, [single_session(name, a, b, {}, moved=moved) for a, b in zip(firsts, thens)])


def test_a_context_made_after_a_move_is_built_on_the_moved_plan(contexts):
    """One problem, then three on moved vertices: the second slot's context is created on the moved plan and shares the refreshed factor."""
    from dots_socp_amd.socp import BatchSession

    name = "torus"
    moved = thm.moved_of(name)
    with BatchSession(sc.CASES[name][0], sc.problems(name)[0], max_batch=2) as bs:
        bs.solve_many([dict(three(name)[0], nit=sc.LIVE_STOP)], outputs=())
        plan = bs.base
        assert len(contexts) == 1
        got = bs.solve_many(three(name), vertices=moved)
        assert len(contexts) == 2
    same(got, many_moved(sc.problems(name)[0], plan, moved, three(name)))


def test_moved_on_a_factor_with_merged_bands_top_inverse_and_leaf_inverses(monkeypatch):
    """The 960-vertex torus of test_hip_move.py at T = 7: two members, 30 iterations, so that a refresh under sharing reaches the
    merged blocks, the top band's inverse and the leaves' local inverses."""
    from dots_socp_amd.socp import BatchSession

    monkeypatch.setenv("DOTS_FRONT_BANDS", thm.BIG_BANDS)      # (the session plans inside its first call: the cuts hold for the whole test,
    monkeypatch.setenv("DOTS_FRONT_TOPINV", "1")               # and explicit cuts leave the top band's form to this switch)
    n_time, mesh, p1, p2 = thm.case_problem(thm.BIG)
    moved = mc.displaced(mesh["vertices"])
    problems = [dict(mu0=m[0], mu1=m[1], tol=sc.TOL, nit=30) for m in (p1, p2)]
    with BatchSession(n_time, mesh, max_batch=2) as bs:
        bs.solve_many(problems, outputs=())
        plan = bs.base
        summary = bs.solvers[1].dev.front_summary
        assert summary["top_inverse"] and summary["leaf_inverse"] and bool(np.any(np.diff(summary["bands"]) > 1))
        got = bs.solve_many(problems, vertices=moved)
        back = bs.solve_many(problems, vertices=mesh["vertices"])
    from dots_socp_amd.socp import solver_socp_many

    same(got, many_moved(mesh, plan, moved, problems))
    same(back, solver_socp_many(n_time, mesh, problems, max_batch=2, plan=plan))


# ---- 4 one refresh, one hash ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", (0.0, 1e-2))
@pytest.mark.parametrize("case", NAMES + (thm.BIG,))
def test_one_refresh_serves_every_member(case, eps, monkeypatch):
    from dots_socp_amd.device import DeviceProblem, laplacian_solve_many, move_vertices_many

    n_time, mesh, p1, p2 = thm.case_problem(case)
    moved = mc.displaced(mesh["vertices"])
    with thm.bare(case, monkeypatch, eps=eps) as owner:
        old_plan = owner.plan
        with DeviceProblem(n_time, None, lap_solver="modal_pcg", plan=geometry.plan_with_densities(old_plan, *p2)) as sharer:
            sharer.set_params(eps=eps)
            sharer.share_frontal(owner)
            rng = np.random.default_rng(5)
            rhs = [rng.standard_normal(owner.shape("phi")) for _ in range(2)]
            before = laplacian_solve_many([owner, sharer], rhs)
            info = (owner.debug_counter(10), sharer.debug_counter(10), owner.device_bytes(), sharer.device_bytes())
            ms = move_vertices_many([owner, sharer], moved)
            assert len(ms) == 3 and ms[2] >= ms[1] > 0.0 and owner.move_ms == sharer.move_ms == ms
            assert (owner.debug_counter(10), sharer.debug_counter(10), owner.device_bytes(), sharer.device_bytes()) == info      # nothing allocated
            want_plan = geometry.plan_with_vertices(old_plan, moved)
            for dev, masses in ((owner, p1), (sharer, p2)):
                tables = dev.geometry_tables()
                for k, v in thm.tables_of_plan(want_plan).items():
                    assert np.array_equal(tables[k], v), k
                assert np.array_equal(dev.plan.lap_val, want_plan.lap_val) and np.array_equal(dev.plan.mu1, geometry.plan_with_densities(old_plan, *masses).mu1)
                dev.restart(*masses, mode="cold")
                with DeviceProblem(n_time, None, lap_solver="modal_pcg", plan=mc.twin_plan(old_plan, moved, *masses)) as new:
                    assert ths.params_record(dev) == {**ths.params_record(new), "eps": eps}
            got = laplacian_solve_many([sharer, owner], rhs[::-1])[::-1]
            with thm.bare(case, monkeypatch, eps=eps, plan=mc.twin_plan(old_plan, moved, *p1)) as new:
                want = [laplacian_solve_many([new], [r])[0] for r in rhs]
            for g, w, b in zip(got, want, before):
                assert np.array_equal(g, w) and not np.array_equal(g, b)
            if eps == 0.0:      # one hash for all: the moved plan shares with any member, the old plan with none
                for member in (owner, sharer):
                    with DeviceProblem(n_time, None, lap_solver="modal_pcg", plan=want_plan) as third:
                        third.share_frontal(member)
                        assert np.array_equal(laplacian_solve_many([third], rhs[:1])[0], want[0])
                    with DeviceProblem(n_time, None, lap_solver="modal_pcg", plan=old_plan) as stranger:
                        with pytest.raises(_lib.HipLibraryError, match="another mesh or vertex numbering") as err:
                            stranger.share_frontal(member)
                        assert err.value.status == _lib.ERR_ARGUMENT


def test_one_context_alone_is_the_single_move(monkeypatch):
    """n = 1, a context that holds its store alone: the tables, the parameters and the factor of dots_move_vertices, bit for bit."""
    from dots_socp_amd.device import laplacian_solve_many, move_vertices_many

    case = "torus"
    _, mesh, p1, _ = thm.case_problem(case)
    moved = mc.displaced(mesh["vertices"])
    out = []
    for many in (False, True):
        with thm.bare(case, monkeypatch) as dev:
            rhs = np.random.default_rng(5).standard_normal(dev.shape("phi"))
            ms = move_vertices_many([dev], moved) if many else dev.move_vertices(moved)
            assert len(ms) == 3
            tables = dev.geometry_tables()
            dev.restart(*p1, mode="cold")
            out.append((tables, ths.params_record(dev), laplacian_solve_many([dev], [rhs])[0], dev.debug_counter(9)))
    ths.same_tree(out[0][0], out[1][0])
    assert out[0][1] == out[1][1] and np.array_equal(out[0][2], out[1][2]) and out[0][3] == out[1][3]


# ---- 5 refusals, 6 mid-run, 7 the restart before a step: two members driven by hand ------------------------------------------------------------
def members(name, masses, **options):
    """Two solvers on one factor as ``solver_socp_many`` builds them"""
    n_time = sc.CASES[name][0]
    mesh = sc.problems(name)[0]
    base = geometry.build_plan(n_time, {**mesh, "mu0": masses[0][0], "mu1": masses[0][1]}, reorder="nd")
    out = []
    try:
        for m in masses:
            out.append(ths.AlmSolver(n_time, {**mesh, "mu0": m[0], "mu1": m[1]}, plan=geometry.plan_with_densities(base, *m), reorder="nd",
                                     front_owner=out[0].dev if out else None, **options))
    except Exception:
        for a in out:
            a.close()
        raise
    return out


def lockstep(solvers, steps=None):
    n = 0
    while not all(a.finished for a in solvers) and (steps is None or n < steps):
        ss._lockstep(solvers, len(solvers))
        n += 1
    return solvers


def move_raw_many(devs, positions):
    """dots_move_vertices_many itself, on positions in the DEVICE numbering: the status."""
    d = _lib.MoveDesc()
    positions = np.ascontiguousarray(positions, dtype=np.float64)
    d.vertices = positions.ctypes.data
    hs = (C.c_void_p * len(devs))(*[p._h.value for p in devs])
    return devs[0].lib.dots_move_vertices_many(hs, len(devs), C.byref(d))


def test_refusals_leave_the_batch_as_it_was():
    from dots_socp_amd.socp import solver_socp_many

    name = "plane"
    _, p1, p2 = sc.problems(name)
    opts = run_options(name)
    solvers = members(name, (p1, p2), **opts)
    try:
        a, b = lockstep(solvers, sc.LIVE_STOP)
        assert not a.finished and not b.finished
        good = np.array(a.dev.plan.vertices)
        tables = [s.dev.geometry_tables() for s in solvers]
        last = lambda: a.dev.lib.dots_last_error().decode()
        for devs in ([a.dev], [b.dev], [a.dev, a.dev], [a.dev, b.dev, a.dev]):
            assert move_raw_many(devs, good) == _lib.ERR_STATE and "not the set of holders of one factor store" in last()
        flat, nan = good.copy(), good.copy()
        t0 = a.dev.plan.triangles[0]
        flat[t0[1]] = flat[t0[0]]      # a triangle folded to zero area
        nan[7, 2] = np.nan
        for positions in (flat, nan):
            assert move_raw_many([a.dev, b.dev], positions) == _lib.ERR_ARGUMENT
        for s in solvers:
            assert thm.move_raw(s.dev, good) == _lib.ERR_STATE and "factor store is shared" in last()
        for s, t in zip(solvers, tables):
            ths.same_tree(s.dev.geometry_tables(), t)
        lockstep(solvers)
        got = [s.finalize() for s in solvers]
    finally:
        for s in solvers:
            s.close()
    same(got, solver_socp_many(sc.CASES[name][0], sc.problems(name)[0], [dict(mu0=m[0], mu1=m[1], **opts) for m in (p1, p2)], max_batch=2))


@pytest.mark.parametrize("name", ("torus", "icosphere1"))
def test_a_move_in_the_middle_of_a_batch_flushes_with_the_old_geometry(name):
    """Both members stop after the iteration that leaves a penalty division pending (session_checks.LIVE_STOP: z_mid deferred, the
    division not carried out), move together and restart warm: each equals the single context that did the same on its own.
    (On "plane" the update of iteration 38 leaves the penalty where it was: what is live there on a single context is the launch
    ahead, which a batch does not have, so nothing would be pending.)"""
    from dots_socp_amd.device import move_vertices_many

    n_time, opts = ths.options_of(name)
    _, p1, p2 = sc.problems(name)
    firsts, thens = (p1, swapped(p1)), (p2, swapped(p2))
    moved = thm.moved_of(name)
    live = dict(tol=1e-12, nit=4000)
    want = []
    for first, then in zip(firsts, thens):
        alm = ths.AlmSolver(n_time, {**sc.problems(name)[0], "mu0": first[0], "mu1": first[1]}, **live)
        try:
            ths.run(alm, sc.LIVE_STOP)
            alm.restart(*then, warm=True, vertices=moved, **opts)      # no finalize, no download
            want.append(ths.run(alm).finalize())
        finally:
            alm.close()
    solvers = members(name, firsts, **live)
    try:
        lockstep(solvers, sc.LIVE_STOP - 1)
        before = [s.r for s in solvers]
        lockstep(solvers, 1)
        for s, r in zip(solvers, before):
            assert s.counter_main == sc.LIVE_STOP - 1 and not s.finished and not s._last_quiet
            assert s.adjust_params.last_it == sc.LIVE_STOP - 1 and s.r != r      # a penalty update whose division is pending
        ms = move_vertices_many([s.dev for s in solvers], moved)
        assert len(ms) == 3
        for s, then in zip(solvers, thens):
            s._geometry_moved(np.array(moved))
            s.restart(*then, warm=True, batch_member=True, **opts)
        got = [s.finalize() for s in lockstep(solvers)]
    finally:
        for s in solvers:
            s.close()
    same(got, want)


def test_moved_members_step_only_after_all_have_restarted():
    from dots_socp_amd.device import move_vertices_many, step_many

    name = "icosphere1"
    _, p1, p2 = sc.problems(name)
    solvers = members(name, (p1, p2), **run_options(name))
    try:
        a, b = lockstep(solvers, 5)
        move_vertices_many([a.dev, b.dev], thm.moved_of(name))
        for restart in (lambda: None, lambda: a.dev.restart(*p2, mode="cold")):
            restart()
            for devs in ([a.dev, b.dev], [b.dev, a.dev]):
                with pytest.raises(_lib.HipLibraryError, match="dots_step_many: the vertices were moved .*needs a dots_restart") as err:
                    step_many(devs)
                assert err.value.status == _lib.ERR_STATE
        b.dev.restart(*p1, mode="cold")
        step_many([a.dev, b.dev])
        a.dev.sync()
        b.dev.sync()
    finally:
        for s in solvers:
            s.close()


# ---- 8 torch --------------------------------------------------------------------------------------------------------------------------------
def test_the_torch_function_on_a_batch_session():
    import torch

    from dots_socp_amd import torch_cost
    from dots_socp_amd.socp import BatchSession

    name = "torus"
    n_time, opts = ths.options_of(name)
    mesh, p1, p2 = sc.problems(name)
    moved = thm.moved_of(name)
    geom, _ = meshes.make_geometry(mesh["vertices"], mesh["triangles"], normalize=False)
    masses = (np.stack([p1[0], p2[0], p1[1]]), np.stack([p1[1], p2[1], p1[0]]))

    def call(positions, **kw):
        m0, m1 = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in masses)
        x = torch.tensor(positions, dtype=torch.float64, requires_grad=True)
        c = torch_cost.transport_costs(m0, m1, x, mesh["triangles"], n_time, **opts, **kw)
        (c * torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64)).sum().backward()
        return {"cost": c.detach().numpy(), "mu0": m0.grad.numpy(), "mu1": m1.grad.numpy(), "vertices": x.grad.numpy()}

    with BatchSession(n_time, geom, max_batch=2) as bs:
        got = call(mesh["vertices"], session=bs, warm=False)
        again = call(mesh["vertices"], session=bs, move=True)      # equal positions: nothing moves
        assert all(s.move_ms is None for s in bs.solvers)
        plan = bs.base
        got_moved = call(moved, session=bs, move=True, warm=False)
        assert all(s.move_ms is not None for s in bs.solvers) and np.array_equal(bs.geometry["vertices"], moved)
    want = call(mesh["vertices"], max_batch=2)
    ths.assert_same(got, want)
    ths.assert_same(again, want)
    ths.assert_same(got_moved, call(moved, max_batch=2, plan=geometry.plan_with_vertices(plan, moved)))
    assert not np.array_equal(got_moved["cost"], want["cost"])

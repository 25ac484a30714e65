"""GPU tests of moved vertices on a live context: dots_move_vertices, dots_geometry_copy, DeviceProblem.move_vertices,
AlmSolver.restart(vertices=), SolveSession.solve(vertices=) and transport_cost(move=True).  The contract is bit identity with a new
solver on the same plan: every comparison is np.array_equal with NaN positions equal.  The twin is a new AlmSolver (or DeviceProblem) on
``plan_with_densities(plan_with_vertices(session plan, moved), mu0, mu1)``: the same numbering and tree, assembled and factorised from
scratch.  Cases and the displacement: move_checks.py; the record of a run: test_hip_session.record."""
import ctypes as C

import numpy as np
import pytest

import move_checks as mc
import session_checks as sc
import test_hip_session as ths
from conftest import has_gpu
from dots_socp_amd import _lib, geometry, meshes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

NAMES = tuple(sc.CASES)
BIG = "torus40x24"      # 960 vertices at T = 7, band 0 one tree height: the leaves run as explicit local inverses (tables and factor tests only)
BIG_BANDS = "0,1,4,7"


def moved_of(name, a=mc.AMPLITUDE):
    return mc.displaced(sc.problems(name)[0]["vertices"], a)


def twin(name, plan, moved, masses, init_solution=None, finalize=None, **more):
    """The record of a new solver on the moved mesh in the numbering of ``plan``."""
    n_time, opts = ths.options_of(name, **more)
    geom = {**mc.moved_mesh(sc.problems(name)[0], moved), "mu0": masses[0], "mu1": masses[1]}
    alm = ths.AlmSolver(n_time, geom, plan=mc.twin_plan(plan, moved, *masses), batched=False, init_solution=init_solution, **opts)
    try:
        ths.run(alm)
        return ths.record(alm) if finalize is None else alm.finalize(**finalize)
    finally:
        alm.close()


_cold = {}


def twin_cold(name, plan):
    """The twin's cold solve of P2 on the moved mesh, computed once per case and left unchanged."""
    if name not in _cold:
        _cold[name] = twin(name, plan, moved_of(name), sc.problems(name)[2])[0]
    return _cold[name]


# ---- bare contexts with their own factor (tables and factor) --------------------------------------------------------------------------
def big_problem():
    v, t = meshes.torus(40, 24)
    geom, _ = meshes.make_geometry(v, t, normalize=False)
    v, t = geom["vertices"], geom["triangles"]
    far = int(np.argmax(np.sum((v - v[0]) ** 2, axis=1)))
    mu0, mu1 = sc._bumps(v, t, 0, far)
    _, mu1b = sc._bumps(v, t, 0, sc.neighbour_of(t, far))
    return geom, (mu0, mu1), (mu0.copy(), mu1b)


def case_problem(case):
    """``(n_time, mesh, P1, P2)``"""
    if case == BIG:
        return (7,) + big_problem()
    return (sc.CASES[case][0],) + sc.problems(case)


def bare(case, monkeypatch, eps=0.0, plan=None, masses=None):
    from dots_socp_amd.device import DeviceProblem

    n_time, mesh, p1, _ = case_problem(case)
    m0, m1 = p1 if masses is None else masses
    if plan is None and case == BIG:
        monkeypatch.setenv("DOTS_FRONT_BANDS", BIG_BANDS)
        plan = geometry.build_plan(n_time, {**mesh, "mu0": m0, "mu1": m1}, reorder="nd")
        monkeypatch.delenv("DOTS_FRONT_BANDS")
    dev = DeviceProblem(n_time, {**mesh, "mu0": m0, "mu1": m1}, lap_solver="modal_pcg", reorder="nd", plan=plan)
    try:
        dev.setup_frontal(eps=eps)
    except Exception:
        dev.close()
        raise
    return dev


def tables_of_plan(plan):
    return {"area_tri": plan.area_tri, "hat_grad": plan.hat_grad, "mass_vert": plan.mass_vert, "lap_val": plan.lap_val, **mc.derived_tables(plan)}


def move_raw(dev, positions, device_pointers=False):
    """dots_move_vertices itself, on positions in the DEVICE numbering: the status."""
    d = _lib.MoveDesc()
    if device_pointers:
        d.vertices, d.device_pointers = positions.data_ptr(), 1
    else:
        positions = np.ascontiguousarray(positions, dtype=np.float64)
        d.vertices = positions.ctypes.data
    return dev.lib.dots_move_vertices(dev._h, C.byref(d))


# ---- G1 tables ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NAMES + (BIG,))
def test_tables_after_a_move_are_the_moved_plans(case, monkeypatch):
    from dots_socp_amd.device import DeviceProblem

    n_time, mesh, _, p2 = case_problem(case)
    moved = mc.displaced(mesh["vertices"])
    with bare(case, monkeypatch) as dev:
        old_plan = dev.plan
        assert ths.same_tree(dev.geometry_tables(), tables_of_plan(old_plan)) is None      # the window itself, on a new context
        ms = dev.move_vertices(moved)
        assert len(ms) == 3 and all(x >= 0.0 for x in ms) and ms[2] >= ms[1]
        want_plan = geometry.plan_with_vertices(old_plan, moved)
        got = dev.geometry_tables()
        want = tables_of_plan(want_plan)
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
            assert not np.array_equal(got[k], tables_of_plan(old_plan)[k]), k
        assert dev.plan.dissection is old_plan.dissection and np.array_equal(dev.plan.lap_val, want_plan.lap_val)
        dev.restart(*p2, mode="cold")
        got_params = ths.params_record(dev)
        with DeviceProblem(n_time, None, lap_solver="modal_pcg", plan=mc.twin_plan(old_plan, moved, *p2)) as new:
            assert got_params == ths.params_record(new)


def test_the_cases_cover_merged_bands_top_inverse_and_leaf_inverses(monkeypatch):
    seen = {"merged": False, "top_inverse": False, "leaf_inverse": False}
    for case in NAMES + (BIG,):
        with bare(case, monkeypatch) as dev:
            s = dev.front_summary
            seen["merged"] |= bool(np.any(np.diff(s["bands"]) > 1))
            seen["top_inverse"] |= bool(s["top_inverse"])
            seen["leaf_inverse"] |= bool(s["leaf_inverse"])
    assert all(seen.values()), seen


# ---- G2 factor ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", (0.0, 1e-2))
@pytest.mark.parametrize("case", NAMES + (BIG,))
def test_the_refreshed_factor_solves_as_a_new_one(case, eps, monkeypatch):
    from dots_socp_amd.device import laplacian_solve_many

    n_time, mesh, p1, _ = case_problem(case)
    moved = mc.displaced(mesh["vertices"])
    with bare(case, monkeypatch, eps=eps) as dev:
        old_plan = dev.plan
        rhs = np.random.default_rng(5).standard_normal(dev.shape("phi"))
        before = laplacian_solve_many([dev], [rhs])[0]
        info = (dev.front_summary["launches_per_solve"], dev.debug_counter(10), dev.device_bytes())
        dev.move_vertices(moved)
        assert (dev.front_launches(), dev.debug_counter(10), dev.device_bytes()) == info      # nothing allocated, nothing rescheduled
        got = laplacian_solve_many([dev], [rhs])[0]
        with bare(case, monkeypatch, eps=eps, plan=mc.twin_plan(old_plan, moved, *p1)) as new:
            want = laplacian_solve_many([new], [rhs])[0]
            assert np.array_equal(got, want) and not np.array_equal(got, before)
            if eps == 0.0:      # lap_hash follows the move: the moved plan shares, the old plan is refused
                from dots_socp_amd.device import DeviceProblem

                with DeviceProblem(n_time, None, lap_solver="modal_pcg", plan=dev.plan) as sharer:
                    sharer.share_frontal(dev)
                    assert np.array_equal(laplacian_solve_many([sharer], [rhs])[0], want)
                with DeviceProblem(n_time, None, lap_solver="modal_pcg", plan=old_plan) as stranger:
                    with pytest.raises(_lib.HipLibraryError, match="another mesh or vertex numbering") as err:
                        stranger.share_frontal(dev)
                    assert err.value.status == _lib.ERR_ARGUMENT


# ---- G3 trajectories ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_cold_solve_after_a_move_equals_the_twin_from_zero(name):
    n_time, opts = ths.options_of(name)
    _, _, p2 = sc.problems(name)
    alm = ths.AlmSolver(n_time, sc.geometry(name, 1), **opts)
    try:
        ths.run(alm).finalize(download=False)
        plan = alm.dev.plan
        alm.restart(*p2, warm=False, vertices=moved_of(name))
        assert alm.move_ms is not None and np.array_equal(alm.geometry["vertices"], moved_of(name))
        got = ths.record(ths.run(alm))[0]
    finally:
        alm.close()
    ths.assert_same(got, twin_cold(name, plan))
    assert not np.array_equal(got["kkt_errors"], ths.fresh_p2(name)["kkt_errors"], equal_nan=True)      # (another surface, another run)


@pytest.mark.parametrize("name", NAMES)
def test_warm_solve_after_a_move_equals_the_twin_with_init_solution(name):
    n_time, opts = ths.options_of(name)
    _, _, p2 = sc.problems(name)
    alm = ths.AlmSolver(n_time, sc.geometry(name, 1), **opts)
    try:
        _, first = ths.record(ths.run(alm))
        plan = alm.dev.plan
        alm.restart(*p2, warm=True, vertices=moved_of(name))
        got = ths.record(ths.run(alm))[0]
    finally:
        alm.close()
    ths.assert_same(got, twin(name, plan, moved_of(name), p2, init_solution=ths.whole(first))[0])


# ---- G4 mid-run -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_a_move_in_the_middle_of_a_run_flushes_with_the_old_geometry(name):
    """A penalty division pending, a launch ahead, z_mid not yet rebuilt (test_hip_session.live_solver): the warm start is the solution
    ``finalize`` would have given at that point, on the OLD surface."""
    _, _, p2 = sc.problems(name)
    _, opts = ths.options_of(name)
    first_solver, live = ths.live_solver(name)
    try:
        first, _ = first_solver.finalize()
    finally:
        first_solver.close()
    assert live["update"] and live["read_back"] and (live["division"] or live["ahead"]), live
    alm, live2 = ths.live_solver(name)
    try:
        assert live2 == live
        plan = alm.dev.plan
        alm.restart(*p2, warm=True, vertices=moved_of(name), **opts)      # no finalize, no download
        got = ths.record(ths.run(alm))[0]
    finally:
        alm.close()
    ths.assert_same(got, twin(name, plan, moved_of(name), p2, init_solution=ths.whole(first))[0])


# ---- G5 there and back ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_there_and_back_is_the_solver_that_never_moved(name, monkeypatch):
    from dots_socp_amd.device import laplacian_solve_many

    n_time, opts = ths.options_of(name)
    mesh, _, p2 = sc.problems(name)
    with bare(name, monkeypatch) as dev:
        tables = dev.geometry_tables()
        rhs = np.random.default_rng(7).standard_normal(dev.shape("phi"))
        solved = laplacian_solve_many([dev], [rhs])[0]
        dev.move_vertices(moved_of(name))
        dev.move_vertices(mesh["vertices"])
        ths.same_tree(dev.geometry_tables(), tables)
        assert np.array_equal(laplacian_solve_many([dev], [rhs])[0], solved)
    alm = ths.AlmSolver(n_time, sc.geometry(name, 1), **opts)
    try:
        ths.run(alm, sc.LIVE_STOP)
        plan = alm.dev.plan
        alm.restart(*p2, warm=False, vertices=moved_of(name))
        alm.restart(*p2, warm=False, vertices=mesh["vertices"])
        ths.assert_same(ths.record(ths.run(alm))[0], ths.fresh_p2(name))
        # two different moves in a row: the twin of the second
        alm.restart(*p2, warm=False, vertices=moved_of(name, 0.5 * mc.AMPLITUDE))
        alm.restart(*p2, warm=False, vertices=moved_of(name))
        ths.assert_same(ths.record(ths.run(alm))[0], twin_cold(name, plan))
    finally:
        alm.close()


# ---- G6 refusals: argument and state checks only ----------------------------------------------------------------------------------------
def test_refused_positions_leave_the_context_as_it_was():
    import torch

    name = "plane"
    n_time, opts = ths.options_of(name)
    _, _, p2 = sc.problems(name)
    alm = ths.AlmSolver(n_time, sc.geometry(name, 1), **opts)
    try:
        ths.run(alm).finalize(download=False)
        dev = alm.dev
        tables, good = dev.geometry_tables(), np.array(dev.plan.vertices)
        flat = good.copy()
        t0 = dev.plan.triangles[0]
        flat[t0[1]] = flat[t0[0]]      # a collapsed triangle
        nan = good.copy()
        nan[7, 2] = np.nan
        for positions in (flat, nan):
            assert move_raw(dev, positions) == _lib.ERR_ARGUMENT
            on_device = torch.tensor(positions, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            assert move_raw(dev, on_device, device_pointers=True) == _lib.ERR_ARGUMENT
        with pytest.raises(ValueError, match="degenerate triangle"):      # (the driver refuses the same before the library is asked)
            alm.restart(*p2, warm=False, vertices=flat[alm._caller_order()])
        ths.same_tree(dev.geometry_tables(), tables)
        alm.restart(*p2, warm=False)
        ths.assert_same(ths.record(ths.run(alm))[0], ths.fresh_p2(name))
    finally:
        alm.close()


def test_contexts_that_cannot_move_say_why(monkeypatch):
    from dots_socp_amd.device import DeviceProblem

    name = "torus"
    n_time, _ = sc.CASES[name]
    geom = sc.geometry(name, 1)

    def refused(dev, text):
        positions = np.array(dev.plan.vertices)
        assert move_raw(dev, positions) == _lib.ERR_STATE
        assert text in dev.lib.dots_last_error().decode()

    with DeviceProblem(n_time, geom, lap_solver="modal_pcg", reorder="nd", time_slab=(0, 2)) as slab:
        refused(slab, "time slab")
    with DeviceProblem(n_time, geom, lap_solver="spacetime_pcg") as plain:
        refused(plain, "not modal")
    with DeviceProblem(n_time, geom, lap_solver="modal_pcg") as mg:
        mg.setup_multigrid(coarsest=32)
        refused(mg, "multigrid hierarchy")
    with bare(name, monkeypatch) as owner:
        with DeviceProblem(n_time, None, lap_solver="modal_pcg", plan=owner.plan) as sharer:
            sharer.share_frontal(owner)
            refused(sharer, "factor store is shared")
            refused(owner, "factor store is shared")
        owner.set_params(eps=1e-3)
        refused(owner, "the factor was built with")
        owner.set_params(eps=0.0)
        assert move_raw(owner, np.array(owner.plan.vertices)) == 0      # its sharer gone, the owner moves


def test_a_moved_context_steps_only_after_a_restart():
    name = "icosphere1"
    n_time, opts = ths.options_of(name)
    _, _, p2 = sc.problems(name)
    alm = ths.AlmSolver(n_time, sc.geometry(name, 1), **opts)
    try:
        ths.run(alm, sc.LIVE_STOP)
        alm.dev.move_vertices(moved_of(name))
        for call in (lambda: alm.dev.step(1, wait=False), lambda: alm.dev.kkt([0]), alm.dev.objective):
            with pytest.raises(_lib.HipLibraryError, match="needs a dots_restart") as err:
                call()
            assert err.value.status == _lib.ERR_STATE
        alm.dev.restart(*p2, mode="cold")
        alm.dev.step(1, wait=False)
        alm.dev.sync()
    finally:
        alm.close()


# ---- G7 a Jacobi modal PCG context without a factor ---------------------------------------------------------------------------------------
def test_a_jacobi_pcg_context_moves_its_tables_only():
    name, more = "torus", dict(lap_solver="modal_pcg", preconditioner="jacobi")
    n_time, opts = ths.options_of(name, **more)
    _, _, p2 = sc.problems(name)
    alm = ths.AlmSolver(n_time, sc.geometry(name, 1), **opts)
    try:
        ths.run(alm, sc.LIVE_STOP)
        plan = alm.dev.plan
        alm.restart(*p2, warm=False, vertices=moved_of(name))
        assert alm.move_ms[1] >= 0.0 and alm.dev.debug_counter(10) == 0      # no factor anywhere
        got = ths.record(ths.run(alm))[0]
    finally:
        alm.close()
    ths.assert_same(got, twin(name, plan, moved_of(name), p2, **more)[0])


# ---- G8 API ---------------------------------------------------------------------------------------------------------------------------
def test_session_solve_with_vertices_equals_the_twin(monkeypatch):
    from dots_socp_amd import frontal
    from dots_socp_amd.socp import SolveSession

    planned = []
    original = frontal.factorize
    monkeypatch.setattr(frontal, "factorize", lambda *a, **kw: (planned.append(1), original(*a, **kw))[1])
    name = "plane"
    n_time, opts = ths.options_of(name)
    mesh, p1, p2 = sc.problems(name)
    moved = moved_of(name)
    with SolveSession(n_time, mesh, **opts) as s:
        s.solve(*p1, outputs=(), nit=sc.LIVE_STOP)
        plan = s.alm.dev.plan
        got, hist = s.solve(*p2, warm=False, vertices=moved, nit=opts["nit"])
        stats = hist.solver_stats["session"]
        assert stats["moved"] is True and len(stats["move_ms"]) == 3 and stats["restart_ms"] > 0.0 and stats["index"] == 1
        assert np.array_equal(s.geometry["vertices"], moved) and np.array_equal(s.geometry["area_triangles"], mc.moved_mesh(mesh, moved)["area_triangles"])
        _, hist2 = s.solve(*p2, warm=False, outputs=())      # no vertices: the session stays where it is
        assert hist2.solver_stats["session"]["moved"] is False and hist2.solver_stats["session"]["move_ms"] is None
        assert planned == [1]      # the symbolic analysis ran for the first solve only: a move plans nothing
    want, hist_w = twin(name, plan, moved, p2, finalize={})
    ths.same_tree(got, want)
    assert np.array_equal(hist.kkt_errors, hist_w.kkt_errors, equal_nan=True) and np.array_equal(hist2.kkt_errors, hist_w.kkt_errors, equal_nan=True)


@pytest.mark.parametrize("name", ("torus",))
def test_the_torch_function_moves_its_session(name):
    import torch

    from dots_socp_amd import sensitivity, torch_cost
    from dots_socp_amd.socp import SolveSession

    n_time, opts = ths.options_of(name)
    mesh, p1, p2 = sc.problems(name)
    moved = moved_of(name)
    geom, _ = meshes.make_geometry(mesh["vertices"], mesh["triangles"], normalize=False)

    def call(session, masses, positions, **kw):
        m0, m1 = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in masses)
        x = torch.tensor(positions, dtype=torch.float64, requires_grad=True)
        c = torch_cost.transport_cost(m0, m1, x, mesh["triangles"], n_time, session=session, **opts, **kw)
        c.backward()
        return {"cost": np.array(float(c.detach())), "mu0": m0.grad.numpy(), "mu1": m1.grad.numpy(), "vertices": x.grad.numpy()}

    with SolveSession(n_time, geom) as s:
        call(s, p1, mesh["vertices"], move=True)      # equal positions: nothing moves
        assert s.alm.move_ms is None
        plan = s.alm.dev.plan
        got = call(s, p2, moved, move=True, warm=False)
        assert s.alm.move_ms is not None and np.array_equal(s.geometry["vertices"], moved)
    solution, hist = twin(name, plan, moved, p2, finalize={"outputs": (), "sensitivity": True})
    g0, g1, gx = sensitivity.cost_gradients(solution["sensitivity"], moved, np.asarray(mesh["triangles"], dtype=np.int64))
    ths.assert_same(got, {"cost": np.array(float(hist.history["Transportation cost"][-1])), "mu0": g0, "mu1": g1, "vertices": gx})


# ---- G9 read-outs after a move ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("request_", ({"read_out": {"dot_units": True, "centred": True}}, {"sensitivity": True, "outputs": ("phi", "mu")},
                                      {"flow_map": {"starts": "vertices", "push": True}, "outputs": ()}), ids=("read_out", "sensitivity", "flow_map"))
def test_derived_outputs_after_a_move(request_):
    from dots_socp_amd.socp import SolveSession

    name = "torus"
    n_time, opts = ths.options_of(name)
    mesh, p1, p2 = sc.problems(name)
    moved = moved_of(name)
    with SolveSession(n_time, mesh, **opts) as s:
        s.solve(*p1, outputs=(), nit=sc.LIVE_STOP)
        plan = s.alm.dev.plan
        got, hist = s.solve(*p2, warm=False, vertices=moved, nit=opts["nit"], **request_)
    want, hist_w = twin(name, plan, moved, p2, finalize=request_)
    ths.same_tree(got, want)
    assert np.array_equal(hist.kkt_errors, hist_w.kkt_errors, equal_nan=True)
    if "read_out" in request_:
        ths.same_tree(hist.solver_stats["readout"], hist_w.solver_stats["readout"])


# ---- G10 device positions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_device_positions_give_what_the_host_array_gives(name):
    import torch

    n_time, opts = ths.options_of(name)
    _, _, p2 = sc.problems(name)
    alm = ths.AlmSolver(n_time, sc.geometry(name, 1), **opts)
    try:
        ths.run(alm, sc.LIVE_STOP)
        plan = alm.dev.plan
        alm.restart(*p2, warm=False, vertices=torch.tensor(moved_of(name), dtype=torch.float64, device="cuda"))
        assert np.array_equal(alm.geometry["vertices"], moved_of(name)) and np.array_equal(alm.dev.plan.vertices, moved_of(name)[plan.perm_vert])
        got = ths.record(ths.run(alm))[0]
    finally:
        alm.close()
    ths.assert_same(got, twin_cold(name, plan))

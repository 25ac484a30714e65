"""GPU parity of the whole solver against the reference's recorded runs (tests/golden/run_*.npz):
same stopping iteration, same lazy-KKT pattern, KKT values, cost and solution arrays."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_oracle

pytestmark = pytest.mark.gpu

O = load_oracle()
RUNS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN_DIR, "run_*.npz")))
SMALL = [r for r in RUNS if "refplane20" not in r]
HEADLINE = [r for r in RUNS if "refplane20" in r]
REL_TOL = 1e-6     # BASELINE.json north_star: cost and KKT residuals within 1e-6 relative of the reference


def golden(name):
    return np.load(os.path.join(GOLDEN_DIR, name))


def geom_of(g):
    return dict(vertices=g["vertices"], triangles=g["triangles"], mu0=g["mu0"], mu1=g["mu1"])


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def run_hip(g, **extra):
    from dots_socp_amd.socp import solver_socp

    geom = dict(vertices=g["vertices"], triangles=g["triangles"], mu0=g["mu0"], mu1=g["mu1"])
    kw = {}
    for k in g.files:
        if k.startswith("kw_"):
            val = g[k]
            kw[k[3:]] = val.tolist() if val.ndim else val.item()
    kw.update(extra)
    return solver_socp(int(g["n_time"]), geom, **kw)


def mass_of(g):
    area = O.triangle_quantities(g["vertices"], g["triangles"])[0]
    return O.corner_maps(g["vertices"].shape[0], g["triangles"], area)[1] / 3.0


def remove_gauge(phi, mass_v):
    w = np.broadcast_to(mass_v[None, :], phi.shape)
    return phi - np.sum(phi * w) / np.sum(w)


def compare(g, sol, hist, rtol):
    assert int(hist.kkt_iteration[-1]) == int(g["last_iteration"])
    want, got = g["hist_kkt_errors"], hist.kkt_errors
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "lazy KKT schedule differs from the reference"
    m = ~np.isnan(want)
    assert np.allclose(got[m], want[m], rtol=rtol, atol=1e-13)
    for key in ("Transportation cost", "Objective value"):
        w = g["hist_" + key.replace(" ", "_")]
        assert np.allclose(hist.history[key], w, rtol=rtol, atol=0, equal_nan=True), key
    eps = float(g["kw_eps"]) if "kw_eps" in g.files else 0.0
    for k in g.files:
        if not k.startswith("sol_"):
            continue
        a, b = sol[k[4:]], g[k]
        if k == "sol_phi" and eps == 0.0:
            a, b = remove_gauge(a, mass_of(g)), remove_gauge(b, mass_of(g))
        assert rel(a, b) < 50 * rtol, k


@pytest.mark.parametrize("fname", SMALL)
@pytest.mark.parametrize("lap_solver", ["modal_direct", "modal_pcg+mg", "modal_pcg", "spacetime_pcg"])
def test_runs_match_reference(fname, lap_solver):
    g = golden(fname)
    if lap_solver == "modal_direct":
        sol, hist = run_hip(g, lap_solver="modal_direct")
    elif lap_solver.endswith("+mg"):   # tiny meshes: force a multi-level hierarchy
        sol, hist = run_hip(g, lap_solver="modal_pcg", preconditioner="multigrid", mg_coarsest=6, cg_tol=1e-11)
    else:
        sol, hist = run_hip(g, lap_solver=lap_solver, preconditioner="jacobi", cg_tol=1e-11)
    assert hist.solver_stats["cg_not_converged"] == 0
    compare(g, sol, hist, REL_TOL)
    if "ckpt_iteration" in g.files:
        assert [c["iteration"] for c in sol["checkpoints"]] == g["ckpt_iteration"].tolist()
        assert rel(np.stack([c["mu"] for c in sol["checkpoints"]]), g["ckpt_mu"]) < 1e-5


@pytest.mark.parametrize("fname", ["run_ico2_T15_cong_tol1e-3.npz", "run_refplane20_T31_tol1e-3.npz", "run_torus_T7_tol1e-4.npz"])
def test_runs_match_reference_with_unmerged_tree_heights(fname, monkeypatch):
    """One launch per tree height (DOTS_FRONT_BANDS=off) puts the leaves of these small meshes into their own band: the leaves are then
    stored as explicit local inverses (kernels_front.hip: k_front_leaf_fwd / _bwd) -- the runs are the reference's all the same."""
    monkeypatch.setenv("DOTS_FRONT_BANDS", "off")
    g = golden(fname)
    sol, hist = run_hip(g, lap_solver="modal_direct")
    assert hist.solver_stats["cg_not_converged"] == 0
    compare(g, sol, hist, REL_TOL)


@pytest.mark.parametrize("fname", HEADLINE)
def test_headline_runs(fname):
    """plane n=20, T=31, tol=1e-3: iteration index 361 / cost 4.00756e-2
    (113 / 4.15684e-1 with congestion 0.1), reproduced on the GPU with the default solver settings."""
    g = golden(fname)
    sol, hist = run_hip(g)
    compare(g, sol, hist, REL_TOL)
    cost = hist.history["Transportation cost"][-1] / float(g["scale_factor"]) ** 2
    want = 4.156843973748015e-01 if "cong" in fname else 4.007560699483875e-02
    assert abs(cost - want) < REL_TOL * want


def test_decorators_and_argument_errors():
    from dots_socp_amd.socp import solver, solver_raw

    g = golden("run_refplane4_T8_tol1e-3.npz")
    geom = dict(vertices=g["vertices"], triangles=g["triangles"], mu0=g["mu0"], mu1=g["mu1"])
    raw, hist = solver_raw(8, geom, nit=30, tol=1e-3)
    cen, _ = solver(8, geom, nit=30, tol=1e-3)
    assert raw["mu"].shape == (8, geom["vertices"].shape[0]) and cen["mu"].shape == (9, geom["vertices"].shape[0])
    assert np.allclose(cen["mu"][0], g["mu0"]) and np.allclose(cen["mu"][-1], g["mu1"])
    assert np.allclose(cen["mu"][1:-1], 0.5 * (raw["mu"][:-1] + raw["mu"][1:]))
    # masses: every time slice of the staggered solution carries total mass ~ 1 once converged enough
    assert "Transportation cost" in hist.history
    for bad in ([], [2.0], "x", [1e-9]):
        with pytest.raises(ValueError):
            solver_raw(8, geom, nit=1, tol=1e-3, tol_checkpoints=bad)


@pytest.mark.parametrize("fname", ["f1_ico2_T15_ckpt.npz", "f1_torus_T7_cong.npz"])
def test_solver_and_solver_raw_match_the_reference_decorators(fname):
    """outputs of the reference's ``solver_raw`` / ``solver`` (socp/solver_decorator.py:10-72,
    utils/type.py:48-65: masses, fluxes, time-centred grid, converted checkpoints) recorded by make_golden.py f1."""
    from dots_socp_amd.socp import solver, solver_raw

    g = golden(fname)
    geom = dict(vertices=g["vertices"], triangles=g["triangles"], mu0=g["mu0"], mu1=g["mu1"])
    kw = {k[3:]: (g[k].tolist() if g[k].ndim else g[k].item()) for k in g.files if k.startswith("kw_")}
    for tag, fn in (("raw", solver_raw), ("center", solver)):
        kw_run = {k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()}
        sol, hist = fn(int(g["n_time"]), dict(geom), **kw_run)
        assert int(hist.kkt_iteration[-1]) == int(g[f"{tag}_last_iteration"])
        assert sol["mu"].shape == g[f"{tag}_mu"].shape and sol["E"].shape == g[f"{tag}_E"].shape
        assert rel(sol["mu"], g[f"{tag}_mu"]) < 1e-5 and rel(sol["E"], g[f"{tag}_E"]) < 1e-5
        if f"{tag}_ckpt_mu" in g.files:
            assert [c["iteration"] for c in sol["checkpoints"]] == g[f"{tag}_ckpt_iteration"].tolist()
            assert rel(np.stack([c["mu"] for c in sol["checkpoints"]]), g[f"{tag}_ckpt_mu"]) < 1e-5
            assert rel(np.stack([c["E"] for c in sol["checkpoints"]]), g[f"{tag}_ckpt_E"]) < 1e-5
        else:
            assert not sol.get("checkpoints")


def test_warm_start_is_a_fixed_point():
    """Restarting from a converged solution (init_solution, solver_socp.py:239-250) stops at once."""
    from dots_socp_amd.socp import solver_socp

    g = golden("run_refplane4_T8_tol1e-3.npz")
    geom = dict(vertices=g["vertices"], triangles=g["triangles"], mu0=g["mu0"], mu1=g["mu1"])
    sol, hist = solver_socp(8, geom, nit=3000, tol=1e-3, is_z_scaling=False)
    n1 = int(hist.kkt_iteration[-1])
    init = {k: v for k, v in sol.items() if k != "checkpoints"}
    sol2, hist2 = solver_socp(8, geom, nit=3000, tol=1e-3, is_z_scaling=False, init_solution=init)
    assert int(hist2.kkt_iteration[-1]) < max(5, n1 // 10)
    assert abs(hist2.history["Transportation cost"][-1] - hist.history["Transportation cost"][-1]) < 1e-3


def test_plane_against_the_exact_transport():
    """Ground truth independent of the reference (interface.py:386-480, data/settings/plane.py):
    two equal Gaussians on the plane -> a translation, dynamic cost 0.04, displacement interpolation in between."""
    from dots_socp_amd import evaluate, meshes
    from dots_socp_amd.socp import solver

    T = 31
    geom, scale = meshes.example("plane", n=40)
    sol, hist = solver(T, geom, tol=1e-4, nit=5000)
    cost = hist.history["Transportation cost"][-1] / scale ** 2
    assert abs(cost - 0.04) < 1e-4
    assert sol["mu"].shape == (T + 1, geom["vertices"].shape[0])      # time-centred grid: the T + 1 nodes
    tt = np.linspace(0.0, 1.0, T + 1)
    exact = evaluate.plane_exact_transportation(tt, geom["vertices"] / scale, geom["area_vertices"])
    err = evaluate.compare_with_exact_transportation(sol["mu"], exact, geom)
    assert err["l1"] < 2e-2 and err["l2"] < 1e-2 and err["linf"] < 5e-2      # the reference's norms (time step inside)
    assert evaluate.check_mass_conservation(sol["mu"]) < 1e-4
    assert evaluate.check_negative_mass(sol["mu"])[0] < 1e-5


@pytest.mark.parametrize("case", ["one_triangle_T1", "two_triangles_T2", "tetrahedron_T3"])
def test_smallest_problems_match_the_oracle(case):
    """Edge sizes: a single triangle with one time interval, a two-triangle strip, a closed tetrahedron."""
    from dots_socp_amd.socp import solver_socp

    if case == "one_triangle_T1":
        v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.2, 0.9, 0.0]])
        t, T = np.array([[0, 1, 2]]), 1
    elif case == "two_triangles_T2":
        v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.1, 0.8, 0.0], [1.1, 0.9, 0.3]])
        t, T = np.array([[0, 1, 2], [1, 3, 2]]), 2
    else:
        v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.9, 0.0], [0.5, 0.3, 0.8]])
        t, T = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]]), 3
    n = v.shape[0]
    mu0 = np.arange(1.0, n + 1.0)
    mu1 = mu0[::-1].copy()
    geom = dict(vertices=v, triangles=t, mu0=mu0 / mu0.sum(), mu1=mu1 / mu1.sum())
    kw = dict(nit=40, tol=1e-9, check_kkt_step_by_step=True)
    sol, hist = solver_socp(T, geom, **kw)
    ref_sol, ref_hist = O.solver_socp(T, geom, **kw)
    assert hist.kkt_errors.shape == ref_hist.kkt_errors.shape
    assert np.allclose(hist.kkt_errors, ref_hist.kkt_errors, rtol=1e-6, atol=1e-12)
    assert np.allclose(hist.history["Transportation cost"], ref_hist.history["Transportation cost"], rtol=1e-6, atol=1e-14)
    for k in ("mu", "E", "A", "B"):
        assert rel(sol[k], ref_sol[k]) < 1e-6, k


@pytest.mark.parametrize("fname", ["run_ico2_T15_cong_tol1e-3.npz", "run_torus_T7_tol1e-4.npz"])
def test_right_hand_side_ahead_changes_nothing(fname, monkeypatch):
    """The solver starts the next iteration's right-hand side behind the KKT kernels of a read-back iteration that changes nothing
    (DOTS_STEP_RHS_AHEAD; solver_socp.py: iterate): whole runs with it forced on and off are the same bit for bit — iterates,
    recorded KKT values, stopping iteration — whatever happens in between (penalty updates, z rescalings, the stop)."""
    g = golden(fname)
    out = []
    for mode in ("0", "2"):
        monkeypatch.setenv("DOTS_RHS_AHEAD", mode)
        out.append(run_hip(g, lap_solver="modal_direct"))
    (sol0, hist0), (sol1, hist1) = out
    assert int(hist0.kkt_iteration[-1]) == int(hist1.kkt_iteration[-1]) == int(g["last_iteration"])
    assert np.array_equal(hist0.kkt_errors, hist1.kkt_errors, equal_nan=True)
    for k in ("mu", "E", "A", "B", "phi", "z_fst", "z_mid", "z_end", "beta_fst", "beta_mid", "beta_end", "lambda_c"):
        assert np.array_equal(sol0[k], sol1[k]), k


def test_step_timers_cover_all_iterations():
    """RunningHistory.steps_time (the reference's per-step timers, admm_tools.py:244-251, printed as "Time of steps" :505-540 and
    tabulated by replication/log2table.py:99-106) comes from SAMPLED iterations, scaled to all iterations of their kind: its sum
    must be the device time of the whole loop, not of the samples.  (a) against the same run with EVERY iteration timed
    (DOTS_TIME_EVERY=1), (b) against the wall clock of a loop long enough to be device-bound."""
    from dots_socp_amd import meshes
    from dots_socp_amd.socp import solver_socp
    from dots_socp_amd.socp.solver_socp import AlmSolver

    g = golden("run_refplane20_T31_tol1e-3.npz")
    kw = {k[3:]: (g[k].tolist() if g[k].ndim else g[k].item()) for k in g.files if k.startswith("kw_")}
    sums = {}
    for every in ("32", "1"):
        os.environ["DOTS_TIME_EVERY"] = every
        try:
            _, hist = solver_socp(int(g["n_time"]), geom_of(g), **kw)
        finally:
            del os.environ["DOTS_TIME_EVERY"]
        assert int(hist.kkt_iteration[-1]) == int(g["last_iteration"])
        assert set(hist.steps_time) == {"Step 1-1 (Laplacian)", "Step 1-2 (SOC-Projection)", "Step 2+3 (Q & Lambda, Multiplier)"}
        sums[every] = sum(hist.steps_time.values())
        assert (hist.steps_time_note is None) == (every == "1")
        assert sums[every] < hist.running_time             # (an estimate of the device time of the steps; the run is device-bound)
    assert abs(sums["32"] - sums["1"]) < 0.15 * sums["1"], sums
    # (b) sphere10k-sized iterations take ~0.2 ms on the device against ~30 us of host work: the loop is device-bound
    geom, _ = meshes.example("sphere", level=5)
    alm = AlmSolver(31, geom, nit=400, tol=1e-30, time_limit=1e9)
    for _ in range(40):
        alm.iterate()
    alm.dev.sync()
    alm._collect_step_times(wait=True)
    t_before = sum(alm.run_history.steps_time.values())
    import time

    t0 = time.perf_counter()
    for _ in range(300):
        alm.iterate()
    alm.dev.sync()
    wall = time.perf_counter() - t0
    alm._collect_step_times(wait=True)
    steps = sum(alm.run_history.steps_time.values()) - t_before
    alm.close()
    # the KKT kernels, the penalty divisions and the host's decisions on read-back iterations are not under a step timer (as in the reference)
    assert 0.70 * wall < steps < 1.02 * wall, (steps, wall)


def test_factor_that_does_not_fit_falls_back_to_the_multigrid_pcg(monkeypatch, caplog):
    """Memory-regime policy: when the factor, its workspace and the carried sums exceed the device memory that is
    available (here: DOTS_MEM_BUDGET = 1 MB), dots_front_setup says so with DOTS_ERR_MEMORY -- nothing allocated, the context stays
    usable -- and lap_solver="modal_direct" runs the batched multigrid-PCG instead, with the reason logged and reported: the run
    is the reference's run all the same (same stopping iteration, KKT / cost within 1e-6)."""
    import logging

    from dots_socp_amd import _lib
    from dots_socp_amd.device import DeviceProblem
    from dots_socp_amd.socp import solver_socp

    g = golden("run_ico2_T15_cong_tol1e-3.npz")
    kw = {k[3:]: (g[k].tolist() if g[k].ndim else g[k].item()) for k in g.files if k.startswith("kw_")}
    monkeypatch.setenv("DOTS_MEM_BUDGET", "1")
    dev = DeviceProblem(int(g["n_time"]), geom_of(g), lap_solver="modal_pcg")
    with pytest.raises(_lib.HipLibraryError, match="does not fit") as err:
        dev.setup_frontal()
    assert err.value.status == _lib.ERR_MEMORY
    dev.set_params(cg_tol=1e-10)
    dev.step(1)                                            # the PCG of the same context still works
    assert np.isfinite(dev.kkt([0])[0][0])
    dev.close()
    with caplog.at_level(logging.WARNING, logger="dots_socp_amd"):
        sol, hist = solver_socp(int(g["n_time"]), geom_of(g), **kw)
    assert any("does not fit" in r.getMessage() for r in caplog.records)
    assert "does not fit" in hist.solver_stats["lap_solver_fallback"] and hist.solver_stats["cg_iterations"] > 0
    assert int(hist.kkt_iteration[-1]) == int(g["last_iteration"])
    want, got = g["hist_kkt_errors"], hist.kkt_errors
    m = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.allclose(got[m], want[m], rtol=1e-6, atol=1e-13)
    monkeypatch.setenv("DOTS_MEM_BUDGET", "100000")
    _, hist2 = solver_socp(int(g["n_time"]), geom_of(g), **kw)
    assert "lap_solver_fallback" not in hist2.solver_stats and hist2.solver_stats["cg_iterations"] == 0


@pytest.mark.parametrize("fname", ["run_ico2_T15_cong_tol1e-3.npz", "run_refplane20_T31_tol1e-3.npz"])
def test_penalty_decision_ahead_of_the_host(fname, monkeypatch):
    """dots_penalty_ahead: on penalty-update iterations the library takes the reference's decision (solver_socp.py:806-823,
    admm_tools.py:54-95) itself as soon as the residuals arrive and starts the next iteration's first launch with it; the driver's
    own decision confirms it.  Every anticipation is confirmed (the two decisions are the same arithmetic), and the run is the
    run without any launch ahead, bit for bit."""
    from dots_socp_amd.socp.solver_socp import AlmSolver

    g = golden(fname)
    kw = {k[3:]: (g[k].tolist() if g[k].ndim else g[k].item()) for k in g.files if k.startswith("kw_")}
    runs = {}
    for ahead in ("0", "1"):
        monkeypatch.setenv("DOTS_RHS_AHEAD", ahead)
        alm = AlmSolver(int(g["n_time"]), geom_of(g), **kw)
        for _ in range(kw["nit"]):
            if alm.iterate():
                break
        started, confirmed = alm.dev.debug_counter(2), alm.dev.debug_counter(3)
        sol, hist = alm.finalize()
        alm.close()
        runs[ahead] = (sol, hist.kkt_errors.copy(), hist.kkt_iteration.copy(), started, confirmed)
    if os.environ.get("DOTS_LAZY_DIV", "1") != "0":      # the decision ahead needs the division left pending (A/B switch)
        assert runs["0"][3] == 0 and runs["1"][3] >= 5 and runs["1"][4] == runs["1"][3]
    else:
        assert runs["0"][3] == 0 and runs["1"][3] == 0
    assert int(runs["1"][2][-1]) == int(g["last_iteration"])
    assert np.array_equal(runs["0"][1], runs["1"][1], equal_nan=True) and np.array_equal(runs["0"][2], runs["1"][2])
    for k in runs["0"][0]:
        if k != "checkpoints":
            assert np.array_equal(runs["0"][0][k], runs["1"][0][k]), k


def test_mailbox_fallback_never_returns_stale_sums():
    """when the mailbox's sequence number does not arrive (here: every third hand-over is published with a wrong
    number, and the spin is cut short), the sums are taken from the device scalars after a stream synchronisation -- the run is
    the same run, decision for decision."""
    from dots_socp_amd.socp.solver_socp import AlmSolver

    g = golden("run_ico2_T15_cong_tol1e-3.npz")
    kw = {k[3:]: (g[k].tolist() if g[k].ndim else g[k].item()) for k in g.files if k.startswith("kw_")}
    os.environ.update(DOTS_MAIL_TEST_DROP="3", DOTS_MAIL_SPINS="2000")
    try:
        alm = AlmSolver(int(g["n_time"]), geom_of(g), **kw)
    finally:
        del os.environ["DOTS_MAIL_TEST_DROP"], os.environ["DOTS_MAIL_SPINS"]
    for _ in range(kw["nit"]):
        if alm.iterate():
            break
    sol, hist = alm.finalize()
    fallbacks, handovers = alm.dev.debug_counter(0), alm.dev.debug_counter(1)
    alm.close()
    assert handovers >= 6 and fallbacks == handovers // 3
    want = g["hist_kkt_errors"]
    assert int(hist.kkt_iteration[-1]) == int(g["last_iteration"])
    assert np.array_equal(np.isnan(hist.kkt_errors), np.isnan(want))
    m = ~np.isnan(want)
    assert np.allclose(hist.kkt_errors[m], want[m], rtol=1e-6, atol=1e-13)
    assert np.max(np.abs(sol["mu"] - g["sol_mu"])) < 1e-6 * np.max(np.abs(g["sol_mu"]))


def test_example_from_an_off_file_on_the_device(tmp_path):
    """SURVEY 8(f3) end to end on the GPU: a mesh file (OFF) -> ``examples.load_example("knots_5", path)``
    (data/load_example.py:100-151, data/util.py:73-144, settings/knots_5.py) -> ``solver`` on the device, against the CPU oracle
    on the same geometry: same stopping iteration, same lazy-KKT pattern, KKT / cost within 1e-6; and the densities against the
    reference's own ``get_mu`` output where it was recorded (settings_get_mu.npz)."""
    from dots_socp_amd import examples, meshes
    from dots_socp_amd.socp import solver, solver_socp

    v, t = meshes.torus_knot_tube(nu=216, nv=14)             # 3 024 vertices: the recipe names vertices up to 2 786
    path = tmp_path / "knots_5.off"
    meshes.write_off(path, v, t)
    geom, scale = examples.load_example("knots_5", str(path))
    assert geom["vertices"].shape == (3024, 3) and abs(geom["mu0"].sum() - 1) < 1e-14 and abs(geom["mu1"].sum() - 1) < 1e-14
    v2, t2, _ = meshes.read_off(str(path))
    assert np.array_equal(t2, t) and np.allclose(v2, v, rtol=0, atol=1e-15)
    kw = dict(nit=2000, tol=1e-2)
    sol, hist = solver_socp(11, geom, **kw)
    ref_sol, ref_hist = O.solver_socp(11, geom, **kw)
    assert int(hist.kkt_iteration[-1]) == int(ref_hist.kkt_iteration[-1]) and 50 < int(hist.kkt_iteration[-1]) < 1999
    assert np.array_equal(np.isnan(hist.kkt_errors), np.isnan(ref_hist.kkt_errors))
    m = ~np.isnan(ref_hist.kkt_errors)
    assert np.allclose(hist.kkt_errors[m], ref_hist.kkt_errors[m], rtol=1e-6, atol=1e-13)
    assert np.allclose(hist.history["Transportation cost"], ref_hist.history["Transportation cost"], rtol=1e-6, equal_nan=True)
    assert np.max(np.abs(sol["mu"] - ref_sol["mu"])) < 1e-6 * np.max(np.abs(ref_sol["mu"]))
    # the decorated solver the interface calls (centred time grid, masses): the cost the paper tabulates is de-scaled by 1 / scale^2
    dot, dot_hist = solver(11, geom, **kw)
    assert dot["mu"].shape == (12, 3024) and np.allclose(dot["mu"][0], geom["mu0"]) and np.allclose(dot["mu"][-1], geom["mu1"])
    cost = dot_hist.history["Transportation cost"][-1] / scale ** 2
    assert cost == pytest.approx(ref_hist.history["Transportation cost"][-1] / scale ** 2, rel=1e-6)
    # get_mu itself against the reference's recorded output (the fixture's synthetic mesh)
    gm = golden("settings_get_mu.npz")
    m0, m1 = examples.get_mu("knots_5", gm["area_vertices"], gm["vertices"])
    assert np.max(np.abs(m0 - gm["knots_5_mu0"])) <= 1e-13 * np.max(np.abs(gm["knots_5_mu0"]))
    assert np.max(np.abs(m1 - gm["knots_5_mu1"])) <= 1e-13 * np.max(np.abs(gm["knots_5_mu1"]))


def test_bench_plain_run_dumps_what_the_solver_hands_out(tmp_path):
    """A plain ``bench.py`` run in a process of its own prints the headline over exactly the K timed steps and nothing of --full;
    its --dump-outputs hold the state of the last timed step as the solver hands it to a caller: the same problem solved for
    W + K iterations."""
    import json
    import subprocess
    import sys

    from conftest import ROOT
    from dots_socp_amd import meshes
    from dots_socp_amd.device import STATE_NAMES
    from dots_socp_amd.socp import solver_socp

    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "7", "--warmup", "3", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "ALM iterations/s" and line["steps"] == 7 and line["warmup"] == 3 and line["dtype"] == "f64"
    assert line["ms_per_step"] == pytest.approx(1e3 / line["value"])
    assert not {"steady_state", "roofline", "time_to_tol", "configs", "solver_alternatives", "cpu_baseline"} & set(line)
    geom, _ = meshes.example("knot")
    sol, _ = solver_socp(31, geom, nit=10, tol=1e-30)
    assert not (out / "z_mid.npy").exists()
    for name in STATE_NAMES:
        if name != "z_mid":
            got = np.load(out / f"{name}.npy")
            assert got.dtype == np.float64 and got.shape == sol[name].shape, name
            assert rel(got, sol[name]) < 1e-9, name

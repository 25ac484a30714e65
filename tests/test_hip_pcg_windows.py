"""GPU: the windowed modal PCG (dots_pcg_windows) -- long horizons without a factor.  Above 256 time nodes the T + 1 modal problems
are solved in windows of 256 modes, each through the PCG kernels at pitch 256, between the windowed time transforms
(k_time_modes_windows in kernels_modes.hip: time space at the full pitch, mode space in compact windows).

Iterates: phi after cg_max_iter = 8 and 16 against the fp64 host PCG of pcg_checks.py, whose single loop over all T + 1 columns is the
reference of every window (per-column scalars; a frozen column changes nothing).  The random warm start catches a wrong Q^T phi, the
unequal masses of pcg_checks.geometry_of a wrong column-0 sum (the mean removal of the singular mode at eps = 0), the torus the
k_collapse path of the window view.  Bound: pcg_window_checks.BOUND["windows"] = 100 x the host PCG's own rounding spread (3e-12).
Converged solves: both preconditioners against the oracle's per-mode SuperLU within pcg_window_checks.CONVERGED_BOUND = 10 x what
the stopping rule leaves the host PCG (5e-10), repeat runs bit-identical.  Whole runs against the reference's recorded runs at the
margin test_hip_long_horizon.py gives another PCG at this tolerance.  Both bounds are measured by test_pcg_windows_cpu.py."""
import functools
import logging
import os

import numpy as np
import pytest

import pcg_checks as pc
import pcg_window_checks as pw
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

RESIDUAL_TOL = 1e-9      # test_hip_pcg.py's


@functools.lru_cache(maxsize=None)
def plan_of(mesh_key, T):
    from dots_socp_amd.geometry import build_plan

    return build_plan(T, pc._geometry(*mesh_key), reorder=True)


@functools.lru_cache(maxsize=None)
def host(mesh_key, T, eps):
    """The host PCG on the CSR and masses the device is handed: ``{cg_max_iter: Result}``, computed once and read-only."""
    _, p = pc.seeded_problem(mesh_key, T, "modal_pcg", eps)
    out = pc.host_pcg(pc.with_plan_operator(p, plan_of(mesh_key, T)), eps, pc.ITERATE_TOL, pc.CUTS)
    for res in out.values():
        res.phi.setflags(write=False)
    return out


def open_windowed(geom, T, s, cg_tol, cg_max_iter, **kw):
    from dots_socp_amd.device import DeviceProblem

    dev = DeviceProblem(T, geom, lap_solver="modal_pcg", pcg_windows=True, **kw)
    pc.upload_state(dev, s, cg_tol, cg_max_iter)
    return dev


def solve(dev, s):
    dev.upload("phi", s.phi)
    st = dev.run_phase("laplacian")
    return dev.download("phi"), st


@pytest.mark.parametrize("eps", pc.EPS)
@pytest.mark.parametrize("mesh,T", pw.ITERATE_CASES, ids=[f"{m[0]}-T{T}" for m, T in pw.ITERATE_CASES])
def test_iterates_match_host_pcg(mesh, T, eps):
    key = pw.mesh_key(mesh)
    s, _ = pc.seeded_problem(key, T, "modal_pcg", eps)
    want = host(key, T, eps)
    dev = open_windowed(pc.geometry_of(mesh), T, s, pc.ITERATE_TOL, pc.CUTS[0])
    try:
        assert dev.pcg_windows_ran() == (0, False)      # nothing solved yet
        got = []
        for cut in pc.CUTS:
            dev.set_params(cg_max_iter=cut)
            got.append(solve(dev, s))
            assert dev.pcg_windows_ran() == (pw.WINDOWS[T], True)
        names, vt, cap, G = dev.cg_path()
    finally:
        dev.close()
    if mesh == pw.COLLAPSE_MESH:      # the pitch-256 view has more than 1024 workgroups
        assert "collapse" in names and G > 1024, (names, G)
    else:
        assert names == {"modal"} and vt == 4, (names, vt)
    for cut, (phi, st) in zip(pc.CUTS, got):
        ref = want[cut]
        err = pc.rel_max(phi, ref.phi)
        res_err = abs(st.cg_last_rel_residual - ref.rel_residual) / ref.rel_residual
        print(f"pcg windows {mesh[0]} T {T} eps {eps:g} cut {cut}: phi error {err:.3e} (bound {pw.BOUND['windows']:.0e}), iterations "
              f"{st.cg_last_iterations} (host {ref.iterations}), residual off {res_err:.1e}, not converged {st.cg_not_converged}")
        assert st.cg_last_iterations == ref.iterations
        assert st.cg_not_converged == int(ref.not_converged)
        assert res_err <= RESIDUAL_TOL
        assert err < pw.BOUND["windows"]


@pytest.mark.parametrize("eps", pc.EPS)
@pytest.mark.parametrize("T", pw.HORIZONS)
@pytest.mark.parametrize("preconditioner", ["jacobi", "multigrid"])
def test_converged_solves_match_superlu(preconditioner, T, eps):
    s, _, want = pw.converged_case(T, eps)
    dev = open_windowed(pw.converged_geometry(), T, s, pw.CONVERGED_TOL, pc.CONVERGE)
    try:
        if preconditioner == "multigrid":
            summary = dev.setup_multigrid(eps=eps, coarsest=6)
            assert summary is not None and summary["levels"] >= 2
        out = []
        for _ in range(2):
            phi, st = solve(dev, s)
            assert st.cg_not_converged == 0 and st.cg_last_iterations > 0
            out.append(phi)
        assert dev.pcg_windows_ran() == (pw.WINDOWS[T], True)
        assert ("mg" in dev.cg_path()[0]) == (preconditioner == "multigrid")
    finally:
        dev.close()
    assert np.array_equal(out[0], out[1])
    got = pw.remove_gauge(out[0], s.mass_v) if eps == 0.0 else out[0]
    err = pc.rel_max(got, want)
    print(f"pcg windows converged {preconditioner} T {T} eps {eps:g}: error {err:.3e} (bound {pw.CONVERGED_BOUND:.0e}), "
          f"{st.cg_last_iterations} iterations")
    assert err < pw.CONVERGED_BOUND


def golden(name):
    return np.load(os.path.join(GOLDEN_DIR, name))


def geom_of(g):
    return dict(vertices=g["vertices"], triangles=g["triangles"], mu0=g["mu0"], mu1=g["mu1"])


def kw_of(g):
    return {k[3:]: (g[k].tolist() if g[k].ndim else g[k].item()) for k in g.files if k.startswith("kw_")}


RUNS = [("long_plane8_T383_tol1e-3.npz", "jacobi"), ("long_plane8_T383_tol1e-3.npz", "multigrid"),
        ("long_plane8_T383_cong_tol1e-3.npz", "jacobi"), ("long_plane8_T383_cong_tol1e-3.npz", "multigrid"),
        ("long_plane8_T1023_tol1e-3.npz", "multigrid")]


@pytest.mark.parametrize("fname,preconditioner", RUNS)
def test_runs_match_reference(fname, preconditioner):
    """Stopping iteration, lazy KKT schedule, residuals and cost at rtol = 1e-6, mu within 1e-5 of the recorded run."""
    from dots_socp_amd.socp import solver_socp

    g = golden(fname)
    T = int(g["n_time"])
    sol, hist = solver_socp(T, geom_of(g), lap_solver="modal_pcg", pcg_windows=True, cg_tol=1e-12, preconditioner=preconditioner,
                            mg_coarsest=6, **kw_of(g))
    assert hist.solver_stats["cg_not_converged"] == 0 and hist.solver_stats["cg_iterations"] > 0
    assert int(hist.kkt_iteration[-1]) == int(g["last_iteration"])
    got, want = hist.kkt_errors, g["hist_kkt_errors"]
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), "lazy KKT schedule differs"
    m = ~np.isnan(want)
    assert np.allclose(got[m], want[m], rtol=1e-6, atol=1e-13)
    for key in ("Transportation cost", "Objective value"):
        assert np.allclose(hist.history[key], g["hist_" + key.replace(" ", "_")], rtol=1e-6, atol=0, equal_nan=True), key
    err = float(np.max(np.abs(sol["mu"] - g["sol_mu"])) / np.max(np.abs(g["sol_mu"])))
    print(f"pcg windows run {fname} {preconditioner}: mu off {err:.2e}, PCG iterations {hist.solver_stats['cg_iterations']}")
    assert err < 1e-5


def test_direct_falls_back_to_the_windowed_pcg(monkeypatch, caplog):
    from dots_socp_amd import meshes
    from dots_socp_amd.socp import solver_socp

    geom, _ = meshes.example("sphere", level=2)
    monkeypatch.setenv("DOTS_MEM_BUDGET", "0")
    with caplog.at_level(logging.WARNING, logger="dots_socp_amd"):
        sol, hist = solver_socp(511, geom, nit=20, pcg_windows=True, mg_coarsest=6)
    assert any("does not fit" in r.getMessage() for r in caplog.records)
    assert hist.solver_stats["lap_solver"] == "modal_pcg (asked for modal_direct)"
    assert "does not fit" in hist.solver_stats["lap_solver_fallback"] and hist.solver_stats["cg_iterations"] > 0
    monkeypatch.delenv("DOTS_MEM_BUDGET")
    # the same solver asked for by name, in the numbering the direct solver's plan has
    sol2, hist2 = solver_socp(511, geom, nit=20, lap_solver="modal_pcg", pcg_windows=True, mg_coarsest=6, reorder="nd")
    assert "lap_solver_fallback" not in hist2.solver_stats
    assert np.array_equal(hist.kkt_errors, hist2.kkt_errors, equal_nan=True)
    for k in sol2:
        if k != "checkpoints":
            assert np.array_equal(sol[k], sol2[k]), k


def test_contract():
    from dots_socp_amd import _lib, meshes
    from dots_socp_amd.device import DeviceProblem

    geom, _ = meshes.example("sphere", level=2)
    old = "T + 1 > 256 needs the direct solver (dots_front_setup); the modal PCG takes T + 1 <= 256"
    for kw in (dict(lap_solver="modal_pcg", time_slab=(0, 2)), dict(lap_solver="spacetime_pcg")):
        dev = DeviceProblem(63, geom, **kw)
        try:
            with pytest.raises(_lib.HipLibraryError) as e:
                dev.enable_pcg_windows()
            assert e.value.status == _lib.ERR_STATE and not dev.pcg_windows
        finally:
            dev.close()
    with pytest.raises(_lib.HipLibraryError) as e:
        DeviceProblem(63, geom, lap_solver="spacetime_pcg", pcg_windows=True)
    assert e.value.status == _lib.ERR_STATE

    rng = np.random.default_rng(11)
    dev = DeviceProblem(300, geom, lap_solver="modal_pcg", reorder="nd")
    try:
        state = {k: rng.standard_normal(dev.shape(k)) for k in ("phi",) + pc.RHS_ARRAYS}

        def laplacian():
            for k, a in state.items():
                dev.upload(k, a)
            st = dev.run_phase("laplacian")
            return dev.download("phi"), st

        dev.set_params(cg_tol=1e-10)
        dev.enable_pcg_windows()
        phi_pcg, st = laplacian()
        assert st.cg_not_converged == 0 and st.cg_last_iterations > 0 and dev.pcg_windows_ran() == (2, True)
        assert dev.setup_multigrid(coarsest=6) is not None      # accepted with n_cols = T + 1
        assert laplacian()[1].cg_not_converged == 0 and "mg" in dev.cg_path()[0]
        # what stays refused above 256 with the switch on
        with pytest.raises(_lib.HipLibraryError, match="256") as e:
            dev.mg_apply(np.zeros((301, dev.V)))
        assert e.value.status == _lib.ERR_STATE
        for which in (0, 1, 2):
            with pytest.raises(_lib.HipLibraryError, match="256") as e:
                dev.bench_kernel(which, reps=1)
            assert e.value.status == _lib.ERR_STATE
        # switched off again: the old refusals with their message, the hierarchy of the windowed layout gone
        dev.enable_pcg_windows(False)
        for call in (lambda: dev.step(1), lambda: dev.run_phase("laplacian"), lambda: dev.setup_multigrid(coarsest=6)):
            with pytest.raises(_lib.HipLibraryError, match="256") as e:
                call()
            assert e.value.status == _lib.ERR_STATE
        with pytest.raises(_lib.HipLibraryError) as e:
            dev.run_phase("laplacian")
        assert old in str(e.value)
        # an installed and enabled factor keeps precedence: the sweeps, bit for bit what the context gives without the switch
        dev.setup_frontal()
        phi_direct, st = laplacian()
        assert st.cg_last_iterations == 0
        dev.enable_pcg_windows()
        phi_switch, st = laplacian()
        assert st.cg_last_iterations == 0 and np.array_equal(phi_switch, phi_direct)
        assert dev.pcg_windows_ran() == (0, False)      # no PCG solve since the switch was set
        dev.enable_frontal(False)      # the factor switched off: now the windows run
        phi_again, st = laplacian()
        assert st.cg_last_iterations > 0 and dev.pcg_windows_ran() == (2, True) and np.array_equal(phi_again, phi_pcg)
    finally:
        dev.close()

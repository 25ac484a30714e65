"""GPU tests of the direct solver at long time horizons: T + 1 in (256, 1024], mode pitches 512 and 1024.

Above 256 time nodes the factorisation and the sweeps cut the mode axis into chunks of 256 (kernels_factor.hip, kernels_front.hip) and the
time transforms run as k_time_modes_wide (kernels_modes.hip).  Whole runs against the reference's recorded runs (tests/golden/long_*.npz,
make_long_horizon.py), the Laplacian phase against the oracle's per-mode SuperLU, the element-wise phases against the oracle, the batched
solver against runs alone, and the error contract of the limits."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, has_gpu, load_oracle
from dots_socp_amd import meshes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

O = load_oracle()
LONG = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN_DIR, "long_*.npz")))
STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")
MESHES = {"sphere": dict(level=2), "torus": dict(nu=16, nv=10), "knot": dict(nu=60, nv=8)}


def golden(name):
    return np.load(os.path.join(GOLDEN_DIR, name))


def geom_of(g):
    return dict(vertices=g["vertices"], triangles=g["triangles"], mu0=g["mu0"], mu1=g["mu1"])


def kw_of(g):
    return {k[3:]: (g[k].tolist() if g[k].ndim else g[k].item()) for k in g.files if k.startswith("kw_")}


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def remove_gauge(phi, mass_v):
    w = np.broadcast_to(mass_v[None, :], phi.shape)
    return phi - np.sum(phi * w) / np.sum(w)


def same_run(hist, want_iteration, want_kkt, want_hist, rtol):
    assert int(hist.kkt_iteration[-1]) == int(want_iteration)
    got = hist.kkt_errors
    assert got.shape == want_kkt.shape
    assert np.array_equal(np.isnan(got), np.isnan(want_kkt)), "lazy KKT schedule differs"
    m = ~np.isnan(want_kkt)
    assert np.allclose(got[m], want_kkt[m], rtol=rtol, atol=1e-13)
    for key in ("Transportation cost", "Objective value"):
        assert np.allclose(hist.history[key], want_hist[key], rtol=rtol, atol=0, equal_nan=True), key


@pytest.mark.parametrize("fname", LONG)
def test_runs_match_reference(fname):
    from dots_socp_amd.socp import solver_socp

    g = golden(fname)
    sol, hist = solver_socp(int(g["n_time"]), geom_of(g), **kw_of(g))
    assert hist.solver_stats.get("lap_solver_fallback") is None
    want_hist = {k: g["hist_" + k.replace(" ", "_")] for k in ("Transportation cost", "Objective value")}
    same_run(hist, g["last_iteration"], g["hist_kkt_errors"], want_hist, 1e-6)
    assert rel(sol["mu"], g["sol_mu"]) < 1e-5


def test_direct_matches_spacetime_pcg():
    """An independent path that already ran at these pitches: the Jacobi-PCG on the space-time operator."""
    from dots_socp_amd.socp import solver_socp

    g = golden("long_plane8_T383_tol1e-3.npz")
    kw = kw_of(g)
    _, hd = solver_socp(383, geom_of(g), **kw)
    _, hp = solver_socp(383, geom_of(g), lap_solver="spacetime_pcg", preconditioner="jacobi", cg_tol=1e-12, **kw)
    assert hp.solver_stats["cg_not_converged"] == 0
    same_run(hd, hp.kkt_iteration[-1], hp.kkt_errors, hp.history, 1e-6)


def make_pair(geom, T, eps=0.0, congestion=0.0, seed=7, s=None):
    """The oracle's solver with a seeded state and a device context holding the same state (``s``: that oracle solver, already made)."""
    from dots_socp_amd.device import DeviceProblem

    if s is not None:
        dev = DeviceProblem(T, geom, lap_solver="modal_pcg", reorder="nd")
        for k in STATE:
            dev.upload(k, s[k])
        dev.set_params(r=1.7, scale_z=2.5, const_d=1.3, norm_d=s["norm_d"], congestion=congestion, eps=eps, tau=s["tau"])
        return None, dev
    s = O.OracleSolver(T, geom, congestion=congestion, eps=eps)
    rng = np.random.default_rng(seed)
    for k in STATE:
        setattr(s, k, rng.standard_normal(getattr(s, k).shape))
    s.beta_fst[:, ::3] -= 6.0     # all three branches of the cone projection
    s.beta_fst[:, 1::3] += 6.0
    s.r, s.sz, s.d = 1.7, 2.5, 1.3
    s.norm_d *= 1.3
    s.bnd /= s.r
    dev = DeviceProblem(T, geom, lap_solver="modal_pcg", reorder="nd")
    for k in STATE:
        dev.upload(k, getattr(s, k))
    dev.set_params(r=s.r, scale_z=s.sz, const_d=s.d, norm_d=s.norm_d, congestion=congestion, eps=eps, tau=s.tau)
    return s, dev


@pytest.mark.parametrize("mesh", sorted(MESHES))
@pytest.mark.parametrize("T", [300, 511, 600, 1023])
@pytest.mark.parametrize("eps", [0.0, 1e-2])
def test_laplacian_phase(mesh, T, eps, monkeypatch):
    """Per-mode SuperLU of the oracle after gauge, repeat runs bit-identical; merged bands with the top band as L'^-1 or as S^-1, and one
    band per tree height (DOTS_FRONT_BANDS=off: the band kernels take the leaves).  Chunks of 256 modes: T = 300 / 1023 end on a partly live
    chunk, T = 511 on a full one, T = 600 (pitch 1024) leaves the last chunk without a live mode."""
    geom, _ = meshes.example(mesh, **MESHES[mesh])
    s, dev = make_pair(geom, T, eps=eps)
    dev.close()
    init = {k: getattr(s, k).copy() for k in STATE}
    init.update(norm_d=s.norm_d, tau=s.tau)
    s.step_laplacian()
    want = remove_gauge(s.phi, s.mass_v) if eps == 0.0 else s.phi
    for bands, top in (("auto", None), ("auto", True), ("auto", False), ("off", False)):
        monkeypatch.setenv("DOTS_FRONT_BANDS", bands)      # (read when the plan's tree is cut into bands)
        _, dev = make_pair(geom, T, eps=eps, s=init)
        try:
            summary = dev.setup_frontal(eps=eps, top_inverse=top)
            assert int(dev.lib.dots_front_pitch(dev._h)) == (512 if T < 512 else 1024)
            assert dev.debug_counter(4) == 0      # no leaf inverses above a pitch of 256
            if bands == "off":
                assert summary["bands"] == list(range(len(summary["bands"])))
            out = []
            for _ in range(2):
                for k in STATE:
                    dev.upload(k, init[k])
                st = dev.run_phase("laplacian")
                assert st.cg_not_converged == 0
                out.append(dev.download("phi"))
            assert np.array_equal(out[0], out[1]), ("repeat", bands, top)
            got = remove_gauge(out[0], s.mass_v) if eps == 0.0 else out[0]
            assert rel(got, want) < 1e-10, (bands, top, summary.get("bands"), rel(got, want))
        finally:
            dev.close()


@pytest.mark.parametrize("T", [383, 1023])
@pytest.mark.parametrize("congestion", [0.0, 0.15])
def test_elementwise_phases(T, congestion):
    geom, _ = meshes.example("sphere", level=2)
    s, dev = make_pair(geom, T, congestion=congestion)
    try:
        s.step_soc_projection()
        dev.run_phase("soc_projection")
        for k in ("z_fst", "z_mid", "z_end"):
            assert rel(dev.download(k), getattr(s, k)) < 1e-12, k
        s.step_q_lambda()
        s.step_multipliers()
        dev.run_phase("q_lambda_mult")
        for k in ("A", "B", "lambda_c", "mu", "E", "beta_fst", "beta_mid", "beta_end"):
            assert rel(dev.download(k), getattr(s, k)) < 1e-12, k
        want = [f() for f in s.kkt_functions()]
        got = dev.kkt(range(7))
        for i in range(7):
            assert abs(got[i][0] - want[i][0]) <= 1e-12 * abs(want[i][0]), i
        cost, obj = dev.objective()
        wc, wo = s.objective()
        assert abs(cost - wc) < 1e-12 * abs(wc) and abs(obj - wo) < 1e-12 * abs(wo)
    finally:
        dev.close()


def test_batched_runs_equal_runs_alone():
    from dots_socp_amd.device import DeviceProblem, laplacian_solve_many
    from dots_socp_amd.socp import solver_socp, solver_socp_many

    geom, _ = meshes.example("sphere", level=2)
    v, av = geom["vertices"], geom["area_vertices"]
    probs = []
    for k, c in enumerate(([0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0])):
        mu0 = meshes.gaussian_density(v, av, c, 0.1)
        mu1 = meshes.gaussian_density(v, av, [-x for x in c], 0.1)
        probs.append(dict(mu0=mu0 / mu0.sum(), mu1=mu1 / mu1.sum(), nit=40, tol=1e-12, congestion=0.05 * k))
    out = solver_socp_many(511, geom, probs, max_batch=2)
    for p, (sol, hist) in zip(probs, out):
        sol1, hist1 = solver_socp(511, {**geom, "mu0": p["mu0"], "mu1": p["mu1"]}, nit=p["nit"], tol=p["tol"], congestion=p["congestion"])
        assert np.array_equal(hist.kkt_errors, hist1.kkt_errors, equal_nan=True)
        for k in ("phi", "mu", "E", "A", "B"):
            assert np.array_equal(sol[k], sol1[k]), k
    # the batched sweeps at pitch 512 on one factor, each result equal to its solve alone.  Two problems (NR = 2): every launch takes both
    # (the 1024-thread forward launches take 2 right-hand sides): one solve's launches, none split (dots_debug_counter 7, 8).  Three (NR = 4):
    # the 1024-thread forward launches of this small mesh's bands are split in halves
    owner = DeviceProblem(511, geom, lap_solver="modal_pcg", reorder="nd")
    devs = [owner]
    try:
        summary = owner.setup_frontal()
        for _ in range(2):
            d = DeviceProblem(511, geom, lap_solver="modal_pcg", plan=owner.plan)
            devs.append(d)
            d.share_frontal(owner)
        lps = summary["launches_per_solve"]
        rng = np.random.default_rng(5)
        rhs = [rng.standard_normal((512, owner.V)) for _ in range(3)]
        alone = [laplacian_solve_many([d], [b])[0] for d, b in zip(devs, rhs)]
        assert owner.debug_counter(7) == lps and owner.debug_counter(8) == 0
        two = laplacian_solve_many(devs[:2], rhs[:2])
        assert owner.debug_counter(7) == lps and owner.debug_counter(8) == 0
        three = laplacian_solve_many(devs, rhs)
        launches, split = owner.debug_counter(7), owner.debug_counter(8)
        assert split > 0 and launches > lps and split <= launches, (launches, split, lps)
        for k in range(3):
            assert np.all(np.isfinite(alone[k])) and np.array_equal(three[k], alone[k]), k
            if k < 2:
                assert np.array_equal(two[k], alone[k]), k
    finally:
        for d in devs[::-1]:
            d.close()


def test_error_contract(monkeypatch):
    from dots_socp_amd import _lib
    from dots_socp_amd.device import DeviceProblem
    from dots_socp_amd.socp import solver_socp

    geom, _ = meshes.example("sphere", level=2)
    with pytest.raises(ValueError, match="modal_direct"):
        solver_socp(300, geom, lap_solver="modal_pcg")
    with pytest.raises(ValueError, match="1024"):
        solver_socp(1024, geom)
    with pytest.raises(_lib.HipLibraryError, match="1024"):
        DeviceProblem(1024, geom, lap_solver="modal_pcg")
    with pytest.raises(_lib.HipLibraryError, match="256") as exc:
        DeviceProblem(300, geom, lap_solver="modal_pcg", time_slab=(0, 2))
    assert exc.value.status == _lib.ERR_ARGUMENT
    # a modal context of T + 1 > 256 without a factor refuses the PCG's entry points
    dev = DeviceProblem(300, geom, lap_solver="modal_pcg")
    try:
        for call in (lambda: dev.step(1), lambda: dev.run_phase("laplacian"), lambda: dev.setup_multigrid(coarsest=6),
                     lambda: dev.bench_kernel(0, reps=1), lambda: dev.bench_kernel(1, reps=1), lambda: dev.bench_kernel(2, reps=1)):
            with pytest.raises(_lib.HipLibraryError, match="256") as exc:
                call()
            assert exc.value.status == _lib.ERR_STATE
        # a budget too small: ERR_MEMORY, and the context takes a factor afterwards
        monkeypatch.setenv("DOTS_MEM_BUDGET", "0")
        with pytest.raises(_lib.HipLibraryError) as exc:
            dev.setup_frontal()
        assert exc.value.status == _lib.ERR_MEMORY
        monkeypatch.delenv("DOTS_MEM_BUDGET")
        dev.setup_frontal()
        assert dev.run_phase("laplacian").cg_not_converged == 0
        for which in (0, 1):      # with a factor too: the PCG kernels stay refused, the sweeps run
            with pytest.raises(_lib.HipLibraryError, match="256") as exc:
                dev.bench_kernel(which, reps=1)
            assert exc.value.status == _lib.ERR_STATE
        assert dev.bench_kernel(3, reps=1)[0] > 0.0
        dev.enable_frontal(False)      # the factor switched off: the PCG would run, and is refused
        with pytest.raises(_lib.HipLibraryError, match="256"):
            dev.run_phase("laplacian")
        dev.enable_frontal(True)
        assert np.all(np.isfinite(dev.download("phi")))
    finally:
        dev.close()
    monkeypatch.setenv("DOTS_MEM_BUDGET", "0")
    with pytest.raises(_lib.HipLibraryError) as exc:
        solver_socp(511, geom, nit=2)
    assert exc.value.status == _lib.ERR_MEMORY and "does not fit" in str(exc.value)

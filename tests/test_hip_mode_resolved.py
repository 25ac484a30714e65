"""GPU: step 1's solve checked per time mode against a refined reference (tests/mode_checks.py).

Every other test of the solve measures max|got - want| / max|want| over the nodal array for a white right-hand side, a figure the low
time modes own: test_mode_checks_cpu.py plants defects in the high modes that pass it.  Here the right-hand sides are band-limited in
time (one octave of modes per solve) and every mode a of the band is compared with a long-double-refined solve of its own
K + (sigma_a + eps) M; what the solve leaves in the modes outside the band (``leak``) is bounded too.

(a) ``test_direct_solve``: device.laplacian_solve_many (forward transform, sweeps, inverse transform), one band per context of a
    share_frontal family (8 per batched call, the rest in a second), at every pitch and chunk shape: T = 6 (pitch 8), 20 (32, ragged),
    63 and 127 (64 and 128: the matrix-core transforms), 300 (512, last chunk of 256 partly live), 600 (1024, last chunk dead), 1023
    (1024, full); eps 0 and 1e-2; the factor from the device's kernels and from the host (which separates the factorisation kernels from
    the sweeps).  ``test_direct_solve_variants``: at T = 63 and 127 also one band per tree height, the top band as factors, and the forced
    forward-sweep variants of test_hip_frontal.test_forward_kernel_variants_agree.
(b) ``test_phase_launch``: run_phase("laplacian"), the iteration's own right-hand-side launch (k_rhs_modes2 below pitch 64,
    k_rhs_modes_mfma at 64 and 128; asserted on dots_debug_counter 12), on planted states: zero except mu, which a cumulative sum in
    long double chooses so that the oracle's laplacian_rhs() is a band without mode 0 (mu1 = mu0: the boundary term has no time sum).
    b is the oracle's own fp64 laplacian_rhs(): the reference covers what rounding leaks out of the band.
(c) ``test_iterative_solvers``: the same planted states through the modal PCG (Jacobi; with the multigrid preconditioner; in windows of
    256 modes) and the space-time PCG at cg_tol = 1e-12, the path asserted on dots_debug_counter 13 and 14.

Bounds (from the reference, none from a device run): direct paths tol_a = 16 max(p, 2^-53 kappa_a), p the worst per-mode error of the
plain fp64 solve mode_checks.plain_solve of the same right-hand sides against the same reference, kappa_a = (lambda_max + sigma_a +
eps) / (lambda_min + sigma_a + eps) (lambda_2 below mode 0 at eps = 0); the leak the same with the largest kappa outside the band.
PCG paths: 16 q, q the worst per-mode error of the band (and the leak) of pcg_checks.host_pcg, the fp64 host PCG with the device's
stopping rule, with the direct bound as floor.

MEASURED on an MI355X (worst per-mode error of the case; in brackets its share of the bound, then the leak's share of its bound):

    path                          T      p / q               eps = 0                     eps = 1e-2
    direct, device factor         6      p 2.2e-15 / 3.3e-13  3.2e-15 (0.05, 0.01)       2.5e-13 (0.00, 0.00)
    (host factor in the second    20     p 3.2e-15 / 3.3e-13  3.8e-15 (0.06, 0.05)       2.5e-13 (0.00, 0.00)
    line where it differs)               host                 5.3e-15 (0.08, 0.05)       3.2e-13 (0.01, 0.00)
                                  63     p 7.0e-15 / 2.4e-13  7.1e-15 (0.06, 0.09)       5.7e-14 (0.00, 0.00)
                                         host                 7.1e-15 (0.06, 0.09)       4.2e-13 (0.01, 0.00)
                                  127    p 4.0e-14 / 3.3e-13  4.1e-14 (0.06, 0.12)       1.9e-13 (0.01, 0.04)
                                  300    p 1.9e-13 / 3.3e-13  1.9e-13 (0.06, 0.05)       1.9e-13 (0.04, 0.08)
                                  600    p 9.7e-13            9.7e-13 (0.06, 0.07)       9.7e-13 (0.06, 0.60)
                                  1023   p 1.7e-12            1.7e-12 (0.06, 0.21)       1.7e-12 (0.06, 0.43)
    direct, refplane4             20     p 4.0e-15 / 2.1e-13  4.2e-15 (0.07, 0.05)       3.9e-13 (0.02, 0.01)
                                  127    p 2.5e-14 / 2.1e-13  2.6e-14 (0.06, 0.18)       2.5e-13 (0.01, 0.02)
    direct, forced variants       63     as above             7.0e-15 to 7.1e-15         1.3e-14 to 5.7e-14
                                  127    as above             4.0e-14 to 4.1e-14         1.9e-13 to 2.2e-13
    run_phase, k_rhs_modes2       7      p 8.5e-16 / 1.1e-15  1.1e-15 (0.08, 0.01)       9.2e-16 (0.05, 0.00)
                                  20     p 3.1e-15 / 3.3e-15  3.2e-15 (0.06, 0.03)       3.3e-15 (0.06, 0.00)
    run_phase, k_rhs_modes_mfma   63     p 7.3e-15 / 7.4e-15  8.0e-15 (0.07, 0.10)       7.8e-15 (0.07, 0.02)
                                  127    p 3.1e-14            3.1e-14 (0.06, 0.11)       3.1e-14 (0.06, 0.11)
    modal PCG, Jacobi             20     q 1.3e-12            1.3e-12 (0.06, 0.03)       1.3e-12 (0.06, 0.00)
                                  127    q 9.4e-13            9.4e-13 (0.06, 0.07)       9.4e-13 (0.06, 0.12)
                                  255    q 1.1e-12            1.1e-12 (0.06, 0.08)       1.1e-12 (0.06, 0.27)
    modal PCG, multigrid          127    q 9.4e-13 (Jacobi's) 8.3e-13 (0.52, 0.07)       8.3e-13 (0.52, 0.12)
    modal PCG in windows          383    q 1.2e-12            1.2e-12 (0.06, 0.36)       1.2e-12 (0.06, 0.10)
    space-time PCG                20     q 7.1e-13 / 6.5e-13  7.1e-13 (0.06, 0.06)       6.5e-13 (0.06, 0.06)

(p / q: eps = 0 / eps = 1e-2 where they differ: at eps = 1e-2 mode 0 has kappa = 3e4 and owns p on the short horizons.)  The device sits on
the plain fp64 solve's own error in every mode -- both carry the fp64 sigma_a of geometry.time_modes and the fp64 transforms, which is what
p consists of -- so the margin of 16 is unused but for the multigrid PCG, whose iterates are not the Jacobi host PCG's.  No defect found.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import mode_checks as mc
import pcg_checks as pc
import step_checks as sc
from conftest import has_gpu, load_oracle
from dots_socp_amd import geometry, meshes
from test_hip_batch_pitches import ND_LEAF, pitch_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

O = load_oracle()
LD = np.longdouble
EPS = (0.0, 1e-2)
T_DIRECT = (6, 20, 63, 127, 300, 600, 1023)
T_PHASE = (7, 20, 63, 127)
NR = 8                          # contexts of one batched call
PCG_TOL = 1e-12
# solver -> T: the modal PCG with Jacobi, with the multigrid preconditioner, in windows of 256 modes, and the space-time PCG
PCG_CASES = [("modal_pcg", 20), ("modal_pcg", 127), ("modal_pcg", 255), ("modal_pcg+mg", 127), ("modal_pcg+windows", 383), ("spacetime_pcg", 20)]


def leaf_of(T):
    return ND_LEAF.get(T, 16)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """sphere level 2 (V = 162: leaf kernels below a merged band below an inverted top band at the leaf sizes of ND_LEAF), the open
    refined plane of the golden fixtures, and the sphere with mu1 = mu0 for the planted states."""
    if name == "refplane4":
        return sc.geometry("ops_refplane4")
    g = meshes.example("sphere", level=2)[0]
    if name == "sphere2_same_ends":
        return dict(vertices=g["vertices"], triangles=g["triangles"], mu0=g["mu0"], mu1=g["mu0"])
    assert name == "sphere2"
    return g


@functools.lru_cache(maxsize=None)
def operator(name, T):
    """(plan, K, mass): the operator the device is handed (reorder="nd"), dense, in the caller's numbering."""
    plan = geometry.build_plan(T, mesh(name), reorder="nd", nd_leaf=leaf_of(T))
    return (plan,) + mc.plan_operator(plan)


def yardstick(K, mass, T, eps, bands, b):
    """reference, kappa and p (the plain fp64 solve's worst per-mode error) of the stack b[k] of right-hand sides in the bands[k]."""
    xr = mc.reference(K, mass, T, eps, b)
    x = mc.plain_solve(K, mass, T, eps, b)
    p = max(float(mc.mode_errors(x[k], xr[k], S, mass, eps)[0].max()) for k, S in enumerate(bands))
    for a in (b, xr):
        a.setflags(write=False)
    return dict(bands=bands, b=b, xr=xr, p=p, kappa=mc.kappa(K, mass, T, eps))


@functools.lru_cache(maxsize=None)
def direct_case(name, T, eps):
    """One right-hand side per octave of modes; computed once per (mesh, T, eps) and read-only."""
    _, K, mass = operator(name, T)
    bands = mc.octaves(T + 1)
    b = np.stack([mc.band_rhs(T, mass.size, S, 100 + k, eps) for k, S in enumerate(bands)])
    return yardstick(K, mass, T, eps, bands, b)


def check_bands(c, xs, mass, eps, what, record_property, q=None):
    """Every band's solution within its bounds; prints and records the worst figures before it asserts."""
    n = c["xr"].shape[1]
    rows, worst_e, worst_ratio, worst_leak = [], 0.0, 0.0, 0.0
    for k, S in enumerate(c["bands"]):
        assert np.all(np.isfinite(xs[k])), (what, k)
        e, leak = mc.mode_errors(xs[k], c["xr"][k], S, mass, eps)
        tol, tol_leak = mc.tolerances(c["p"], c["kappa"], S)
        if q is not None:
            tol, tol_leak = np.maximum(tol, mc.MARGIN * q[k][0]), max(tol_leak, mc.MARGIN * q[k][1])
        rows.append((S, e, leak, tol, tol_leak))
        worst_e, worst_ratio, worst_leak = max(worst_e, float(e.max())), max(worst_ratio, float((e / tol).max())), max(worst_leak, leak / tol_leak)
    qs = "" if q is None else f", q = {max(x[0] for x in q):.2e}"
    print(f"mode resolved {what}: worst per-mode error {worst_e:.2e} = {worst_ratio:.2f} of its bound, leak {worst_leak:.2f} of its bound, "
          f"p = {c['p']:.2e}{qs}")
    record_property("worst_mode_error", worst_e)
    record_property("worst_error_over_bound", worst_ratio)
    record_property("worst_leak_over_bound", worst_leak)
    record_property("p", c["p"])
    if q is not None:
        record_property("q", max(x[0] for x in q))
    for S, e, leak, tol, tol_leak in rows:
        mc.assert_modes(e, leak, tol, tol_leak, S, n, what)


# ---- (a) the direct solve ---------------------------------------------------------------------------------------------------------------
def solve_bands(name, T, eps, b, numeric="device", top_inverse=None):
    """laplacian_solve_many on a share_frontal family, one right-hand side per context: NR per batched call, the rest in a second."""
    from dots_socp_amd.device import DeviceProblem, laplacian_solve_many

    geom = mesh(name)
    owner = DeviceProblem(T, geom, lap_solver="modal_pcg", reorder="nd", nd_leaf=leaf_of(T))
    devs = [owner]
    try:
        owner.set_params(r=1.3, eps=eps)
        summary = owner.setup_frontal(eps=eps, numeric=numeric, top_inverse=top_inverse)
        for _ in range(min(len(b), NR) - 1):
            d = DeviceProblem(T, geom, lap_solver="modal_pcg", plan=owner.plan)
            devs.append(d)
            d.set_params(r=1.3, eps=eps)
            d.share_frontal(owner)
        xs = laplacian_solve_many(devs[:min(len(b), NR)], list(b[:NR]))
        if len(b) > NR:
            xs += laplacian_solve_many(devs[:len(b) - NR], list(b[NR:]))
        info = dict(summary, pitch=int(owner.lib.dots_front_pitch(owner._h)), leaves=owner.debug_counter(4))
    finally:
        for d in devs[::-1]:
            d.close()
    return xs, info


DIRECT = [("sphere2", T) for T in T_DIRECT] + [("refplane4", T) for T in (20, 127)]


@pytest.mark.parametrize("numeric", ["device", "host"])
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("name,T", DIRECT, ids=[f"{m}-T{T}" for m, T in DIRECT])
def test_direct_solve(name, T, eps, numeric, record_property):
    c = direct_case(name, T, eps)
    _, _, mass = operator(name, T)
    xs, info = solve_bands(name, T, eps, c["b"], numeric=numeric)
    assert info["pitch"] == pitch_of(T)
    if name == "sphere2" and T in ND_LEAF:
        assert info["leaves"] > 0 and len(info["bands"]) > 2, info      # leaf kernels, a merged band of several heights, the top band
    if T + 1 > 256:
        assert info["leaves"] == 0                                       # no leaf inverses above a pitch of 256
    check_bands(c, xs, mass, eps, f"direct {name} T {T} eps {eps:g} factor {numeric}", record_property)


def variants_for(T):
    groups = 64 // max(pitch_of(T) // 2, 1)      # lane groups of a wavefront = the largest Q of the row kernel
    out = [("unmerged", {"DOTS_FRONT_BANDS": "off"}, None), ("top_not_inverted", {}, False), ("fold", {"DOTS_FRONT_ROWS": "0"}, None),
           ("rows_everywhere", {"DOTS_FRONT_ROWS": "2"}, None), ("leaves_in_band_kernels", {"DOTS_FRONT_LEAFINV": "0"}, None),
           ("unmerged_leaves_in_band_kernels", {"DOTS_FRONT_BANDS": "off", "DOTS_FRONT_LEAFINV": "0"}, None),
           ("unmerged_fold", {"DOTS_FRONT_BANDS": "off", "DOTS_FRONT_ROWS": "0"}, None)]
    out += [(f"r{q}_leaves", {"DOTS_FRONT_BANDS": "off", "DOTS_FRONT_CFG": f"fwd:r{q}"}, None) for q in (1, 2, 4, 8) if q <= groups]
    return out


VARIANTS = [(T, tag, env, top) for T in (63, 127) for tag, env, top in variants_for(T)]


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("T,tag,env,top", VARIANTS, ids=[f"T{T}-{tag}" for T, tag, _, _ in VARIANTS])
def test_direct_solve_variants(T, tag, env, top, eps, monkeypatch, record_property):
    for k, v in env.items():      # (read when the plan's tree is cut into bands and when the factor is installed)
        monkeypatch.setenv(k, v)
    c = direct_case("sphere2", T, eps)
    _, _, mass = operator("sphere2", T)
    xs, info = solve_bands("sphere2", T, eps, c["b"], top_inverse=top)
    assert info["pitch"] == pitch_of(T)
    if env.get("DOTS_FRONT_BANDS") == "off":
        assert info["bands"] == list(range(len(info["bands"])))
    if "DOTS_FRONT_LEAFINV" in env:
        assert info["leaves"] == 0
    if top is not None:
        assert info["top_inverse"] == top
    check_bands(c, xs, mass, eps, f"direct sphere2 T {T} eps {eps:g} {tag}", record_property)


# ---- the planted states of (b) and (c) --------------------------------------------------------------------------------------------------
def planted_oracle(T, eps):
    """The oracle with make_pair's parameters (test_hip_phases.py) on the sphere with mu1 = mu0, every array zero."""
    with pc._no_factorisation():
        s = O.OracleSolver(T, mesh("sphere2_same_ends"), eps=eps)
    s.r, s.sz, s.d = 1.7, 2.5, 1.3
    s.norm_d *= 1.3
    s.bnd /= s.r
    return s


def planted_mu(s, S, seed):
    """mu with - laplacian_rhs() = Q[:, S] bhat up to rounding, everything else zero: laplacian_rhs() = div_time(h, - mu w) - bnd, and
    div_time(h, y)[t] = (y[t] - y[t-1]) / h with y[-1] = y[T] = 0, so y = h cumsum(bnd - Q[:, S] bhat) in long double.  The sum over all
    T + 1 nodes closes because neither the band (no mode 0) nor the boundary term (mu1 = mu0) has a time sum."""
    assert S[0] > 0
    Q, _ = mc.basis(s.T)
    bhat = np.random.default_rng(seed).standard_normal((len(S), s.V))
    target = mc.ld_matmul(Q[:, np.asarray(S)], bhat)             # = - laplacian_rhs()
    c = -target + s.bnd.astype(LD)                                 # div_time(h, y) must equal this
    y = LD(s.h) * np.cumsum(c[:-1], axis=0)
    return np.asarray(-y / s.mass_v.astype(LD)[None, :], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def planted_case(T, eps):
    """The planted mu per band without mode 0, b = - the oracle's fp64 laplacian_rhs() of each, and the yardstick on the device's
    operator; read-only."""
    s = planted_oracle(T, eps)
    _, K, mass = operator("sphere2_same_ends", T)
    bands = mc.octaves(T + 1)[1:]
    mus, bs = [], []
    for k, S in enumerate(bands):
        mu = planted_mu(s, S, 300 + k)
        s.mu = mu
        b = -s.laplacian_rhs()
        # the condition on the INPUT: outside the band b holds rounding only
        bhat = np.asarray(mc.forward(T, b), dtype=np.float64)
        outside = np.ones(T + 1, dtype=bool)
        outside[S] = False
        assert np.abs(bhat[outside]).max() < 1e-11 * np.abs(bhat[S]).max(), (T, k)
        mu.setflags(write=False)
        mus.append(mu)
        bs.append(b)
    s.mu = np.zeros_like(s.mu)
    out = yardstick(K, mass, T, eps, bands, np.stack(bs))
    out.update(mus=mus, oracle=s)
    return out


def upload_planted(dev, s, mu, **params):
    for k in ("phi",) + pc.RHS_ARRAYS:
        dev.upload(k, mu if k == "mu" else np.zeros(dev.shape(k)))
    dev.set_params(r=s.r, scale_z=s.sz, const_d=s.d, norm_d=s.norm_d, congestion=0.0, eps=s.eps, tau=s.tau, **params)


# ---- (b) the iteration's own launch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("T", T_PHASE)
def test_phase_launch(T, eps, record_property):
    from dots_socp_amd import _lib
    from dots_socp_amd.device import DeviceProblem

    c = planted_case(T, eps)
    _, _, mass = operator("sphere2_same_ends", T)
    want_path = _lib.STEP_PATH["rhs_mfma"] if T + 1 >= 64 else _lib.STEP_PATH["rhs_modes2"]
    xs = []
    with DeviceProblem(T, mesh("sphere2_same_ends"), lap_solver="modal_pcg", reorder="nd", nd_leaf=leaf_of(T)) as dev:
        dev.setup_frontal(eps=eps)
        for mu in c["mus"]:
            upload_planted(dev, c["oracle"], mu)
            assert dev.debug_counter(_lib.STEP_PATH_COUNTER) == 0
            st = dev.run_phase("laplacian")
            assert dev.debug_counter(_lib.STEP_PATH_COUNTER) == want_path, hex(dev.debug_counter(_lib.STEP_PATH_COUNTER))
            assert st.cg_not_converged == 0 and st.cg_last_iterations == 0      # the sweeps, not a PCG
            xs.append(dev.download("phi"))
    check_bands(c, xs, mass, eps, f"phase launch T {T} eps {eps:g}", record_property)


# ---- (c) the iterative solvers --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_pcg_errors(T, eps, modal):
    """Per band (worst per-mode error, leak) of the fp64 host PCG with the device's stopping rule against the reference."""
    c = planted_case(T, eps)
    s = c["oracle"]
    _, K, mass = operator("sphere2_same_ends", T)
    Q, sigma = geometry.time_modes(T)
    out = []
    for k, S in enumerate(c["bands"]):
        prob = pc.Problem(modal=modal, T=T, h=s.h, K=sp.csr_matrix(K), mass=mass, b=c["b"][k], x0=np.zeros_like(c["b"][k]), Q=Q, sigma=sigma)
        res = pc.host_pcg(prob, eps, PCG_TOL, pc.CONVERGE)
        assert not res.not_converged and res.iterations > 0
        e, leak = mc.mode_errors(res.phi, c["xr"][k], S, mass, eps)
        out.append((float(e.max()), leak))
    return out


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("solver,T", PCG_CASES, ids=[f"{s}-T{T}" for s, T in PCG_CASES])
def test_iterative_solvers(solver, T, eps, record_property):
    from dots_socp_amd.device import DeviceProblem

    c = planted_case(T, eps)
    _, _, mass = operator("sphere2_same_ends", T)
    lap_solver, _, extra = solver.partition("+")
    q = host_pcg_errors(T, eps, lap_solver == "modal_pcg")
    xs = []
    with DeviceProblem(T, mesh("sphere2_same_ends"), lap_solver=lap_solver, reorder="nd", nd_leaf=leaf_of(T), pcg_windows=extra == "windows") as dev:
        if extra == "mg":
            dev.set_params(eps=eps)
            summary = dev.setup_multigrid(eps=eps, coarsest=6)
            assert summary is not None and summary["levels"] >= 2
        for mu in c["mus"]:
            upload_planted(dev, c["oracle"], mu, cg_tol=PCG_TOL, cg_max_iter=pc.CONVERGE)
            st = dev.run_phase("laplacian")
            assert st.cg_not_converged == 0 and st.cg_last_iterations > 0
            xs.append(dev.download("phi"))
        names = dev.cg_path()[0]
        assert ("modal" in names) == (lap_solver == "modal_pcg") and ("mg" in names) == (extra == "mg"), names
        assert dev.pcg_windows_ran() == ((2, True) if extra == "windows" else (0, False))
    check_bands(c, xs, mass, eps, f"{solver} T {T} eps {eps:g}", record_property, q=q)

"""The Jacobi PCG of csrc/kernels_cg.hip restated on the host, iterate by iterate (plain numpy / scipy, TEST INFRASTRUCTURE shared by
test_pcg_checks_cpu.py and test_hip_pcg.py):

``CASES``          the meshes, solvers and T of the GPU cases with the launch path each must report (dots_debug_counter 13);
``seeded_problem`` the oracle's right-hand side and the random warm start for a seeded state, as test_hip_phases.make_pair plants it;
``host_pcg``       the PCG with the device's start, stopping rule, freezing of converged columns and units of eight iterations, for a
                   batch of independent columns (MODAL) or one coupled system (SPACETIME), with knobs for deliberate defects.

The host works in the caller's vertex numbering: Jacobi PCG is invariant under the device's permutation up to the order of its sums."""
import contextlib
import functools
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

from conftest import load_oracle
from step_checks import geometry as fixture_geometry

O = load_oracle()
UNIT = 8                      # iterations per graph replay of the Jacobi PCG: the flags are tested between units
ITERATE_TOL = 1e-12           # cg_tol of the iterate cases (make_pair's)
CUTS = (8, 16)                # cg_max_iter of the iterate cases
EPS = (0.0, 1e-2)
RHS_ARRAYS = ("A", "B", "lambda_c", "mu", "E")      # what step 1's right-hand side reads beside phi
MUTATIONS = ("stale_parity", "beta_zero", "no_freeze", "freeze_on_r2", "no_mean_removal", "dinv_without_eps", "drop_unstaged",
             "tol_not_refreshed")

SPHERE2 = ("sphere", dict(level=2))            # V = 162
TORUS_4176 = ("torus", dict(nu=72, nv=58))
TORUS_8352 = ("torus", dict(nu=96, nv=87))
TORUS_1080 = ("torus", dict(nu=40, nv=27))


def _path(vt, cap, G, *bits):
    return dict(bits=set(bits), vt=vt, cap=cap, G=G)


def _cases():
    """id -> family, solver, mesh, T, reorder and the path record the launcher must give (literal numbers: a change of the launcher's
    thresholds fails the case)."""
    sphere_path = {1: (128, 1600, 8), 7: (128, 1600, 8), 20: (32, 448, 8), 63: (16, 256, 16), 100: (8, 160, 24), 127: (8, 160, 24),
                   255: (4, 112, 48)}
    c = {}
    for T in (1, 7, 20, 63):
        c[f"small-T{T}"] = dict(family="small pitches", solver="modal_pcg", mesh=SPHERE2, T=T, path=_path(*sphere_path[T], "modal"))
    for T in (100, 127, 255):
        c[f"wide-T{T}"] = dict(family="wide pitches", solver="modal_pcg", mesh=SPHERE2, T=T, path=_path(*sphere_path[T], "modal"))
    for T in (255, 200):
        c[f"collapse256-T{T}"] = dict(family="collapse 256", solver="modal_pcg", mesh=TORUS_4176, T=T,
                                      path=_path(1, 76, 4176, "modal", "collapse", "small_wg"))
    c["collapse128-T127"] = dict(family="collapse 128", solver="modal_pcg", mesh=TORUS_8352, T=127,
                                 path=_path(2, 88, 4176, "modal", "collapse", "small_wg"))
    for T in (1, 7, 20, 63, 255):
        c[f"spacetime-T{T}"] = dict(family="space-time", solver="spacetime_pcg", mesh=SPHERE2, T=T, path=_path(*sphere_path[T]))
    c["spacetime-collapse-T255"] = dict(family="space-time collapse", solver="spacetime_pcg", mesh=TORUS_4176, T=255,
                                        path=_path(1, 76, 4176, "collapse", "small_wg"))
    c["spacetime-wide-T383"] = dict(family="space-time wide", solver="spacetime_pcg", mesh=TORUS_1080, T=383, path=_path(2, 88, 544))
    c["spacetime-wide-T1023"] = dict(family="space-time wide", solver="spacetime_pcg", mesh=TORUS_1080, T=1023,
                                     path=_path(1, 76, 1080, "collapse"))
    for reorder in (False, True):
        tag = "reordered" if reorder else "hub0"
        for solver in ("modal_pcg", "spacetime_pcg"):
            c[f"wheel200-{solver.split('_')[0]}-{tag}"] = dict(family="wheel", solver=solver, mesh=("wheel", dict(n=200)), T=255, reorder=reorder,
                                                               path=_path(4, 112, 56, *(["modal"] if solver == "modal_pcg" else [])))
        c[f"wheel1500-modal-{tag}"] = dict(family="wheel", solver="modal_pcg", mesh=("wheel", dict(n=1500)), T=7, reorder=reorder,
                                           path=_path(128, 1600, 16, "modal"))
    return c


CASES = _cases()
FAMILIES = tuple(dict.fromkeys(spec["family"] for spec in CASES.values()))
# Freezing: modal, eps = 1e-2, cg_max_iter = 16 and a loose cg_tol chosen on the CPU (test_pcg_checks_cpu.py asserts the conditions)
FREEZE_CASES = {"small-T63": 1e-4, "wide-T255": 1e-5}
FREEZE_EPS = 1e-2
CONVERGE = 2000               # cg_max_iter of the runs to convergence (they take a few dozen iterations)
# Several solves on one context: (eps, cg_tol) in turn, each to convergence from the same uploaded state
SEQUENCE_CASE = "small-T20"
SEQUENCE = ((1e-2, 1e-3), (1e-2, 1e-8), (1e-3, 1e-8))
# The bound of the GPU tests per family: 100 x the rounding spread of the host PCG alone (float64 against np.longdouble, both cuts,
# both eps; measured and asserted by test_pcg_checks_cpu.py::test_rounding_spread_and_bound), never above PHI_TOL = 1e-9.
PHI_CEILING = 1e-9
SPREAD = {
    "small pitches": 1e-14, "wide pitches": 2e-14, "collapse 256": 1e-14, "collapse 128": 2e-14, "space-time": 5e-14,
    "space-time collapse": 1e-13, "space-time wide": 5e-14, "wheel": 5e-14, "freezing": 1e-13, "solve sequence": 1e-12,
}
BOUND = {family: 100.0 * s for family, s in SPREAD.items()}


def wheel_geometry(n):
    """A closed wheel: hub 0 of valence n, rim vertices 1..n of valence 3 on a gently corrugated cone; V = n + 1, F = n; positive densities
    of equal mass.  The hub's CSR row holds n + 1 entries."""
    ang = 2.0 * np.pi * np.arange(n) / n
    rad = 1.0 + 0.1 * np.cos(5.0 * ang)
    rim = np.stack([rad * np.cos(ang), rad * np.sin(ang), 0.05 * np.sin(3.0 * ang)], axis=1)
    vertices = np.concatenate([[[0.0, 0.0, 0.3]], rim])
    triangles = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], dtype=np.int32)
    rng = np.random.default_rng(n)
    mu0, mu1 = rng.uniform(0.5, 1.5, n + 1), rng.uniform(0.5, 1.5, n + 1)
    return dict(vertices=vertices, triangles=triangles, mu0=mu0 / mu0.sum(), mu1=mu1 / mu1.sum())


@functools.lru_cache(maxsize=None)
def _geometry(name, kw):
    if name == "fixture":
        return fixture_geometry(dict(kw)["mesh"])
    if name == "wheel":
        g = wheel_geometry(**dict(kw))
    else:
        from dots_socp_amd import meshes

        g = meshes.example(name, **dict(kw))[0]
    # densities of UNEQUAL mass: the right-hand side of step 1 then has a mean, and the mean removal of the singular mode (eps = 0) has
    # something to remove (with equal masses the divergences and the boundary term sum to rounding noise)
    return dict(vertices=g["vertices"], triangles=g["triangles"], mu0=g["mu0"], mu1=1.25 * g["mu1"])


def geometry_of(mesh):
    name, kw = mesh
    return _geometry(name, tuple(sorted(kw.items())))


@contextlib.contextmanager
def _no_factorisation():
    """The oracle without its sparse LU per time mode: only its right-hand side is wanted, and the factors of the large cases take long."""
    keep = O.LaplacianInverse
    O.LaplacianInverse = lambda *a, **k: None
    try:
        yield
    finally:
        O.LaplacianInverse = keep


def seeded_oracle(T, geom, eps, seed=7, factorise=False):
    """The oracle with make_pair's parameters (test_hip_phases.py) and a seeded random phi and right-hand-side state; the arrays step 1 does
    not read stay zero."""
    with contextlib.nullcontext() if factorise else _no_factorisation():
        s = O.OracleSolver(T, geom, eps=eps)
    rng = np.random.default_rng(seed)
    for k in ("phi",) + RHS_ARRAYS:
        setattr(s, k, rng.standard_normal(getattr(s, k).shape))
    s.r, s.sz, s.d = 1.7, 2.5, 1.3
    s.norm_d *= 1.3
    s.bnd /= s.r
    return s


def upload_state(dev, s, cg_tol, cg_max_iter):
    for k in ("phi",) + RHS_ARRAYS:
        dev.upload(k, getattr(s, k))
    dev.set_params(r=s.r, scale_z=s.sz, const_d=s.d, norm_d=s.norm_d, congestion=0.0, eps=s.eps, tau=s.tau, cg_tol=cg_tol, cg_max_iter=cg_max_iter)


@dataclass(frozen=True)
class Problem:
    modal: bool
    T: int
    h: float
    K: sp.csr_matrix        # K_space = - cotangent Laplacian, the caller's numbering
    mass: np.ndarray        # (V,)
    b: np.ndarray           # (T + 1, V) right-hand side of K x = b in time space: - laplacian_rhs() of the oracle
    x0: np.ndarray          # (T + 1, V) the uploaded phi
    Q: np.ndarray           # (T + 1, T + 1) Q[t, a]
    sigma: np.ndarray       # (T + 1,)


def problem_of(s, solver):
    """The system step 1 solves for the state the oracle ``s`` holds (its phi is the warm start)."""
    from dots_socp_amd.geometry import time_modes

    Q, sigma = time_modes(s.T)
    b, x0 = -s.laplacian_rhs(), s.phi.copy()
    for a in (b, x0):
        a.setflags(write=False)
    return Problem(modal=solver == "modal_pcg", T=s.T, h=s.h, K=(-s.L).tocsr(), mass=s.mass_v.copy(), b=b, x0=x0, Q=Q, sigma=sigma)


@functools.lru_cache(maxsize=None)
def seeded_problem(mesh_key, T, solver, eps, seed=7):
    """``(oracle, Problem)`` of a mesh of ``CASES`` (``mesh_key = (name, sorted kwargs)``), computed once and then read-only."""
    s = seeded_oracle(T, _geometry(*mesh_key), eps, seed)
    return s, problem_of(s, solver)


def case_problem(case, eps, seed=7):
    spec = CASES[case]
    name, kw = spec["mesh"]
    return seeded_problem((name, tuple(sorted(kw.items()))), spec["T"], spec["solver"], eps, seed)


def with_plan_operator(p, plan):
    """``p`` with K_space and the masses the device was handed (the plan's CSR, back in the caller's numbering) in place of the oracle's.
    The oracle forms its cotangents from angles, which on the thin triangles of the wheel (apex angle 2 pi / n) costs about 1e-16 / angle^2
    relative: 1e-13 at n = 200, 1e-11 at n = 1500 -- the assembly's difference, not the PCG's, and beyond the bound of these tests."""
    V = plan.n_vertices
    perm = np.arange(V) if plan.perm_vert is None else np.asarray(plan.perm_vert)
    Kd = sp.csr_matrix((plan.lap_val, plan.lap_col, plan.lap_rowptr), shape=(V, V)).tocoo()
    K = sp.csr_matrix((Kd.data, (perm[Kd.row], perm[Kd.col])), shape=(V, V))
    K.sort_indices()
    mass = np.empty(V)
    mass[perm] = plan.mass_vert
    return Problem(modal=p.modal, T=p.T, h=p.h, K=K, mass=mass, b=p.b, x0=p.x0, Q=p.Q, sigma=p.sigma)


def _spmm(K, X):
    """K X^T transposed back, for X (columns, V); numpy's reduceat where scipy has no kernel for the dtype (np.longdouble)."""
    if X.dtype == np.float64:
        return np.ascontiguousarray((K @ X.T).T)
    prod = K.data.astype(X.dtype)[:, None] * X.T[K.indices]
    return np.ascontiguousarray(np.add.reduceat(prod, K.indptr[:-1], axis=0).T)      # (every row holds its diagonal: no empty row)


def unstaged_dropped(K, plan, vt, cap):
    """K_space with the entries of every tile's rows beyond the staged capacity left out (the defect ``drop_unstaged``): tiles of ``vt``
    rows of the device's CSR (``plan``), of which the first ``cap`` entries are staged.  Returned in the caller's numbering."""
    rp, col, val = plan.lap_rowptr.astype(np.int64), plan.lap_col, plan.lap_val.copy()
    V = rp.size - 1
    first = rp[(np.arange(V) // vt) * vt]                       # the tile's first entry, per row
    local = np.arange(val.size) - np.repeat(first, np.diff(rp))
    val[local >= cap] = 0.0
    Kd = sp.csr_matrix((val, col, plan.lap_rowptr), shape=(V, V)).tocoo()
    perm = np.arange(V) if plan.perm_vert is None else np.asarray(plan.perm_vert)
    return sp.csr_matrix((Kd.data, (perm[Kd.row], perm[Kd.col])), shape=(V, V)), int(np.count_nonzero(local >= cap))


def overflowing_tiles(plan, vt, cap):
    """Tiles of the device's CSR whose rows hold more entries than are staged, and of those the ones whose first unstaged entry lies
    inside a row (the row straddles the capacity)."""
    rp = plan.lap_rowptr.astype(np.int64)
    V = rp.size - 1
    starts = np.arange(0, V, vt)
    over = [int(g) for g, v0 in enumerate(starts) if rp[min(v0 + vt, V)] - rp[v0] > cap]
    straddle = [g for g in over if not np.any(rp[starts[g]:min(starts[g] + vt, V) + 1] - rp[starts[g]] == cap)]
    return over, straddle


@dataclass
class Result:
    phi: np.ndarray             # (T + 1, V) float64, time space
    live_iterations: np.ndarray  # per column: iterations that began with the column live
    iterations: int             # the device's count: iterations that began with at least one live column (FLAG_ITERS)
    rel_residual: float         # sqrt(max crit / bref) as the last iteration that ran saw it (cg_last_rel_residual)
    margin: float               # smallest relative distance of a freeze decision from its threshold
    frozen: np.ndarray          # per column, as the last iteration that ran left the flags
    launched: int

    @property
    def not_converged(self):
        return not bool(np.all(self.frozen))


def apply_operator(p, X, eps, K=None):
    """K X for X (T + 1, V): per mode K_space + (sigma_a + eps) M (MODAL, X in mode space), or the coupled operator
    -(L_time (x) M + I (x) L_space) + eps I (x) M with the Neumann stencil of k_cg_apply<false>."""
    K = p.K if K is None else K
    dt = X.dtype
    mass = p.mass.astype(dt)[None, :]
    out = _spmm(K, X)
    if p.modal:
        return out + (p.sigma.astype(dt)[:, None] + dt.type(eps)) * mass * X
    ct = np.full((p.T + 1, 1), 2.0, dtype=dt)
    ct[0] = ct[-1] = 1.0
    st = ct * X
    st[1:] -= X[:-1]
    st[:-1] -= X[1:]
    return out + mass * (st / dt.type(p.h * p.h) + dt.type(eps) * X)


def jacobi_diagonal(p, eps, dtype=np.float64):
    """D = diag of the operator, (T + 1, V)."""
    dt = np.dtype(dtype)
    if p.modal:
        shift = p.sigma.astype(dt)[:, None]
    else:
        shift = np.full((p.T + 1, 1), 2.0, dtype=dt)
        shift[0] = shift[-1] = 1.0
        shift = shift / dt.type(p.h * p.h)
    return p.K.diagonal().astype(dt)[None, :] + (shift + dt.type(eps)) * p.mass.astype(dt)[None, :]


def host_pcg(p, eps, tol, max_iter, mutation=None, dtype=np.float64, x0=None, dropped=None, stale_tol=None):
    """The Jacobi PCG of ``k_cg_r0`` / ``k_cg_apply`` / ``k_cg_update`` on ``Problem`` ``p`` from the warm start ``x0`` (default: the
    problem's), in ``dtype``.  ``max_iter``: one ``cg_max_iter`` -> one ``Result``; a tuple of them -> ``{cg_max_iter: Result}`` from one
    run (a converged or cut solve changes nothing afterwards).  The device runs units of eight iterations and tests the flags between
    units: the result is the iterate after ``8 ceil(max_iter / 8)`` iterations or the converged one.

    ``mutation``: a deliberate defect (``MUTATIONS``); ``drop_unstaged`` needs ``dropped`` (``unstaged_dropped``), ``tol_not_refreshed``
    the first solve's ``stale_tol``."""
    assert mutation is None or mutation in MUTATIONS, mutation
    dt = np.dtype(dtype)
    cuts = (max_iter,) if np.isscalar(max_iter) else tuple(max_iter)
    if mutation == "tol_not_refreshed":
        tol = stale_tol
    tol2 = dt.type(tol) * dt.type(tol)
    Q = p.Q.astype(dt)
    b = p.b.astype(dt)
    x = (p.x0 if x0 is None else x0).astype(dt)
    if p.modal:      # mode space: column a of the device is row a here
        b, x = Q.T @ b, Q.T @ x
    red = (lambda a: a.sum(axis=1)) if p.modal else (lambda a: a.sum(keepdims=True).reshape(1))
    col = lambda s: s[:, None]      # noqa: E731  per-column scalars against (columns, V) arrays
    if eps == 0.0 and mutation != "no_mean_removal":      # unweighted means: over V for mode 0, over V (T + 1) for the coupled system
        if p.modal:
            b[0] -= b[0].mean()
        else:
            b -= b.mean()
    dinv = 1.0 / jacobi_diagonal(p, 0.0 if mutation == "dinv_without_eps" else eps, dt)
    K_iter = dropped if mutation == "drop_unstaged" else None

    r = b - apply_operator(p, x, eps)
    z = dinv * r
    bref = red(b * dinv * b)
    ncol = bref.size
    frozen = np.zeros(ncol, dtype=bool)
    flags = frozen.copy()
    live_iters = np.zeros(ncol, dtype=np.int64)
    rz_hist = []
    pvec = np.zeros_like(x)
    count, margin, last_crit = 0, np.inf, red(r * z)
    out, launched = {}, 0

    def result():
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bref > 0, last_crit / bref, 0.0)
        phi = (Q @ x) if p.modal else x
        return Result(phi=np.array(phi, dtype=np.float64), live_iterations=live_iters.copy(), iterations=count,
                      rel_residual=float(np.sqrt(max(ratio.max(), 0.0))), margin=float(margin), frozen=flags.copy(), launched=launched)

    done = False
    while not done and launched < max(cuts):
        for _ in range(UNIT):
            rz_new = red(r * z)
            crit = red(r * r) if mutation == "freeze_on_r2" else rz_new
            thr = tol2 * bref
            live = ~frozen
            if np.any(live & (thr > 0)):
                sel = live & (thr > 0)
                margin = min(margin, float(np.min(np.abs(crit[sel] - thr[sel]) / thr[sel])))
            if mutation != "no_freeze":
                frozen = frozen | (crit <= thr)
            last_crit, flags = crit, frozen.copy()
            if mutation == "stale_parity":
                rz_old = rz_hist[-2] if len(rz_hist) >= 2 else np.zeros(ncol, dtype=dt)
            else:
                rz_old = rz_hist[-1] if rz_hist else np.zeros(ncol, dtype=dt)
            rz_hist.append(rz_new)
            if np.all(frozen):
                continue      # nothing runs and nothing is counted
            live = ~frozen
            count += 1
            live_iters[live] += 1
            with np.errstate(divide="ignore", invalid="ignore"):
                beta = np.where(rz_old > 0, rz_new / rz_old, 0.0).astype(dt)
            if mutation == "beta_zero":
                beta[:] = 0.0
            pvec = z + col(beta) * pvec
            Ap = apply_operator(p, pvec, eps, K=K_iter)
            pAp = red(pvec * Ap)
            with np.errstate(divide="ignore", invalid="ignore"):
                alpha = np.where(live & (pAp > 0), rz_new / pAp, 0.0).astype(dt)
            if p.modal and not np.all(live):      # a frozen column changes nothing from then on
                upd = np.nonzero(live)[0]
                x[upd] += col(alpha[upd]) * pvec[upd]
                r[upd] -= col(alpha[upd]) * Ap[upd]
                z[upd] = dinv[upd] * r[upd]
            else:
                x += col(alpha) * pvec
                r -= col(alpha) * Ap
                z = dinv * r
        launched += UNIT
        done = bool(np.all(flags))
        for c in cuts:
            if c not in out and (done or launched >= c):
                out[c] = result()
    return out[cuts[0]] if np.isscalar(max_iter) else out


def permuted(p, seed=3):
    """``(problem, perm)``: ``p`` under a seeded random renumbering of its vertices (vertex ``i`` of the result is vertex ``perm[i]`` of
    ``p``): the same arithmetic with every sum over vertices and every CSR row in another order."""
    perm = np.random.default_rng(seed).permutation(p.mass.size)
    K = p.K[perm][:, perm].tocsr()
    K.sort_indices()
    return Problem(modal=p.modal, T=p.T, h=p.h, K=K, mass=p.mass[perm], b=p.b[:, perm], x0=p.x0[:, perm], Q=p.Q, sigma=p.sigma), perm


def host_pcg_permuted(p, *args, **kw):
    """``host_pcg`` of the renumbered problem with phi back in ``p``'s numbering."""
    q, perm = permuted(p)
    out = host_pcg(q, *args, **kw)
    for res in (out.values() if isinstance(out, dict) else [out]):
        phi = np.empty_like(res.phi)
        phi[:, perm] = res.phi
        res.phi = phi
    return out


def rel_max(a, b):
    """max-norm relative error of ``a`` against ``b``."""
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))

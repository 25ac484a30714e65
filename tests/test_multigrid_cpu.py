"""CPU tests of the host-side multigrid setup (dots_socp_amd/multigrid.py): hierarchy invariants, the
three-kernel form of the V-cycle the device uses, and its quality as a PCG preconditioner."""
import numpy as np
import pytest
import scipy.sparse as sp

from dots_socp_amd import geometry, meshes, multigrid


def problem(name, **kw):
    if name == "refplane":
        v, t = meshes.plane(kw.get("n", 12))
        g, _ = meshes.make_geometry(v, t, np.ones(v.shape[0]) / v.shape[0], np.ones(v.shape[0]) / v.shape[0])
    else:
        g, _ = meshes.example(name, **kw)
    plan = geometry.build_plan(7, g)
    K = sp.csr_matrix((plan.lap_val, plan.lap_col, plan.lap_rowptr), shape=(plan.n_vertices,) * 2)
    return plan, K


CASES = [("sphere", dict(level=3)), ("refplane", dict(n=12)), ("torus", dict(nu=24, nv=16)), ("knot", dict(nu=60, nv=8))]


@pytest.mark.parametrize("name,kw", CASES)
def test_hierarchy_invariants(name, kw):
    plan, K = problem(name, **kw)
    levels = multigrid.build_hierarchy(K, plan.mass_vert, coarsest=12)
    assert len(levels) >= 2
    summary = multigrid.hierarchy_summary(levels)
    assert summary["operator_complexity"] < 2.5
    M = sp.diags(plan.mass_vert).tocsr()
    Kl = K
    for lv in levels:
        # K_l, M_l share one pattern and are symmetric; constants stay in the null space of K_l
        assert np.array_equal(lv.K.indptr, lv.M.indptr) and np.array_equal(lv.K.indices, lv.M.indices)
        assert abs(lv.K - lv.K.T).max() < 1e-12 * abs(lv.K).max()
        assert abs(lv.K - Kl).max() < 1e-12 * abs(Kl).max() and abs(lv.M - M).max() < 1e-12 * abs(M).max()
        if lv.P is not None:
            assert abs(lv.R - lv.P.T).max() == 0.0
            assert np.array_equal(lv.KP.indptr, lv.MP.indptr) and np.array_equal(lv.KP.indices, lv.MP.indices)
            assert abs(lv.KP - lv.K @ lv.P).max() < 1e-12 * abs(lv.KP).max()
            assert abs(lv.MP - lv.M @ lv.P).max() < 1e-12 * max(abs(lv.MP).max(), 1e-300)
            assert np.array_equal(lv.PP.indices, lv.KP.indices) and abs(lv.PP - lv.P).max() == 0.0
            Kl, M = (lv.R @ lv.K @ lv.P).tocsr(), (lv.R @ lv.M @ lv.P).tocsr()
    # the near-null-space candidate is carried exactly: K_l c_l = 0 and P_l c_{l+1} = c_l
    assert np.allclose(levels[0].cand, 1.0)
    for lv, nxt in zip(levels[:-1], levels[1:]):
        assert np.max(np.abs(lv.K @ lv.cand)) < 1e-10 * abs(lv.K).max() * np.max(np.abs(lv.cand))
        assert np.max(np.abs(lv.P @ nxt.cand - lv.cand)) < 1e-10 * np.max(np.abs(lv.cand))


@pytest.mark.parametrize("name,kw", CASES)
@pytest.mark.parametrize("shift", [0.0, 9.3, 1900.0])
def test_fused_cycle_equals_plain_cycle(name, kw, shift):
    plan, K = problem(name, **kw)
    levels = multigrid.build_hierarchy(K, plan.mass_vert, coarsest=12)
    vc = multigrid.CpuVcycle(levels, shift)
    b = np.random.default_rng(1).standard_normal(plan.n_vertices)
    if shift == 0.0:
        b -= b.mean()
    plain, fused = vc.cycle(b), vc.cycle_fused(b)
    assert np.max(np.abs(plain - fused)) < 1e-12 * np.max(np.abs(plain))


def pcg_iterations(A, b, prec, dinv, tol=1e-10, maxit=2000):
    x = np.zeros_like(b)
    r = b.copy()
    z = prec(r)
    p = z.copy()
    rz = r @ z
    bref = b @ (dinv * b)
    for it in range(1, maxit + 1):
        Ap = A @ p
        alpha = rz / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        if r @ (dinv * r) <= tol * tol * bref:
            return it, x
        z = prec(r)
        rzn = r @ z
        p = z + (rzn / rz) * p
        rz = rzn
    return maxit, x


@pytest.mark.parametrize("name,kw", [("sphere", dict(level=4)), ("torus", dict(nu=60, nv=40))])
def test_multigrid_beats_jacobi(name, kw):
    plan, K = problem(name, **kw)
    levels = multigrid.build_hierarchy(K, plan.mass_vert)
    rng = np.random.default_rng(2)
    for shift in (0.0, plan.time_eigs[1], plan.time_eigs[-1]):
        A = (K + shift * sp.diags(plan.mass_vert)).tocsr()
        dinv = 1.0 / A.diagonal()
        b = rng.standard_normal(plan.n_vertices)
        if shift == 0.0:
            b -= b.mean()
        it_mg, x = pcg_iterations(A, b, multigrid.CpuVcycle(levels, shift).cycle_fused, dinv)
        it_j, _ = pcg_iterations(A, b, lambda r: dinv * r, dinv)
        assert it_mg <= 40 and (it_mg * 3 <= it_j or it_j <= 40), (shift, it_mg, it_j)
        assert np.max(np.abs(A @ x - b)) < 1e-7 * np.max(np.abs(b))


# ---------------------------------------------------------------------------- what a converged solve cannot see
class WrongPostWeight(multigrid.CpuVcycle):
    """The plain cycle with post-smoothing weight 0.6 instead of 2/3: still symmetric positive enough for PCG, and wrong."""

    def cycle(self, b, l=0):
        if l == len(self.levels) - 1:
            return self.coarse_inv @ b
        A, dinv, lv = self.A[l], self.dinv[l], self.levels[l]
        x = self.omega * dinv * b
        x = x + lv.P @ self.cycle(lv.R @ (b - A @ x), l + 1)
        return x + 0.6 * dinv * (b - A @ x)


@pytest.mark.parametrize("shift", [0.0, 9.3])
def test_wrong_smoother_weight_hides_in_a_converged_solve(shift):
    """Why tests/test_hip_multigrid.py compares ONE cycle element by element: a V-cycle with a wrong coefficient is far outside
    that file's 1e-12 bound, yet a PCG preconditioned with it converges to the same solution and every converged-solve test
    passes."""
    plan, K = problem("torus", nu=24, nv=16)
    levels = multigrid.build_hierarchy(K, plan.mass_vert, coarsest=6)
    assert len(levels) == 3 and levels[0].n == 384
    right, wrong = multigrid.CpuVcycle(levels, shift), WrongPostWeight(levels, shift)
    b = np.random.default_rng(3).standard_normal(plan.n_vertices)
    if shift == 0.0:
        b -= b.mean()
    z, zw = right.cycle(b), wrong.cycle(b)
    assert np.max(np.abs(zw - z)) > 1e-3 * np.max(np.abs(z))
    A, dinv = right.A[0], right.dinv[0]
    it, x = pcg_iterations(A, b, right.cycle, dinv)
    itw, xw = pcg_iterations(A, b, wrong.cycle, dinv)
    assert it < 100 and itw < 100
    if shift == 0.0:
        x, xw = x - x.mean(), xw - xw.mean()
    assert np.max(np.abs(xw - x)) < 1e-7 * np.max(np.abs(x))


def test_setup_multigrid_keeps_the_levels_it_uploads():
    """DeviceProblem.setup_multigrid leaves on the instance the hierarchy it described to the library (plan numbering): the
    reference of the device V-cycle tests runs on these levels.  (The library call is replaced: no GPU here.)"""
    import ctypes

    from dots_socp_amd import _lib
    from dots_socp_amd.device import DeviceProblem

    plan, K = problem("torus", nu=24, nv=16)
    seen = {}

    class Library:
        @staticmethod
        def dots_mg_setup(handle, desc_ref):
            d = ctypes.cast(desc_ref, ctypes.POINTER(_lib.MgDesc)).contents
            seen["sizes"] = [d.levels[l].n for l in range(d.n_levels)]
            seen["p_val"] = [np.ctypeslib.as_array(d.levels[l].p_val, (d.levels[l].p_nnz,)).copy() for l in range(d.n_levels - 1)]
            seen["n_cols"] = d.n_cols
            return 0

    dev = DeviceProblem.__new__(DeviceProblem)
    dev.lib, dev._h, dev.plan, dev.lap_solver, dev.mode_slice = Library(), None, plan, "modal_pcg", None
    summary = dev.setup_multigrid(eps=1e-2, coarsest=6)
    fresh = multigrid.build_hierarchy(K, plan.mass_vert, coarsest=6)
    assert summary["sizes"] == seen["sizes"] == [lv.n for lv in fresh] == [lv.n for lv in dev.mg_levels] and seen["n_cols"] == plan.n_time + 1
    for kept, want, p_val in zip(dev.mg_levels, fresh, seen["p_val"] + [None]):
        for name in ("K", "M", "P", "R", "KP", "MP", "PP"):
            a, b = getattr(kept, name), getattr(want, name)
            assert (a is None) == (b is None)
            if a is not None:
                assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data)
        assert np.array_equal(kept.dK, want.dK) and np.array_equal(kept.dM, want.dM)
        if p_val is not None:
            assert np.array_equal(p_val, kept.P.data)
    dev._h = None      # (nothing to destroy)

"""CPU tests of tests/mode_checks.py: the mode-resolved check of step 1's solve, and the written proof of the gap it closes.

A defect planted in the high time modes of a plain fp64 solve PASSES the figure every existing test of the solve measures (white
right-hand side, max|got - want| / max|want| over the nodal array, 1e-9 up to 256 time nodes and 1e-10 above) and FAILS the per-mode
check by orders of magnitude (``test_mutations``).  The yardstick of the new tolerances -- the error of the plain fp64 solve against the
refined reference -- is measured, logged and held against what rounding alone explains (``test_yardstick``), and the host
factorisation with the numpy sweeps of frontal_cpu.py goes through the same check (``test_host_numeric_path``).

Of the five mutations of mode_checks.plain_solve three are kept as the proof (``KEPT``: each passes the old check and fails the new one
at the cases of ``GAP_CASES``); ``stale_shift`` and ``ground_all`` are dropped from it because the old check catches them already
(``DROPPED``, asserted too): they are not small in the low modes."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import frontal_cpu
import mode_checks as mc
from dots_socp_amd import frontal, geometry, meshes

LD = np.longdouble
ND_LEAF = 16
KEPT = ("offdiag_high", "inverse_row", "forward_col")
# Caught by the nodal figure already (it is owned by the low modes, and these two are not small there): stale_shift moves sigma by a
# whole step (old figure 4e-7 at T = 127, 5e-9 at T = 1023, eps = 1e-2), ground_all pins a vertex of mode 1 (old figure about 1).
DROPPED = ("stale_shift", "ground_all")
# Where each kept mutation passes the old check (measured once on sphere level 2; asserted below)
GAP_CASES = [(20, 1e-2, ("inverse_row", "forward_col")), (127, 0.0, KEPT), (127, 1e-2, KEPT), (1023, 1e-2, KEPT)]


@functools.lru_cache(maxsize=None)
def operator(T):
    plan = geometry.build_plan(T, meshes.example("sphere", level=2)[0], reorder="nd", nd_leaf=ND_LEAF)
    return (plan,) + mc.plan_operator(plan)


@functools.lru_cache(maxsize=None)
def case(T, eps):
    """The bands' right-hand sides and a white one (last), their references, the plain fp64 solves and p; read-only."""
    _, K, mass = operator(T)
    bands = mc.octaves(T + 1)
    b = np.stack([mc.band_rhs(T, mass.size, S, 100 + k, eps) for k, S in enumerate(bands)] + [mc.white_rhs(T, mass.size, 3, eps)])
    xr = mc.reference(K, mass, T, eps, b)
    x = mc.plain_solve(K, mass, T, eps, b)
    errs = [mc.mode_errors(x[k], xr[k], S, mass, eps) for k, S in enumerate(bands)]
    for a in (b, xr, x):
        a.setflags(write=False)
    return dict(bands=bands, b=b, xr=xr, x=x, errs=errs, p=max(float(e.max()) for e, _ in errs), kappa=mc.kappa(K, mass, T, eps),
                white=mc.inverse(T, xr[-1]))


def test_long_double_products_and_basis():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((37, 300)).astype(LD) * (LD(1) + LD(2) ** -60)
    B = rng.standard_normal((300, 23)) * np.exp(6.0 * rng.standard_normal((300, 23)))
    want = A @ B.astype(LD)
    assert np.max(np.abs(mc.ld_matmul(A, B) - want) / np.abs(want).max()) < 2.0 ** -60
    for T in (1, 6, 20, 127):
        Q, sigma = mc.basis(T)
        n = T + 1
        assert np.max(np.abs(mc.ld_matmul(Q.T, Q) - np.eye(n))) < 2.0 ** -58
        lt = np.zeros((n, n), dtype=LD)      # minus the Neumann second difference / h^2
        i = np.arange(n)
        lt[i, i] = 2
        lt[0, 0] = lt[-1, -1] = 1
        lt[i[:-1], i[:-1] + 1] = lt[i[:-1] + 1, i[:-1]] = -1
        assert np.max(np.abs(mc.ld_matmul(lt * LD(T) ** 2, Q) - Q * sigma[None, :])) < 2.0 ** -55 * float(sigma[-1])
        Q64, sigma64 = geometry.time_modes(T)
        assert np.max(np.abs(Q64 - Q)) < 4 * n * mc.U and np.max(np.abs(sigma64 - sigma)) < 16 * mc.U * T * T      # (values up to 4 T^2, a few roundings each)
    assert [s.tolist() for s in mc.octaves(6)] == [[0], [1], [2, 3], [4, 5]]
    assert len(mc.octaves(1024)) == 11 and mc.octaves(301)[-1][[0, -1]].tolist() == [256, 300]
    assert mc.last_chunk(301).sum() == 45 and mc.last_chunk(1024).sum() == 256 and mc.last_chunk(128).sum() == 32


@pytest.mark.parametrize("eps", [0.0, 1e-2])
@pytest.mark.parametrize("T", [6, 20, 127, 1023])
def test_yardstick(T, eps):
    """plain_solve against the reference, mode by mode: within what rounding explains (mode_checks.fp64_floor), the leak within the
    bound the device gets, and the reference itself converged (a fifth refinement step moves it by less than 2^-60).
    Measured worst per-mode error p (max-norm, sphere level 2): 3e-15 at T = 6 and 20 (3e-13 in mode 0 at eps = 1e-2, kappa = 3e4),
    4e-14 at T = 127, 1.7e-12 at T = 1023 (the fp64 sigma of the low modes: 2 - 2 cos loses 1 / sigma_a h^2)."""
    _, K, mass = operator(T)
    c = case(T, eps)
    worst = 0.0
    floors = mc.fp64_floor(K, mass, T, eps, c["bands"])
    for k, S in enumerate(c["bands"]):
        e, leak = c["errs"][k]
        floor = floors[k]
        assert np.all(e <= floor), (k, float((e / floor).max()))
        tol, tol_leak = mc.tolerances(c["p"], c["kappa"], S)
        mc.assert_modes(e, leak, tol, tol_leak, S, T + 1, "plain_solve")
        worst = max(worst, float((e / floor).max()))
    print(f"mode checks yardstick T {T} eps {eps:g}: p = {c['p']:.3e} (at most {worst:.2f} of the fp64 floor), kappa_0 {c['kappa'][0]:.2e}")
    # the old figure sees the plain solve as exact
    assert mc.nodal_rel(c["x"][-1], c["white"], mass, eps) < 1e-11
    if T <= 127:
        keep = mc.REFINE
        try:
            mc.REFINE = keep + 1
            more = mc.reference(K, mass, T, eps, c["b"][-1])
        finally:
            mc.REFINE = keep
        assert np.max(np.abs(more - c["xr"][-1])) <= 2.0 ** -60 * np.max(np.abs(more))


@pytest.mark.parametrize("T,eps,passing", GAP_CASES, ids=[f"T{T}-eps{eps:g}" for T, eps, _ in GAP_CASES])
def test_mutations(T, eps, passing):
    """(i) every mutation of ``passing`` PASSES the old check, (ii) FAILS the new one, by at least 100 x the bound (so neither the margin
    of 16 nor a margin raised within the rule of test_hip_mode_resolved.py hides it); the dropped mutations are the old check's."""
    _, K, mass = operator(T)
    c = case(T, eps)
    old_tol = mc.OLD_TOL[T + 1 > 256]
    for mutation in mc.MUTATIONS:
        x = mc.plain_solve(K, mass, T, eps, c["b"], mutation=mutation)
        old = mc.nodal_rel(x[-1], c["white"], mass, eps)
        ratio, failed = 0.0, 0
        for k, S in enumerate(c["bands"]):
            e, leak = mc.mode_errors(x[k], c["xr"][k], S, mass, eps)
            tol, tol_leak = mc.tolerances(c["p"], c["kappa"], S)
            ratio = max(ratio, float((e / tol).max()), leak / tol_leak)
            try:
                mc.assert_modes(e, leak, tol, tol_leak, S, T + 1, mutation)
            except AssertionError as err:
                failed += 1
                assert "chunk" in str(err) or "leak" in str(err)
        print(f"mode checks mutation {mutation} T {T} eps {eps:g}: old figure {old:.2e} (tolerance {old_tol:.0e}), new worst error / bound {ratio:.2e}, "
              f"{failed} of {len(c['bands'])} bands fail")
        assert failed > 0 and ratio > 1.0, mutation                   # the new check sees every mutation
        if mutation in passing:
            assert old < old_tol, (mutation, old)                     # the gap
            assert ratio >= 100.0, (mutation, ratio)
        if mutation in DROPPED:
            assert old > old_tol, (mutation, old)


@pytest.mark.parametrize("eps", [0.0, 1e-2])
@pytest.mark.parametrize("T", [20, 127])
def test_host_numeric_path(T, eps):
    """frontal.factorize(numeric=True) and the numpy sweeps of frontal_cpu.py (the plan's numbering, fp64 transforms) within the bound of
    the device's direct paths."""
    plan, K, mass = operator(T)
    c = case(T, eps)
    Kp = sp.csr_matrix((plan.lap_val, plan.lap_col, plan.lap_rowptr), shape=(plan.n_vertices,) * 2)
    ff = frontal.factorize(Kp, plan.mass_vert, plan.time_eigs + eps, plan.dissection, numeric=True)
    assert ff.grounded.tolist() == ([0] if eps == 0.0 else [])
    Q64 = geometry.time_modes(T)[0]
    perm = np.asarray(plan.perm_vert)
    worst = 0.0
    for k, S in enumerate(c["bands"]):
        xhat = frontal_cpu.solve(ff, (Q64.T @ c["b"][k][:, perm]).T)      # (V, modes)
        x = np.empty((T + 1, mass.size))
        x[:, perm] = Q64 @ xhat.T
        e, leak = mc.mode_errors(x, c["xr"][k], S, mass, eps)
        tol, tol_leak = mc.tolerances(c["p"], c["kappa"], S)
        mc.assert_modes(e, leak, tol, tol_leak, S, T + 1, "host factor and sweeps")
        worst = max(worst, float((e / tol).max()))
    print(f"mode checks host numeric path T {T} eps {eps:g}: worst error / bound {worst:.2e}")

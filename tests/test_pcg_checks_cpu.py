"""The host PCG of tests/pcg_checks.py against itself and the oracle, without a GPU: (a) unmutated and run to convergence it gives the
oracle's step_laplacian; (b) its own rounding spread on every GPU case of test_hip_pcg.py, which sets the bound of those tests;
(c) every deliberate defect moves phi or the iteration count far beyond that bound on the case meant to expose it -- so the cases
discriminate; (d) the conditions the GPU cases put on their inputs (freeze decisions away from their thresholds, frozen and live
columns at the cut, wheel rows beyond the staged capacity) hold on the reference."""
import numpy as np
import pytest

import pcg_checks as pc

MARGIN = 1e-6      # no freeze decision closer to its threshold than this, relative


def remove_gauge(phi, mass):
    w = np.broadcast_to(mass[None, :], phi.shape)
    return phi - np.sum(phi * w) / np.sum(w)


@pytest.mark.parametrize("eps", pc.EPS)
@pytest.mark.parametrize("solver", ["modal_pcg", "spacetime_pcg"])
@pytest.mark.parametrize("mesh", ["ops_ico1", "fan"])
def test_converged_host_pcg_is_the_oracles_solve(mesh, solver, eps):
    """(a)"""
    s = pc.seeded_oracle(7, pc.geometry_of(("fixture", dict(mesh=mesh))), eps, factorise=True)
    res = pc.host_pcg(pc.problem_of(s, solver), eps, 1e-12, 20000)
    s.step_laplacian()
    got, want = res.phi, s.phi
    if eps == 0.0:
        got, want = remove_gauge(got, s.mass_v), remove_gauge(want, s.mass_v)
    assert not res.not_converged and res.iterations > 0
    assert pc.rel_max(got, want) < 1e-9, res.iterations


def spread_of(p, eps, tol, cuts):
    """Largest relative distance between the float64 host PCG and the same PCG with every sum over vertices re-ordered (a seeded
    renumbering) and, where the problem is small, in np.longdouble; the float64 results."""
    a = pc.host_pcg(p, eps, tol, cuts)
    others = [pc.host_pcg_permuted(p, eps, tol, cuts)]
    if p.b.size < 50000:
        others.append(pc.host_pcg(p, eps, tol, cuts, dtype=np.longdouble))
    spread = 0.0
    for b in others:
        for c in cuts:
            assert (a[c].iterations, a[c].frozen.tolist()) == (b[c].iterations, b[c].frozen.tolist()), c
            assert abs(a[c].rel_residual - b[c].rel_residual) <= 1e-9 * a[c].rel_residual
            spread = max(spread, pc.rel_max(a[c].phi, b[c].phi))
    return spread, a


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_rounding_spread_and_bound(family):
    """(b) and (d): the spread of the reference alone per case, the family's bound = 100 x the recorded spread, below the ceiling."""
    worst = 0.0
    for case, spec in pc.CASES.items():
        if spec["family"] != family:
            continue
        for eps in pc.EPS:
            _, p = pc.case_problem(case, eps)
            spread, a = spread_of(p, eps, pc.ITERATE_TOL, pc.CUTS)
            print(f"pcg spread {case} eps {eps:g}: {spread:.2e}; iterations {[a[c].iterations for c in pc.CUTS]}, live at the cut "
                  f"{int((~a[pc.CUTS[-1]].frozen).sum())} of {a[pc.CUTS[-1]].frozen.size}, margin {a[pc.CUTS[-1]].margin:.1e}")
            assert a[pc.CUTS[-1]].margin > MARGIN, case
            worst = max(worst, spread)
    print(f"pcg family {family!r}: spread {worst:.2e}, recorded {pc.SPREAD[family]:.0e}, bound {pc.BOUND[family]:.0e}")
    assert worst <= pc.SPREAD[family]
    assert pc.BOUND[family] == 100.0 * pc.SPREAD[family] and pc.BOUND[family] <= pc.PHI_CEILING


@pytest.mark.parametrize("case", list(pc.FREEZE_CASES))
def test_freeze_cases(case):
    """(b), (d) for the freezing cases: a column frozen strictly before the cut, one live at it, every decision away from its threshold --
    at the cut and in the run to convergence."""
    tol, eps, cut = pc.FREEZE_CASES[case], pc.FREEZE_EPS, pc.CUTS[-1]
    _, p = pc.case_problem(case, eps)
    spread, a = spread_of(p, eps, tol, (cut, pc.CONVERGE))
    res, full = a[cut], a[pc.CONVERGE]
    print(f"pcg freeze {case} tol {tol:g}: spread {spread:.2e}, bound {pc.BOUND['freezing']:.0e}; frozen before the cut "
          f"{int((res.live_iterations < cut).sum())}, live at it {int((~res.frozen).sum())}, margin {min(res.margin, full.margin):.1e}, "
          f"iterations to convergence {full.iterations}")
    assert np.any(res.live_iterations < cut) and np.any(~res.frozen)
    assert min(res.margin, full.margin) > MARGIN
    assert not full.not_converged and cut < full.iterations < pc.CONVERGE and full.iterations == full.live_iterations.max()
    assert spread <= pc.SPREAD["freezing"] and pc.BOUND["freezing"] <= pc.PHI_CEILING


def test_solve_sequence_inputs():
    """(d) for the solves on one context: converged, every decision away from its threshold, and the steps of the sequence differ."""
    seen = []
    for eps, tol in pc.SEQUENCE:
        _, p = pc.case_problem(pc.SEQUENCE_CASE, eps)
        spread, a = spread_of(p, eps, tol, (pc.CONVERGE,))
        res = a[pc.CONVERGE]
        print(f"pcg sequence eps {eps:g} tol {tol:g}: spread {spread:.2e}, iterations {res.iterations}, margin {res.margin:.1e}")
        assert not res.not_converged and res.margin > MARGIN and spread <= pc.SPREAD["solve sequence"]
        seen.append(res)
    assert seen[0].iterations < seen[1].iterations
    assert min(pc.rel_max(seen[0].phi, seen[1].phi), pc.rel_max(seen[1].phi, seen[2].phi)) >= 100.0 * pc.BOUND["solve sequence"]


def plan_of(case):
    from dots_socp_amd.geometry import build_plan

    spec = pc.CASES[case]
    return build_plan(spec["T"], pc.geometry_of(spec["mesh"]), reorder=spec.get("reorder", True))


@pytest.mark.parametrize("case", [c for c, spec in pc.CASES.items() if spec["family"] == "wheel"])
def test_wheel_rows_exceed_the_staged_capacity(case):
    """(d) with the tiling the case must report, the hub's tile holds more entries than are staged; in the caller's numbering the hub is
    row 0, straddles the capacity and leaves the rest of its tile unstaged."""
    spec = pc.CASES[case]
    plan, vt, cap = plan_of(case), spec["path"]["vt"], spec["path"]["cap"]
    over, straddle = pc.overflowing_tiles(plan, vt, cap)
    print(f"pcg {case}: tiles beyond cap {over}, straddling {straddle}")
    assert over
    if not spec["reorder"]:
        assert over == [0] and straddle == [0] and vt > 1
        if spec["T"] == 255:      # the hub's own row straddles, the other rows of its tile are wholly unstaged
            assert plan.lap_rowptr[1] > cap


# mutation -> (case, eps, cg_tol, cg_max_iter) of the GPU case that is meant to expose it, and the family whose bound it must exceed
EXPOSED_BY = {
    "stale_parity": [("small-T7", 1e-2, pc.ITERATE_TOL, 16), ("spacetime-T20", 0.0, pc.ITERATE_TOL, 16), ("collapse256-T200", 0.0, pc.ITERATE_TOL, 8)],
    "beta_zero": [("small-T7", 1e-2, pc.ITERATE_TOL, 8), ("spacetime-T20", 0.0, pc.ITERATE_TOL, 8), ("wide-T127", 0.0, pc.ITERATE_TOL, 8)],
    "no_freeze": [(c, pc.FREEZE_EPS, tol, 16) for c, tol in pc.FREEZE_CASES.items()],
    "freeze_on_r2": [(c, pc.FREEZE_EPS, tol, 16) for c, tol in pc.FREEZE_CASES.items()],
    "no_mean_removal": [("small-T1", 0.0, pc.ITERATE_TOL, 8), ("wide-T100", 0.0, pc.ITERATE_TOL, 8), ("spacetime-T7", 0.0, pc.ITERATE_TOL, 8),
                        ("spacetime-wide-T383", 0.0, pc.ITERATE_TOL, 8)],
    "dinv_without_eps": [("small-T20", 1e-2, pc.ITERATE_TOL, 8), ("spacetime-T63", 1e-2, pc.ITERATE_TOL, 8)],
    "drop_unstaged": [(c, 1e-2, pc.ITERATE_TOL, 8) for c, spec in pc.CASES.items() if spec["family"] == "wheel"],
    "tol_not_refreshed": [(pc.SEQUENCE_CASE, pc.SEQUENCE[1][0], pc.SEQUENCE[1][1], pc.CONVERGE)],
}
assert set(EXPOSED_BY) == set(pc.MUTATIONS)


@pytest.mark.parametrize("mutation", pc.MUTATIONS)
def test_mutations_show(mutation):
    """(c) the defect moves phi by at least 100 bounds, or changes the iteration count, on every case listed for it."""
    for case, eps, tol, cut in EXPOSED_BY[mutation]:
        family = "freezing" if mutation in ("no_freeze", "freeze_on_r2") else "solve sequence" if mutation == "tol_not_refreshed" else pc.CASES[case]["family"]
        _, p = pc.case_problem(case, eps)
        kw = {}
        if mutation == "drop_unstaged":
            spec = pc.CASES[case]
            kw["dropped"], n = pc.unstaged_dropped(p.K, plan_of(case), spec["path"]["vt"], spec["path"]["cap"])
            assert n > 0
        if mutation == "tol_not_refreshed":
            kw["stale_tol"] = pc.SEQUENCE[0][1]
        good = pc.host_pcg(p, eps, tol, cut)
        bad = pc.host_pcg(p, eps, tol, cut, mutation=mutation, **kw)
        shift = pc.rel_max(bad.phi, good.phi)
        print(f"pcg mutation {mutation} on {case} eps {eps:g}: phi moves {shift:.2e} (bound {pc.BOUND[family]:.0e}), "
              f"iterations {good.iterations} -> {bad.iterations}")
        assert shift >= 100.0 * pc.BOUND[family] or bad.iterations != good.iterations, (case, shift)
        if mutation not in ("no_freeze", "freeze_on_r2"):      # (those two may also show in the count alone)
            assert shift >= 100.0 * pc.BOUND[family], (case, shift)

"""GPU: the Jacobi PCG of kernels_cg.hip against the fp64 host PCG of tests/pcg_checks.py, ITERATE BY ITERATE, through DeviceProblem.

The converged solves of the other files cannot see a wrong iteration: PCG still converges with a stale r.z total, a beta of 0, a
preconditioner without eps, or columns frozen late, and a fault only costs iterations.  Here a solve is cut after 8 and after 16
iterations (cg_max_iter; the device runs units of 8) and the raw phi, the iteration count, the relative residual and the
not-converged mark are compared with the host PCG, which restates the start (warm start, unweighted mean removal when eps = 0), the
stopping rule crit <= tol^2 bref, the freezing of converged columns and the counting of FLAG_ITERS.  Every case first asserts the
launch path the launcher reports (dots_debug_counter 13 through DeviceProblem.cg_path: bits, vertices per tile, staged capacity,
workgroups, as literal numbers in pcg_checks.CASES), so a change of the launcher's thresholds fails the case instead of moving it
onto other kernels.  Covered: both branches of emit_partial / column_total (pitch <= 64 shuffles, above LDS), the collapse of more
than 1024 partial rows with 256-thread and with 1024-thread workgroups, CSR rows beyond the staged capacity (the wheel meshes: the
hub's row straddles it), the mean removal of the singular mode, freezing, and the capture cache across changes of cg_tol and eps.
The densities of these cases have unequal mass so that the right-hand side has a mean to remove.  The host PCG runs on the CSR and
the masses of the plan the device is handed (pcg_checks.with_plan_operator), its right-hand side is the oracle's.

Bounds.  phi: max|phi - phi_host| / max|phi_host| below 100 x the rounding spread of the host PCG alone (float64 against the same
PCG with every sum over vertices re-ordered and, on the small cases, in np.longdouble), per case family; the spreads are measured
and asserted by test_pcg_checks_cpu.py, which also shows that every deliberate defect of pcg_checks.MUTATIONS moves phi by more
than 100 bounds on its case:

    family                 spread measured   recorded   bound
    small pitches          9.1e-15           1e-14      1e-12
    wide pitches           1.8e-14           2e-14      2e-12
    collapse 256           6.7e-15           1e-14      1e-12
    collapse 128           1.3e-14           2e-14      2e-12
    space-time             2.6e-14           5e-14      5e-12
    space-time collapse    4.0e-14           1e-13      1e-11
    space-time wide        1.9e-14           5e-14      5e-12
    wheel                  1.8e-14           5e-14      5e-12
    freezing               7.8e-14           1e-13      1e-11
    solve sequence         5.1e-13           1e-12      1e-10

All are below the ceiling of 1e-9 (PHI_TOL of step_checks.py), so no case is cut at 8 iterations only.  The iteration count is
compared exactly, the relative residual to 1e-9 relative.  The operator alone is compared at FP_TOL = 1e-12.
"""
import functools

import numpy as np
import pytest

import pcg_checks as pc
from step_checks import FP_TOL

pytestmark = pytest.mark.gpu

RESIDUAL_TOL = 1e-9


def open_case(case, eps, cg_tol, cg_max_iter, solver=None):
    from dots_socp_amd.device import DeviceProblem

    spec = pc.CASES[case]
    s, p = pc.case_problem(case, eps) if solver is None else pc.seeded_problem(mesh_key(case), spec["T"], solver, eps)
    dev = DeviceProblem(spec["T"], pc.geometry_of(spec["mesh"]), lap_solver=solver or spec["solver"], reorder=spec.get("reorder", True))
    pc.upload_state(dev, s, cg_tol, cg_max_iter)
    return s, p, dev


def mesh_key(case):
    name, kw = pc.CASES[case]["mesh"]
    return name, tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def plan_of(case):
    """The plan the case's contexts are built on (build_plan is deterministic): the host PCG runs on the CSR the device is handed."""
    from dots_socp_amd.geometry import build_plan

    spec = pc.CASES[case]
    return build_plan(spec["T"], pc.geometry_of(spec["mesh"]), reorder=spec.get("reorder", True))


def assert_path(dev, case, modal=None):
    """The launcher's record against the case's literal one; ``modal=False``: the same mesh and T under the coupled operator."""
    want = pc.CASES[case]["path"]
    bits = want["bits"] - {"modal"} if modal is False else want["bits"]
    names, vt, cap, G = dev.cg_path()
    assert (names, vt, cap, G) == (bits, want["vt"], want["cap"], want["G"]), (case, sorted(names), vt, cap, G)
    return vt, cap


@functools.lru_cache(maxsize=None)
def host(case, eps, tol, cuts):
    """The host PCG of a case, computed once and then read-only: ``{cg_max_iter: Result}``."""
    _, p = pc.case_problem(case, eps)
    out = pc.host_pcg(pc.with_plan_operator(p, plan_of(case)), eps, tol, cuts)
    for res in out.values():
        res.phi.setflags(write=False)
    return out


def solve(dev, s):
    """One step-1 solve from the seeded phi: ``(phi, stats)``."""
    dev.upload("phi", s.phi)
    st = dev.run_phase("laplacian")
    return dev.download("phi"), st


def compare(tag, family, phi, st, want):
    err = pc.rel_max(phi, want.phi)
    res_err = abs(st.cg_last_rel_residual - want.rel_residual) / want.rel_residual
    print(f"pcg {tag} [{family}]: phi error {err:.3e} (bound {pc.BOUND[family]:.0e}), iterations {st.cg_last_iterations} (host "
          f"{want.iterations}), residual {st.cg_last_rel_residual:.6e} (host {want.rel_residual:.6e}, off {res_err:.1e}), not converged "
          f"{st.cg_not_converged} (host {int(want.not_converged)})")
    assert st.cg_last_iterations == want.iterations, tag
    assert st.cg_not_converged == int(want.not_converged), tag
    assert res_err <= RESIDUAL_TOL, tag
    assert err < pc.BOUND[family], tag


@pytest.mark.parametrize("eps", pc.EPS)
@pytest.mark.parametrize("case", list(pc.CASES))
def test_iterates_match_host_pcg(case, eps):
    """phi, count, residual and the not-converged mark after cg_max_iter = 8 and 16, on the launch path the case is about."""
    spec = pc.CASES[case]
    s, _, dev = open_case(case, eps, pc.ITERATE_TOL, pc.CUTS[0])
    want = host(case, eps, pc.ITERATE_TOL, pc.CUTS)
    assert dev.cg_path() == (set(), 0, 0, 0)      # nothing launched yet
    got = []
    for cut in pc.CUTS:
        dev.set_params(cg_max_iter=cut)
        got.append(solve(dev, s))
        vt, cap = assert_path(dev, case)
    if spec["family"] == "wheel":      # the hub's tile holds more CSR entries than are staged, and a row straddles the capacity
        over, straddle = pc.overflowing_tiles(dev.plan, vt, cap)
        assert over and straddle, (case, vt, cap)
        if not spec["reorder"]:
            assert over == [0]
    dev.close()
    for cut, (phi, st) in zip(pc.CUTS, got):
        compare(f"{case} eps {eps:g} cut {cut}", spec["family"], phi, st, want[cut])


OPERATOR_CASES = ["wheel200-spacetime-hub0", "wheel200-spacetime-reordered", "wheel1500-modal-hub0", "wheel1500-modal-reordered",
                  "collapse256-T255", "collapse128-T127", "spacetime-wide-T1023"]


@pytest.mark.parametrize("eps", pc.EPS)
@pytest.mark.parametrize("case", OPERATOR_CASES)
def test_coupled_operator_alone(case, eps):
    """K x of the coupled space-time operator (cg_apply_operator: k_cg_apply without the direction update) against the sparse host
    operator, on the meshes of the wheel, both collapse paths and pitch 1024."""
    from dots_socp_amd.device import DeviceProblem

    spec = pc.CASES[case]
    _, p = pc.seeded_problem(mesh_key(case), spec["T"], "spacetime_pcg", eps)
    dev = DeviceProblem(spec["T"], pc.geometry_of(spec["mesh"]), lap_solver="spacetime_pcg", reorder=spec.get("reorder", True))
    dev.set_params(eps=eps)
    x = np.random.default_rng(spec["T"]).standard_normal(p.b.shape)
    y = dev.apply_operator("laplacian_apply", x)
    vt, cap = assert_path(dev, case, modal=False)
    if spec["family"] == "wheel":
        assert pc.overflowing_tiles(dev.plan, vt, cap)[1]
    dev.close()
    err = pc.rel_max(y, pc.apply_operator(pc.with_plan_operator(p, plan_of(case)), x, eps))
    print(f"pcg operator {case} eps {eps:g}: error {err:.3e}")
    assert err < FP_TOL


@pytest.mark.parametrize("case", list(pc.FREEZE_CASES))
def test_freezing(case):
    """Columns that converge before the cut freeze where the host's do: phi (a column frozen late or early moves it, see
    test_pcg_checks_cpu.py::test_mutations_show) and the count at cg_max_iter = 16, and the count of the run to convergence."""
    tol, eps, cut = pc.FREEZE_CASES[case], pc.FREEZE_EPS, pc.CUTS[-1]
    s, _, dev = open_case(case, eps, tol, cut)
    want = host(case, eps, tol, (cut, pc.CONVERGE))
    assert np.any(want[cut].live_iterations < cut) and want[cut].not_converged
    phi, st = solve(dev, s)
    assert_path(dev, case)
    dev.set_params(cg_max_iter=pc.CONVERGE)
    phi_full, st_full = solve(dev, s)
    dev.close()
    compare(f"{case} freezing cut {cut}", "freezing", phi, st, want[cut])
    compare(f"{case} freezing converged", "freezing", phi_full, st_full, want[pc.CONVERGE])


def test_several_solves_on_one_context():
    """Two solves of one state are bit-identical although the second sizes its first burst from the first's count; a changed cg_tol
    and then a changed eps take effect in the captured graph: each solve matches the host at the new values."""
    case = pc.SEQUENCE_CASE
    (eps0, tol0) = pc.SEQUENCE[0]
    s, _, dev = open_case(case, eps0, tol0, pc.CONVERGE)
    phi1, st1 = solve(dev, s)
    phi2, st2 = solve(dev, s)
    assert_path(dev, case)
    assert st1.cg_last_iterations > 2 * pc.UNIT      # the second solve starts with a longer burst
    assert np.array_equal(phi1, phi2) and st1.cg_last_iterations == st2.cg_last_iterations
    assert st1.cg_last_rel_residual == st2.cg_last_rel_residual
    compare(f"{case} sequence eps {eps0:g} tol {tol0:g}", "solve sequence", phi1, st1, host(case, eps0, tol0, (pc.CONVERGE,))[pc.CONVERGE])
    for eps, tol in pc.SEQUENCE[1:]:
        s, _ = pc.case_problem(case, eps)      # (the same seeded state; the oracle's right-hand side at the new eps)
        dev.set_params(eps=eps, cg_tol=tol)
        phi, st = solve(dev, s)
        compare(f"{case} sequence eps {eps:g} tol {tol:g}", "solve sequence", phi, st, host(case, eps, tol, (pc.CONVERGE,))[pc.CONVERGE])
    dev.close()


def test_modal_pcg_refuses_more_than_256_modes():
    """A modal context of T + 1 > 256 without a factor keeps answering with the existing error."""
    from dots_socp_amd import _lib
    from dots_socp_amd.device import DeviceProblem

    dev = DeviceProblem(256, pc.geometry_of(pc.SPHERE2), lap_solver="modal_pcg")
    with pytest.raises(_lib.HipLibraryError) as e:
        dev.run_phase("laplacian")
    assert e.value.status == _lib.ERR_STATE
    assert "T + 1 > 256 needs the direct solver (dots_front_setup); the modal PCG takes T + 1 <= 256" in str(e.value)
    assert dev.cg_path() == (set(), 0, 0, 0)
    dev.close()

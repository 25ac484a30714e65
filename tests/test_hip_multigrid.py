"""GPU: ONE multigrid V-cycle on the device (kernels_mg.hip through dots_mg_apply) against the plain recursive fp64 host cycle
(multigrid.CpuVcycle.cycle) on exactly the hierarchy that was uploaded, element by element, on every launch path.

The converged-solve tests cannot see a wrong V-cycle: PCG converges with any symmetric positive preconditioner, a fault only costs
iterations (tests/test_multigrid_cpu.py::test_wrong_smoother_weight_hides_in_a_converged_solve).  Here every case is pinned to its
kernels by the path mask of the launcher (dots_debug_counter 11): a change of the launcher's thresholds moves the mask and fails
the case instead of silently moving it onto other kernels.

Case F reaches the collapse of more than 1024 partial rows (V > 4096 at pitch 256): the fine-level kernels of the cycle run with the
256-thread tiling of the large problems and k_collapse sums the r.z rows, which the PCG's own path record (dots_debug_counter 13)
must show.  Time-slab contexts are refused by dots_mg_apply.

Bounds.  z: max|z - z_ref| / max|z_ref| < 1e-12 per mode (FP_TOL of test_hip_phases; the plain and the fused host cycle, two
orderings of the same arithmetic, differ by 2e-16 to 3e-16).  rz: |rz - sum r z_ref| < 1e-12 sum |r_i z_i| per mode.
"""
import functools

import numpy as np
import pytest

from conftest import load_oracle

pytestmark = pytest.mark.gpu

O = load_oracle()
TOL = 1e-12

# mesh, coarsest of build_hierarchy, T values, launches a cycle must report at pitch <= 128 / at pitch 256, levels inside the tail launch
CASES = {
    # 384, 74, 6 rows: both coarse levels inside the tail
    "A": dict(mesh=("torus", dict(nu=24, nv=16)), coarsest=6, T=(7, 20, 63, 127, 255), tail_levels=2,
              narrow={"restrict_rows", "tail"}, wide={"restrict_flat", "tail"}),
    # 384, 74 rows: a lone coarsest level above 64 rows is solved outside the tail
    "B": dict(mesh=("torus", dict(nu=24, nv=16)), coarsest=96, T=(7, 127, 255), tail_levels=0,
              narrow={"restrict_rows", "coarse_rows"}, wide={"restrict_flat", "coarse_flat"}),
    # 642, 42 rows in the caller's numbering (the device's reordering aggregates 79 rows, too many for the tail): the tail is the
    # dense solve alone
    "C": dict(mesh=("sphere", dict(level=3)), coarsest=70, reorder=False, T=(7, 63), tail_levels=1,
              narrow={"restrict_rows", "tail"}, wide=None),
    # 240, 38 rows under the default reordering: the same lone dense solve inside the tail behind a non-trivial vertex permutation
    "E": dict(mesh=("torus", dict(nu=20, nv=12)), coarsest=70, T=(7, 63), tail_levels=1,
              narrow={"restrict_rows", "tail"}, wide=None),
    # 2400, 400, 44, 9 rows: level 1 sits between the finest level and the tail
    "D": dict(mesh=("knot", dict(nu=240, nv=10)), coarsest=12, T=(15, 127, 255), tail_levels=2,
              narrow={"restrict_rows", "tail", "post", "down_above0"}, wide={"restrict_flat", "tail", "post", "down_above0"}),
    # 4176, 976, 101 rows with the default coarsest (a lone coarsest level above 64 rows, level 1 between it and the finest): more than
    # 1024 workgroups at pitch 256, so the finest level runs with one vertex per 256-thread workgroup and the r.z rows are collapsed
    # behind the cycle
    "F": dict(mesh=("torus", dict(nu=72, nv=58)), coarsest=256, T=(255,), tail_levels=0,
              narrow=None, wide={"restrict_flat", "coarse_flat", "post", "down_above0"},
              cg_path=({"modal", "collapse", "small_wg", "mg"}, 1, 76, 4176)),
}
CASE_T = [(c, T) for c, spec in CASES.items() for T in spec["T"]]


@functools.lru_cache(maxsize=None)
def geometry_of(case):
    from dots_socp_amd import meshes

    name, kw = CASES[case]["mesh"]
    return meshes.example(name, **kw)[0]


def open_problem(case, T, eps, lap_solver="modal_pcg", multigrid=True):
    from dots_socp_amd.device import DeviceProblem

    dev = DeviceProblem(T, geometry_of(case), lap_solver=lap_solver, reorder=CASES[case].get("reorder", True))
    dev.set_params(eps=eps)
    if multigrid:
        assert dev.setup_multigrid(eps=eps, coarsest=CASES[case]["coarsest"]) is not None
    return dev


def perm_of(dev):
    p = dev.plan.perm_vert      # None: case C, the one context opened without reordering
    return np.arange(dev.V) if p is None else np.asarray(p)


def residual(case, T, eps, V):
    r = np.random.default_rng(1000 + T).standard_normal((T + 1, V))
    if eps == 0.0:
        r[0] -= r[0].mean()      # mode 0 is singular: its right-hand side is orthogonal to the constant
    return r


_REFERENCE = {}


def reference(dev, case, T, eps):
    """r, z_ref = CpuVcycle.cycle(r) per mode, the entry value D^-1 r, all in the caller's vertex numbering; computed once per
    (case, T, eps) on the levels the device holds (every context of one case and T builds the same plan) and then read-only."""
    key = (case, T, eps)
    if key not in _REFERENCE:
        from dots_socp_amd import multigrid

        perm, levels = perm_of(dev), dev.mg_levels
        r = residual(case, T, eps, dev.V)
        z, jac = np.empty_like(r), np.empty_like(r)
        for a, sigma in enumerate(dev.plan.time_eigs):
            vc = multigrid.CpuVcycle(levels, float(sigma + eps))
            z[a, perm] = vc.cycle(r[a, perm])
            jac[a, perm] = r[a, perm] * vc.dinv[0]
        for x in (r, z, jac):
            x.setflags(write=False)
        _REFERENCE[key] = (r, z, jac)
    return _REFERENCE[key]


def assert_path(dev, case, T):
    spec = CASES[case]
    names, tail_levels = dev.mg_path()
    want = spec["narrow"] if T + 1 <= 128 else spec["wide"]
    assert names == want and tail_levels == spec["tail_levels"], (case, T, dev.mg_summary["sizes"], sorted(names), tail_levels)
    # the tiling of the PCG kernels around the cycle: only case F is large enough for the collapse
    cg = dev.cg_path()
    if "cg_path" in spec:
        assert cg == spec["cg_path"], (case, T, cg)
    else:
        assert "modal" in cg[0] and not cg[0] & {"collapse", "small_wg"}, (case, T, cg)


@pytest.mark.parametrize("eps", [0.0, 1e-2])
@pytest.mark.parametrize("case,T", CASE_T)
def test_vcycle_matches_host_cycle(case, T, eps):
    """(a) z and (b) r.z of one device V-cycle against the plain host cycle, with the launches the case is about."""
    dev = open_problem(case, T, eps)
    r, z_ref, _ = reference(dev, case, T, eps)
    z, rz = dev.mg_apply(r)
    assert_path(dev, case, T)
    dev.close()
    ez = np.max(np.abs(z - z_ref), axis=1) / np.max(np.abs(z_ref), axis=1)
    erz = np.abs(rz - np.sum(r * z_ref, axis=1)) / np.sum(np.abs(r * z_ref), axis=1)
    print(f"mg_apply case {case} T {T} eps {eps}: max rel z error {ez.max():.3e}, max rel rz error {erz.max():.3e}")
    assert ez.max() < TOL, (int(np.argmax(ez)), ez.max())
    assert erz.max() < TOL, (int(np.argmax(erz)), erz.max())


@pytest.mark.parametrize("case,T", [("A", 20), ("D", 127)])
def test_frozen_modes_are_skipped(case, T):
    """(c) a frozen mode keeps its entry value D^-1 r bit for bit; the live ones do not notice."""
    eps = 1e-2
    dev = open_problem(case, T, eps)
    r, _, jac = reference(dev, case, T, eps)
    frozen = np.zeros(T + 1, dtype=bool)
    frozen[[0, (T + 1) // 2, T]] = True
    z_all, rz_all = dev.mg_apply(r)
    z, rz = dev.mg_apply(r, frozen=frozen)
    assert_path(dev, case, T)
    dev.close()
    assert np.array_equal(z[frozen], jac[frozen])
    assert np.array_equal(z[~frozen], z_all[~frozen]) and np.array_equal(rz[~frozen], rz_all[~frozen])
    assert not np.array_equal(z_all[frozen], jac[frozen])


def test_apply_leaves_no_trace_in_the_next_solve():
    """(d) the PCG buffers dots_mg_apply uses are scratch between solves: a solve after it is the solve without it, bit for bit."""
    from test_hip_phases import make_pair

    case, T, eps = "A", 7, 1e-2      # (the oracle of make_pair factorises every mode: no singular one)
    g = dict(geometry_of(case), n_time=T)
    s, dev = make_pair(g, lap_solver="modal_pcg", eps=eps)
    assert dev.setup_multigrid(eps=eps, coarsest=CASES[case]["coarsest"]) is not None
    phi0 = s.phi.copy()
    st = dev.run_phase("laplacian")
    phi1, it1 = dev.download("phi"), st.cg_last_iterations
    dev.upload("phi", phi0)
    frozen = np.arange(T + 1) % 3 == 1
    dev.mg_apply(residual(case, T, eps, dev.V), frozen=frozen)
    st = dev.run_phase("laplacian")
    phi2, it2 = dev.download("phi"), st.cg_last_iterations
    dev.close()
    assert it1 > 0 and it2 == it1 and st.cg_not_converged == 0
    assert np.array_equal(phi1, phi2)


@pytest.mark.parametrize("case,T", [("A", 20), ("D", 255)])
def test_apply_is_deterministic(case, T):
    """(e) fixed reduction orders: the same input gives the same bits."""
    eps = 0.0
    dev = open_problem(case, T, eps)
    r = residual(case, T, eps, dev.V)
    z1, rz1 = dev.mg_apply(r)
    z2, rz2 = dev.mg_apply(r)
    dev.close()
    assert np.array_equal(z1, z2) and np.array_equal(rz1, rz2)


def test_path_mask_belongs_to_the_installed_hierarchy():
    """The mask names the last cycle of the hierarchy in use: empty before the first cycle, after a new dots_mg_setup and after the
    switch to Jacobi; dots_mg_apply runs the installed cycle also while the PCG is switched to Jacobi."""
    case, T, eps = "A", 7, 1e-2
    dev = open_problem(case, T, eps)
    r = residual(case, T, eps, dev.V)
    assert dev.mg_path() == (set(), 0)
    z1, _ = dev.mg_apply(r)
    assert_path(dev, case, T)
    assert dev.setup_multigrid(eps=eps, coarsest=CASES[case]["coarsest"]) is not None
    assert dev.mg_path() == (set(), 0)
    dev.mg_apply(r)
    dev.enable_multigrid(False)
    assert dev.mg_path() == (set(), 0)
    z2, _ = dev.mg_apply(r)
    assert_path(dev, case, T)
    dev.close()
    assert np.array_equal(z1, z2)


def test_refusals():
    """(f) contexts without a V-cycle answer DOTS_ERR_STATE with a message; wrong shapes never reach the library."""
    from dots_socp_amd import _lib
    from dots_socp_amd.device import DeviceProblem

    case, T = "A", 7
    r = residual(case, T, 1e-2, geometry_of(case)["vertices"].shape[0])
    for lap_solver in ("spacetime_pcg", "modal_pcg"):      # the wrong solver; the right one before setup_multigrid
        dev = open_problem(case, T, 1e-2, lap_solver=lap_solver, multigrid=False)
        with pytest.raises(_lib.HipLibraryError) as e:
            dev.mg_apply(r)
        assert e.value.status == _lib.ERR_STATE and "mg_apply" in str(e.value)
        dev.close()
    slab = DeviceProblem(T, geometry_of(case), lap_solver="modal_pcg", time_slab=(0, 2))      # one rank of two, alone on this GPU
    assert slab.setup_multigrid(eps=1e-2, coarsest=CASES[case]["coarsest"]) is not None
    with pytest.raises(_lib.HipLibraryError) as e:
        slab.mg_apply(r)
    assert e.value.status == _lib.ERR_STATE and "slab" in str(e.value)
    slab.close()
    dev = open_problem(case, T, 1e-2)
    with pytest.raises(ValueError):
        dev.mg_apply(r[:-1])
    with pytest.raises(ValueError):
        dev.mg_apply(r[:, :-1])
    with pytest.raises(ValueError):
        dev.mg_apply(r, frozen=np.zeros(T))
    dev.close()


def test_iteration_count_matches_host_pcg():
    """(g) the cycle inside the PCG around it: the device's iteration count against the same PCG on the host, per mode, with
    CpuVcycle.cycle as the preconditioner and the device's stopping rule r^T D^-1 r <= tol^2 b^T D^-1 b.

    The host's right-hand side in mode space is Q^T applied to the oracle's step_laplacian right-hand side for the state that
    was uploaded (phi = 0), with the sign of the device's operator K = -Laplacian + eps M (the sign and the vertex numbering do
    not change an iteration count).  The device steps in units of two iterations."""
    from dots_socp_amd import multigrid
    from test_multigrid_cpu import pcg_iterations
    from test_hip_phases import make_pair

    case, T, eps, tol = "A", 7, 1e-2, 1e-10
    g = dict(geometry_of(case), n_time=T)
    s, dev = make_pair(g, lap_solver="modal_pcg", eps=eps)
    s.phi[:] = 0.0
    dev.upload("phi", s.phi)
    dev.set_params(cg_tol=tol)
    assert dev.setup_multigrid(eps=eps, coarsest=CASES[case]["coarsest"]) is not None
    st = dev.run_phase("laplacian")
    device_iters = int(st.cg_last_iterations)
    perm, levels, plan = perm_of(dev), dev.mg_levels, dev.plan
    dev.close()
    assert st.cg_not_converged == 0
    b_modes = -(plan.time_modes.T @ s.laplacian_rhs())[:, perm]
    host = []
    for a, sigma in enumerate(plan.time_eigs):
        vc = multigrid.CpuVcycle(levels, float(sigma + eps))
        host.append(pcg_iterations(vc.A[0], b_modes[a], vc.cycle, vc.dinv[0], tol=tol)[0])
    even = max(host) + (max(host) & 1)
    print(f"pcg iterations: device {device_iters}, host per mode {host} (max {max(host)})")
    assert device_iters in (even, even + 2), (device_iters, host)

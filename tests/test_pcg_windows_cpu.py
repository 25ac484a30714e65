"""The windowed modal PCG (dots_pcg_windows) without a GPU: the entry point is declared, exported and bound; the window plan; what
check_time_nodes lets through with and without the switch; and the two bounds of test_hip_pcg_windows.py, measured here on the host
references alone and asserted to stay under the values recorded in pcg_window_checks.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import pcg_checks as pc
import pcg_window_checks as pw
from dots_socp_amd import _lib
from dots_socp_amd.device import pcg_window_plan
from dots_socp_amd.socp.solver_socp import check_time_nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-6      # no freeze decision closer to its threshold than this, relative (test_pcg_checks_cpu.py)


def test_entry_point_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dots_socp_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"^int dots_pcg_windows\(dots_ctx \*ctx, int on\);", header, re.M)
    assert re.search(r"#define\s+DOTS_ABI_VERSION\s+7\b", header) and _lib.ABI_VERSION == 7
    assert "dots_pcg_windows" in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        from dots_socp_amd import build

        build.build(verbose=False)
    assert ctypes.CDLL(_lib.LIB_PATH).dots_pcg_windows is not None      # (AttributeError: the library does not export it)
    lib = _lib.load()
    assert lib.dots_pcg_windows.argtypes is not None and lib.dots_abi_version() == 7


def test_window_plan():
    assert pcg_window_plan(255) == [(0, 256)]
    assert pcg_window_plan(256) == [(0, 256), (256, 1)]
    assert pcg_window_plan(300) == [(0, 256), (256, 45)]
    assert pcg_window_plan(511) == [(0, 256), (256, 256)]
    assert pcg_window_plan(600) == [(0, 256), (256, 256), (512, 89)]      # pitch 1024: the fourth window has no live mode
    assert pcg_window_plan(1023) == [(0, 256), (256, 256), (512, 256), (768, 256)]
    with pytest.raises(ValueError, match="1024"):
        pcg_window_plan(1024)
    for T, n in pw.WINDOWS.items():
        plan = pcg_window_plan(T)
        assert len(plan) == n and sum(live for _, live in plan) == T + 1


def test_check_time_nodes():
    for T in (300, 1023):
        for solver in ("modal_pcg", "modal_direct"):
            check_time_nodes(T, solver, pcg_windows=True)
        with pytest.raises(ValueError) as e:
            check_time_nodes(T, "modal_pcg")
        assert str(e.value) == f"lap_solver='modal_pcg' needs n_time + 1 <= 256 (got {T + 1}); use lap_solver='modal_direct'"
        with pytest.raises(ValueError, match="time slab"):
            check_time_nodes(T, "modal_pcg", time_slab=(0, 2), pcg_windows=True)
    with pytest.raises(ValueError, match="time slab"):
        check_time_nodes(63, "modal_pcg", time_slab=(0, 2), pcg_windows=True)
    for flag in (False, True):
        with pytest.raises(ValueError, match="at most 1024"):
            check_time_nodes(1024, "modal_pcg", pcg_windows=flag)
    check_time_nodes(255, "modal_pcg", pcg_windows=True)      # one window: the switch changes nothing


def test_batches_and_cascades_refuse_the_switch():
    import importlib

    ss = importlib.import_module("dots_socp_amd.socp.solver_socp")

    geom = pc.geometry_of(pw.MESH)
    calls = {
        "solver_socp_many": lambda: ss.solver_socp_many(300, geom, [dict()], pcg_windows=True),
        "solver_socp_cascade": lambda: ss.solver_socp_cascade(300, geom, pcg_windows=True),
        "solver_socp_mesh_cascade": lambda: ss.solver_socp_mesh_cascade(300, [geom, geom], pcg_windows=True),
        "solver_socp_spacetime_cascade": lambda: ss.solver_socp_spacetime_cascade(300, [geom, geom], pcg_windows=True),
        "solver_socp_auto_cascade": lambda: ss.solver_socp_auto_cascade(300, geom, pcg_windows=True),
    }
    for who, call in calls.items():
        with pytest.raises(ValueError, match="pcg_windows belongs to solver_socp") as e:
            call()
        assert who in str(e.value)


@pytest.mark.parametrize("mesh,T", pw.ITERATE_CASES, ids=[f"{m[0]}-T{T}" for m, T in pw.ITERATE_CASES])
def test_rounding_spread_and_bound(mesh, T):
    """The spread of the host PCG alone on the iterate cases: float64 against np.longdouble and against a renumbering of the vertices,
    both cuts, both eps; the device bound is 100 x the recorded spread, below the ceiling."""
    for eps in pc.EPS:
        _, p = pw.problem(mesh, T, eps)
        a = pc.host_pcg(p, eps, pc.ITERATE_TOL, pc.CUTS)
        spread = 0.0
        for b in (pc.host_pcg(p, eps, pc.ITERATE_TOL, pc.CUTS, dtype=np.longdouble), pc.host_pcg_permuted(p, eps, pc.ITERATE_TOL, pc.CUTS)):
            for c in pc.CUTS:
                assert (a[c].iterations, a[c].frozen.tolist()) == (b[c].iterations, b[c].frozen.tolist()), c
                assert abs(a[c].rel_residual - b[c].rel_residual) <= 1e-9 * a[c].rel_residual
                spread = max(spread, pc.rel_max(a[c].phi, b[c].phi))
        last = a[pc.CUTS[-1]]
        print(f"pcg windows spread {mesh[0]} T {T} eps {eps:g}: {spread:.2e} (recorded {pw.SPREAD['windows']:.0e}); iterations "
              f"{[a[c].iterations for c in pc.CUTS]}, live at the cut {int((~last.frozen).sum())} of {last.frozen.size}, margin {last.margin:.1e}")
        # the host's single loop and the windows' own loops stop together: a column of window 0 is live at every cut
        assert [a[c].iterations for c in pc.CUTS] == list(pc.CUTS) and np.any(~last.frozen[:256]) and last.margin > MARGIN
        assert spread <= pw.SPREAD["windows"]
    assert pw.BOUND["windows"] == 100.0 * pw.SPREAD["windows"] and pw.BOUND["windows"] <= pc.PHI_CEILING


@pytest.mark.parametrize("T", pw.HORIZONS)
def test_converged_error_and_bound(T):
    """What cg_tol = 1e-12 leaves: the host Jacobi PCG run to convergence against the oracle's per-mode SuperLU."""
    for eps in pc.EPS:
        s, p, want = pw.converged_case(T, eps)
        res = pc.host_pcg(p, eps, pw.CONVERGED_TOL, pc.CONVERGE)
        got = pw.remove_gauge(res.phi, s.mass_v) if eps == 0.0 else res.phi
        err = pc.rel_max(got, want)
        print(f"pcg windows converged T {T} eps {eps:g}: host PCG against SuperLU {err:.2e} (recorded {pw.CONVERGED_MEASURED:.0e}), "
              f"{res.iterations} iterations")
        assert not res.not_converged and 0 < res.iterations < pc.CONVERGE
        assert err <= pw.CONVERGED_MEASURED
    assert pw.CONVERGED_BOUND == 10.0 * pw.CONVERGED_MEASURED and pw.CONVERGED_BOUND <= 1e-8

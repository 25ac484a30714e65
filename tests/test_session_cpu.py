"""CPU tests of the solve session's host side (no device, the library is not loaded): the refusals of AlmSolver.restart and
socp.SolveSession with their texts, option names checked first, the caller's arrays and dict left alone, the host scalars of a new
solver against the values recorded before __init__'s tail became _start_run, and the export of dots_restart."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import session_checks as sc
from conftest import ROOT
from dots_socp_amd import _lib

ss = importlib.import_module("dots_socp_amd.socp.solver_socp")


@pytest.fixture
def alm(monkeypatch):
    return sc.recording_solver(monkeypatch.setattr)


def restarts(solver):
    return [c for c in solver.dev.calls if c.startswith("restart")]


def p2(name="plane"):
    return sc.problems(name)[2]


# ---- refusals, all before the library (here: the stand-in's restart) is touched ---------------------------------------------------
def test_restart_refuses_a_time_slab(alm):
    alm.dev.slab = (0, 2, 4)
    with pytest.raises(ValueError, match="restart: not available on time slabs"):
        alm.restart(*p2())
    assert not restarts(alm)


def test_restart_refuses_a_solver_started_from_init_from(alm):
    alm._init_from = True
    with pytest.raises(ValueError, match="restart: the solver was started from init_from"):
        alm.restart(*p2())
    assert not restarts(alm)


def test_a_solver_built_with_init_from_remembers_it(monkeypatch):
    coarse = sc.recording_solver(monkeypatch.setattr)
    coarse.finalized = True
    coarse.dev.prolong_from = lambda *a: 0.5
    fine = sc.recording_solver(monkeypatch.setattr, init_from=coarse)
    assert fine._init_from and not coarse._init_from
    with pytest.raises(ValueError, match="sessions over the cascades are not supported"):
        fine.restart(*p2())


@pytest.mark.parametrize("which", (0, 1))
def test_restart_refuses_wrong_shapes(alm, which):
    masses = list(p2())
    masses[which] = masses[which][:-1]
    with pytest.raises(ValueError, match=rf"restart: mu{which} must have shape \(90,\), got \(89,\)"):
        alm.restart(*masses)
    assert not restarts(alm)


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_restart_refuses_masses_that_are_not_finite(alm, bad):
    mu0, mu1 = p2()
    mu1 = mu1.copy()
    mu1[17] = bad
    with pytest.raises(ValueError, match="restart: mu1 has entries that are not finite"):
        alm.restart(mu0, mu1)
    assert not restarts(alm)


def test_restart_refuses_a_member_of_a_batch(monkeypatch):
    member = sc.recording_solver(monkeypatch.setattr, batched=True)
    with pytest.raises(ValueError, match=r"restart: the solver is stepped by a batch \(solver_socp_many\)"):
        member.restart(*p2())
    assert not restarts(member)


def test_restart_refuses_a_closed_solver(alm):
    alm.close()
    with pytest.raises(ValueError, match="restart: the solver is closed"):
        alm.restart(*p2())
    assert not restarts(alm)


def test_warm_restart_refuses_an_iterate_without_z_mid(alm):
    """After a quiet iteration z_mid was not stored: only a cold restart is possible (the library says the same: DOTS_ERR_STATE)."""
    alm.counter_main, alm._last_quiet = 4, True
    with pytest.raises(ValueError, match="restart: the last iteration stored no z_mid"):
        alm.restart(*p2(), warm=True)
    assert not restarts(alm)
    alm.restart(*p2(), warm=False)
    assert restarts(alm) == ["restart cold"]


def test_restart_checks_the_checkpoints_against_the_new_tolerance(alm):
    with pytest.raises(ValueError, match="Checkpoint value must be greater than tol"):
        alm.restart(*p2(), tol=1e-2, tol_checkpoints=[1e-3])
    assert not restarts(alm)


# ---- option names before the library loads -----------------------------------------------------------------------------------------
def test_option_names_are_checked_before_the_library_loads():
    loaded = _lib._lib
    geom = sc.geometry("plane")
    with pytest.raises(ValueError, match=r"SolveSession: unknown option\(s\) \['init_solution'\]"):
        ss.SolveSession(7, geom, init_solution={})
    with pytest.raises(ValueError, match=r"SolveSession: unknown option\(s\) \['time_slab'\]"):
        ss.SolveSession(7, geom, time_slab=(0, 2))
    with pytest.raises(ValueError, match="n_time \\+ 1 = 1025 time nodes"):
        ss.SolveSession(1024, geom)
    with pytest.raises(ValueError, match="SolveSession: geometry must be a dict"):
        ss.SolveSession(7, {"vertices": geom["vertices"]})
    s = ss.SolveSession(7, geom, tol=sc.TOL)
    with pytest.raises(ValueError, match=r"SolveSession.solve: unknown option\(s\) \['eps'\]"):
        s.solve(*p2(), eps=1e-3)
    with pytest.raises(ValueError, match="outputs and read_out are mutually exclusive"):
        s.solve(*p2(), outputs=("mu",), read_out={})
    with pytest.raises(ValueError, match=r"SolveSession.solve: mu0 must have shape \(90,\)"):
        s.solve(p2()[0][:5], p2()[1])
    with pytest.raises(ValueError, match="SolveSession.solve: mu1 has entries that are not finite"):
        s.solve(p2()[0], np.full(90, np.nan))
    assert s.alm is None and s.index == 0
    s.close()
    with pytest.raises(ValueError, match="SolveSession.solve: the session is closed"):
        s.solve(*p2())
    assert _lib._lib is loaded      # (nothing above loaded the library)


def test_the_torch_function_checks_its_session_arguments_first():
    torch = pytest.importorskip("torch")
    from dots_socp_amd import torch_cost

    mesh, _, (mu0, mu1) = sc.problems("plane")
    with pytest.raises(ValueError, match="transport_cost: 'warm' needs a session"):
        torch_cost.transport_cost(mu0, mu1, mesh["vertices"], mesh["triangles"], 7, warm=True)
    s = ss.SolveSession(7, mesh, tol=sc.TOL)
    moved = mesh["vertices"].copy()
    moved[3, 0] += 1e-9
    with pytest.raises(ValueError, match="transport_cost: vertices / triangles are not the session's"):
        torch_cost.transport_cost(torch.tensor(mu0), torch.tensor(mu1), moved, mesh["triangles"], 7, session=s)
    with pytest.raises(ValueError, match="transport_cost: n_time = 8, the session's 7"):
        torch_cost.transport_cost(torch.tensor(mu0), torch.tensor(mu1), mesh["vertices"], mesh["triangles"], 8, session=s)
    assert s.alm is None


# ---- the caller's data ---------------------------------------------------------------------------------------------------------------
def test_restart_leaves_the_callers_dict_and_arrays_alone(monkeypatch):
    geom = sc.geometry("plane", 1)
    keep = {k: np.array(v) for k, v in geom.items()}
    monkeypatch.setattr(ss, "DeviceProblem", sc.RecordingDevice)
    solver = ss.AlmSolver(7, geom, tol=sc.TOL, nit=10)
    mu0, mu1 = p2()
    k0, k1 = mu0.copy(), mu1.copy()
    for warm in (False, True):
        ms = solver.restart(mu0, mu1, warm=warm)
        assert ms == 0.25 and solver.restart_ms == 0.25
        assert solver.geometry is not geom and set(geom) == set(keep)
        assert all(np.array_equal(geom[k], keep[k]) for k in keep)
        assert np.array_equal(mu0, k0) and np.array_equal(mu1, k1)
        assert np.array_equal(solver.geometry["mu1"], mu1) and solver.geometry["mu1"] is not mu1
        assert solver.geometry["vertices"] is geom["vertices"]      # (a shallow copy)
    assert solver.dev.restart_args[2] == "warm" and len(solver.dev.restart_args[3]) == 4


def test_a_warm_restart_hands_over_the_factors_of_the_run_it_ends(monkeypatch):
    solver = sc.recording_solver(monkeypatch.setattr)
    solver.r, solver.prim_scale, solver.dual_scale = 1.75, 0.5, 3.0      # (as a run leaves them; scale_z = 2 from the initial scaling)
    want = (0.5, 0.25, 1.75 * 3.0, 1.75 * 2.0 * 3.0)
    solver.restart(*p2())
    assert solver.dev.restart_args[2:] == ("warm", want)
    assert solver.r == 1.0 and solver.prim_scale == 1.0      # the new run starts as a new solver's


def test_solve_leaves_the_callers_dict_and_arrays_alone(monkeypatch):
    built = []

    class Solver:
        nit, congestion0 = 3, 0.0

        def __init__(self, n_time, geometry, **options):
            built.append((n_time, geometry, options))
            self.restarted = []

        def restart(self, mu0, mu1, warm=True, **kw):
            self.restarted.append((mu0, mu1, warm, kw))
            return 0.125

        def iterate(self):
            return True

        def finalize(self, **kw):
            import types
            return {"checkpoints": None}, types.SimpleNamespace(solver_stats={})

        def close(self):
            self.was_closed = True

    monkeypatch.setattr(ss, "AlmSolver", Solver)
    geom = sc.geometry("plane", 1)
    keep = {k: np.array(v) for k, v in geom.items()}
    (a0, a1), (b0, b1) = sc.problems("plane")[1:]
    with ss.SolveSession(7, geom, tol=sc.TOL, is_multi_threads=True) as s:
        _, h0 = s.solve(a0, a1)                     # warm=True on the first solve is a cold start
        _, h1 = s.solve(b0, b1, nit=5)
        _, h2 = s.solve(a0, a1, warm=False)
        solver = s.alm
    assert solver.was_closed and len(built) == 1
    n_time, g, options = built[0]
    assert n_time == 7 and options == {"tol": sc.TOL} and np.array_equal(g["mu1"], a1) and g["mu1"] is not a1
    assert [r[2:] for r in solver.restarted] == [(True, {"nit": 5}), (False, {})]
    assert [h.solver_stats["session"]["index"] for h in (h0, h1, h2)] == [0, 1, 2]
    assert [h.solver_stats["session"]["warm"] for h in (h0, h1, h2)] == [False, True, False]
    assert h0.solver_stats["session"]["restart_ms"] is None and h1.solver_stats["session"]["restart_ms"] == 0.125
    assert h0.solver_stats["session"]["setup_seconds_saved"] == 0.0
    assert h1.solver_stats["session"]["setup_seconds_saved"] == h0.solver_stats["session"]["setup_seconds"] == s.setup_seconds
    assert all(np.array_equal(geom[k], keep[k]) for k in keep) and set(geom) == set(keep)


# ---- __init__'s tail, now _start_run ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(sc.VARIANTS))
def test_a_new_solver_leaves_the_recorded_host_scalars(monkeypatch, variant):
    solver = sc.recording_solver(monkeypatch.setattr, **sc.VARIANTS[variant])
    scalars, calls = sc.RECORDED[variant]
    assert sc.host_scalars(solver) == scalars
    assert solver.dev.calls == calls
    assert solver.counter_main == -1 and not solver.finished and not solver.finalized


@pytest.mark.parametrize("variant", sorted(sc.VARIANTS))
def test_a_cold_restart_leaves_the_scalars_of_a_new_solver(monkeypatch, variant):
    """... on what dots_restart reports: the stand-in halves norm_boundary, everything else is a new context's."""
    solver = sc.recording_solver(monkeypatch.setattr, **sc.VARIANTS[variant])
    solver.r, solver.prim_scale, solver.counter_main, solver.finished = 3.0, 0.25, 17, True
    first = solver.run_history
    del solver.dev.calls[:]
    solver.restart(*p2(), warm=False)
    fresh = sc.recording_solver(monkeypatch.setattr, **sc.VARIANTS[variant])
    fresh.dev.params.norm_boundary = solver.dev.params.norm_boundary
    want = sc.host_scalars(fresh)
    if variant != "constant_scaling":      # (there norm_boundary went through the rescaling)
        want["norm_boundary"] = float(0.3125).hex()
        assert sc.host_scalars(solver) == want
    # the calls of a new solver's tail, behind the restart and without building anything
    tail = [c for c in sc.RECORDED[variant][1] if c != "setup_frontal"][1:]      # (one set_params less: cg_tol / cg_max_iter are kept)
    assert solver.dev.calls == ["restart cold"] + tail
    solver.r = 3.0
    del solver.dev.calls[:]
    solver.restart(*p2(), warm=True)
    if variant == "constant_scaling":
        tail.insert(1, "download")      # (phi's storage is borrowed by the constant scaling and put back, as with init_from)
    assert solver.dev.calls == ["restart warm"] + tail
    assert solver.counter_main == -1 and not solver.finished and solver.run_history is not first


def test_restart_takes_the_new_run_options(alm):
    alm.restart(*p2(), nit=5, tol=1e-2, tol_checkpoints=[0.5, 0.1], time_limit=3.0, congestion=0.25)
    assert (alm.nit, alm.tol, alm.tol_checkpoints, alm.time_limit, alm.congestion0) == (5, 1e-2, [0.5, 0.1], 3.0, 0.25)
    assert alm.run_history._max_num == 5
    alm.restart(*p2())
    assert (alm.nit, alm.tol, alm.tol_checkpoints, alm.congestion0) == (5, 1e-2, None, 0.25)


# ---- the library -------------------------------------------------------------------------------------------------------------------
def test_the_built_library_exports_dots_restart():
    assert "dots_restart" in _lib.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "dots_restart" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "kernels_restart.hip" in importlib.import_module("dots_socp_amd.build").SOURCES


def test_restart_desc_matches_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dots_socp_hip.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(dots_restart_desc), offsetof(dots_restart_desc, mode),'
                   " offsetof(dots_restart_desc, factors), offsetof(dots_restart_desc, ms), DOTS_RESTART_COLD, DOTS_RESTART_WARM,"
                   " DOTS_ABI_VERSION); return 0;}\n")
    exe = tmp_path / "probe"
    assert os.system(f"gcc -I{ROOT}/include {src} -o {exe}") == 0
    got = [int(x) for x in os.popen(str(exe)).read().split()]
    assert got == [ctypes.sizeof(_lib.RestartDesc), _lib.RestartDesc.mode.offset, _lib.RestartDesc.factors.offset, _lib.RestartDesc.ms.offset,
                   _lib.RESTART_COLD, _lib.RESTART_WARM, 7]

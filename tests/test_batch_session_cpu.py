"""CPU tests of the batch session's host side (no device): dots_move_vertices_many in the library, the header and the ctypes layer; the
option checks of socp.BatchSession and solve_many, all before a device is touched; the order of the device calls the driver makes on
the recording stand-in of DeviceProblem (session_checks.RecordingDevice) -- restarts instead of constructions, one move of all holders
before any restart --; AlmSolver.restart's refusal of a batch member without the session's route; and the session arguments of
torch_cost.transport_costs."""
import importlib
import os
import subprocess
import types

import numpy as np
import pytest

import move_checks as mc
import session_checks as sc
from conftest import ROOT
from dots_socp_amd import _lib

ss = importlib.import_module("dots_socp_amd.socp.solver_socp")
NAME = "plane"
N_TIME = sc.CASES[NAME][0]


def three_problems():
    """P1, P2 and P1 with its end masses swapped"""
    _, p1, p2 = sc.problems(NAME)
    return [dict(mu0=p1[0], mu1=p1[1]), dict(mu0=p2[0], mu1=p2[1]), dict(mu0=p1[1], mu1=p1[0])]


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_and_the_header_declares_the_call():
    assert "dots_move_vertices_many" in _lib.EXPORTS and _lib.ABI_VERSION == 7
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "dots_move_vertices_many" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    with open(os.path.join(ROOT, "include", "dots_socp_hip.h")) as fh:
        text = fh.read()
    assert "int dots_move_vertices_many(dots_ctx *const *ctxs, int n, const dots_move_desc *desc);" in text
    assert "#define DOTS_ABI_VERSION 7" in text
    lib = _lib.load(host_only=True)
    assert hasattr(lib, "dots_move_vertices_many")


def test_the_call_refuses_null_arguments_without_a_device():
    """The argument checks come before anything touches a context or a device."""
    import ctypes as C

    lib = _lib.load(host_only=True)
    d = _lib.MoveDesc()
    assert lib.dots_move_vertices_many(None, 1, C.byref(d)) == _lib.ERR_ARGUMENT
    hs = (C.c_void_p * 2)(None, None)
    positions = np.zeros((4, 3))
    d.vertices = positions.ctypes.data
    assert lib.dots_move_vertices_many(hs, 2, C.byref(d)) == _lib.ERR_ARGUMENT
    assert b"null context" in lib.dots_last_error()
    assert lib.dots_move_vertices_many(hs, 0, C.byref(d)) == _lib.ERR_ARGUMENT


# ---- option checks, all before a device is touched -------------------------------------------------------------------------------------
def test_the_session_checks_its_options_before_the_library_loads():
    loaded, made = _lib._lib, len(sc.RecordingDevice.instances)
    mesh, p1, _ = sc.problems(NAME)
    with pytest.raises(ValueError, match=r"BatchSession: unknown option\(s\) \['nit'\]"):
        ss.BatchSession(N_TIME, mesh, nit=5)
    with pytest.raises(ValueError, match=r"BatchSession: unknown option\(s\) \['init_solution'\]"):
        ss.BatchSession(N_TIME, mesh, init_solution={})
    with pytest.raises(ValueError, match="lap_solver must be 'modal_direct'"):
        ss.BatchSession(N_TIME, mesh, lap_solver="modal_pcg")
    with pytest.raises(ValueError, match="BatchSession: geometry must be a dict"):
        ss.BatchSession(N_TIME, {"vertices": mesh["vertices"]})
    with pytest.raises(ValueError, match="slots = 1 < max_batch = 2"):
        ss.BatchSession(N_TIME, mesh, max_batch=2, slots=1)
    with pytest.raises(ValueError, match="max_batch >= 1"):
        ss.BatchSession(N_TIME, mesh, max_batch=0)
    with pytest.raises(ValueError, match="pcg_windows belongs to solver_socp"):
        ss.BatchSession(N_TIME, mesh, pcg_windows=True)
    bs = ss.BatchSession(N_TIME, mesh, max_batch=2, tau=1.8, is_constant_scaling=True, eps=0.0)
    assert len(bs.solvers) == 2 and bs.solver_kw["tau"] == 1.8 and bs.solver_kw["is_constant_scaling"] is True
    assert ss.BatchSession(N_TIME, mesh, max_batch=2, slots=5).solvers == [None] * 5
    p = dict(mu0=p1[0], mu1=p1[1])
    with pytest.raises(ValueError, match="BatchSession.solve_many: no problems"):
        bs.solve_many([])
    with pytest.raises(ValueError, match=r"unknown per-problem option 'colour' \(problem 1\)"):
        bs.solve_many([p, dict(p, colour="red")])
    for key in ss.BATCH_SESSION_FIXED + ("eps", "device"):
        with pytest.raises(ValueError, match=f"'{key}' is fixed for the session"):
            bs.solve_many([dict(p, **{key: 1})])
    with pytest.raises(ValueError, match="problem 0: no init_solution"):
        bs.solve_many([dict(p, init_solution={})])
    with pytest.raises(ValueError, match="problem 0 has no mu1"):
        bs.solve_many([dict(mu0=p1[0])])
    with pytest.raises(ValueError, match=r"problem 1: mu0 must have shape \(90,\), got \(89,\)"):
        bs.solve_many([p, dict(p, mu0=p1[0][:-1])])
    for bad in (np.nan, np.inf):
        mu1 = p1[1].copy()
        mu1[17] = bad
        with pytest.raises(ValueError, match="problem 0: mu1 has entries that are not finite"):
            bs.solve_many([dict(p, mu1=mu1)])
    with pytest.raises(ValueError, match="Checkpoint value must be greater than tol"):
        bs.solve_many([dict(p, tol=1e-2, tol_checkpoints=[1e-3])])
    with pytest.raises(ValueError, match="outputs and read_out are mutually exclusive"):
        bs.solve_many([p], outputs=("mu",), read_out={})
    with pytest.raises(ValueError, match=r"vertices must have shape \(90, 3\), got \(90, 2\)"):
        bs.solve_many([p], vertices=mesh["vertices"][:, :2])
    far = mesh["vertices"].copy()
    far[0, 0] = np.inf
    with pytest.raises(ValueError, match="vertices has entries that are not finite"):
        bs.solve_many([p], vertices=far)
    with pytest.raises(ValueError, match=r"warm=True runs problem i in slot i: 3 problems, 2 slots \(problem 2 has none\)"):
        bs.solve_many([p, p, p], warm=True)
    with pytest.raises(ValueError, match="warm=True: slot 0 has not solved a problem yet: problem 0 has no iterate"):
        bs.solve_many([p], warm=True)
    assert bs.solvers == [None, None] and bs.index == 0 and bs.base is None
    bs.close()
    with pytest.raises(ValueError, match="BatchSession.solve_many: the session is closed"):
        bs.solve_many([p])
    assert _lib._lib is loaded and len(sc.RecordingDevice.instances) == made      # (nothing above loaded the library or made a context)


def test_a_problem_describes_its_run_completely():
    """What a problem leaves out is a new solver's default, whatever the slot ran last (cold equals solver_socp_many on the same list)."""
    mesh, p1, _ = sc.problems(NAME)
    bs = ss.BatchSession(N_TIME, mesh)
    got = bs._problems([dict(mu0=p1[0], mu1=p1[1], nit=7), dict(mu0=p1[0], mu1=p1[1])])
    assert {k: got[0][k] for k in ss.SESSION_SOLVE_KEYS} == {**ss.BATCH_SOLVE_DEFAULTS, "nit": 7}
    assert {k: got[1][k] for k in ss.SESSION_SOLVE_KEYS} == ss.BATCH_SOLVE_DEFAULTS
    import inspect

    defaults = {k: v.default for k, v in inspect.signature(ss.AlmSolver.__init__).parameters.items()}
    assert ss.BATCH_SOLVE_DEFAULTS == {k: defaults[k] for k in ss.SESSION_SOLVE_KEYS}


# ---- the driver's device calls on the recording stand-in ---------------------------------------------------------------------------------
class _Calls(list):
    """A device's call list that also writes every call, with the device's number, into one log"""

    def __init__(self, log, tag):
        super().__init__()
        self.log, self.tag = log, tag

    def append(self, name):
        super().append(name)
        self.log.append((self.tag, name))


@pytest.fixture
def recorded(monkeypatch):
    """``log``: (device number, call) in the order the driver makes them; a device's creation is the call "create".  The lockstep
    iteration is replaced by one that records its members and ends their runs; finalize by an empty record."""
    log, made = [], []

    class Device(sc.RecordingDevice):
        def __init__(self, n_time, geometry, **kw):
            super().__init__(n_time, geometry, **kw)
            made.append(self)
            self.tag = len(made) - 1
            log.append((self.tag, "create"))
            self.calls = _Calls(log, self.tag)

    def lockstep(solvers, max_batch):
        running = [a for a in solvers if not a.finished]
        for at in range(0, len(running), max_batch):
            log.append(("step_many", tuple(a.dev.tag for a in running[at:at + max_batch])))
        for a in running:
            a.counter_main, a._last_quiet, a.finished = 0, False, True

    def move_vertices_many(problems, vertices, device_pointers=False):
        log.append(("move_vertices_many", tuple(p.tag for p in problems)))
        return (0.125, 0.25, 0.5)

    monkeypatch.setattr(ss, "DeviceProblem", Device)
    monkeypatch.setattr(ss, "_lockstep", lockstep)
    monkeypatch.setattr(ss.AlmSolver, "finalize", lambda self, **kw: ({"checkpoints": None}, types.SimpleNamespace(solver_stats={})))
    monkeypatch.setattr(importlib.import_module("dots_socp_amd.device"), "move_vertices_many", move_vertices_many)
    return log, made


def device_calls(log, names=("create", "restart cold", "restart warm", "share_frontal", "setup_frontal")):
    return [(tag, c) for tag, c in log if c in names or tag in ("step_many", "move_vertices_many")]


def test_the_second_call_restarts_and_builds_nothing(recorded):
    log, made = recorded
    mesh = sc.problems(NAME)[0]
    problems = three_problems()
    with ss.BatchSession(N_TIME, mesh, max_batch=2) as bs:
        first = bs.solve_many(problems)
        # two contexts: the first builds the factor, the second shares it; the third problem takes the first free slot by a restart
        assert device_calls(log) == [(0, "create"), (0, "setup_frontal"), (1, "create"), (1, "share_frontal"), ("step_many", (0, 1)),
                                     (0, "restart cold"), ("step_many", (0,))]
        assert len(made) == 2 and bs.solved == [True, True]
        assert [h.solver_stats["session"]["index"] for _, h in first] == [0, 1, 2]
        assert [h.solver_stats["session"]["restart_ms"] for _, h in first] == [None, None, 0.25]
        assert [h.solver_stats["batch"]["index"] for _, h in first] == [0, 1, 2] and first[0][1].solver_stats["batch"]["size"] == 3
        saved = [h.solver_stats["session"]["setup_seconds_saved"] for _, h in first]
        assert saved[:2] == [0.0, 0.0] and saved[2] == bs.setup_seconds == first[0][1].solver_stats["session"]["setup_seconds"]
        del log[:]
        second = bs.solve_many(problems)
        assert device_calls(log) == [(0, "restart cold"), (1, "restart cold"), ("step_many", (0, 1)), (0, "restart cold"), ("step_many", (0,))]
        assert len(made) == 2 and all(h.solver_stats["session"]["moved"] is False and h.solver_stats["session"]["move_ms"] is None for _, h in second)
        assert [h.solver_stats["session"]["index"] for _, h in second] == [3, 4, 5]
        # the masses each restart handed over, in input order
        assert np.array_equal(made[1].restart_args[1], problems[1]["mu1"]) and np.array_equal(made[0].restart_args[0], problems[2]["mu0"])
    assert all(d.closed for d in made)


def test_moved_vertices_go_to_all_holders_once_before_any_restart(recorded):
    log, made = recorded
    mesh = sc.problems(NAME)[0]
    moved = mc.displaced(mesh["vertices"])
    problems = three_problems()
    with ss.BatchSession(N_TIME, mesh, max_batch=2) as bs:
        bs.solve_many(problems)
        del log[:]
        results = bs.solve_many(problems, vertices=moved)
        calls = device_calls(log)
        assert calls[0] == ("move_vertices_many", (0, 1)) and [c for c in calls if c[0] == "move_vertices_many"] == calls[:1]
        assert calls[1:] == [(0, "restart cold"), (1, "restart cold"), ("step_many", (0, 1)), (0, "restart cold"), ("step_many", (0,))]
        assert not any(c == "move_vertices" for _, c in log)      # (no member moves on its own)
        assert all(h.solver_stats["session"]["moved"] is True and h.solver_stats["session"]["move_ms"] == (0.125, 0.25, 0.5) for _, h in results)
        want = mc.moved_mesh(mesh, moved)
        for geom in (bs.geometry, bs.solvers[0].geometry, bs.solvers[1].geometry):
            for k in ("vertices", "area_triangles", "area_vertices"):
                assert np.array_equal(geom[k], want[k]), k
        assert "mu0" not in bs.geometry and np.array_equal(bs.solvers[1].geometry["mu1"], problems[1]["mu1"])
        assert np.array_equal(mesh["vertices"], sc.problems(NAME)[0]["vertices"])      # (the caller's mesh is not written to)
        # warm: problem i in slot i, from its own iterate; the move still comes first
        del log[:]
        bs.solve_many(problems[:2], warm=True, vertices=mesh["vertices"])
        assert device_calls(log) == [("move_vertices_many", (0, 1)), (0, "restart warm"), (1, "restart warm"), ("step_many", (0, 1))]
        assert made[0].restart_args[2] == "warm" and len(made[0].restart_args[3]) == 4


def test_the_first_call_takes_the_vertices_as_the_sessions_mesh(recorded):
    log, made = recorded
    mesh = sc.problems(NAME)[0]
    moved = mc.displaced(mesh["vertices"])
    with ss.BatchSession(N_TIME, mesh, max_batch=2) as bs:
        results = bs.solve_many(three_problems()[:1], vertices=moved)
        assert not any(tag == "move_vertices_many" for tag, _ in log) and len(made) == 1
        assert np.array_equal(bs.geometry["vertices"], moved) and np.array_equal(bs.solvers[0].geometry["vertices"], moved)
        assert np.array_equal(bs.base.vertices, moved[bs.base.perm_vert])
        assert results[0][1].solver_stats["session"]["moved"] is True and results[0][1].solver_stats["session"]["move_ms"] is None


def test_more_slots_than_a_lockstep_group_step_in_groups_in_slot_order(recorded):
    log, made = recorded
    mesh = sc.problems(NAME)[0]
    with ss.BatchSession(N_TIME, mesh, max_batch=2, slots=3) as bs:
        bs.solve_many(three_problems())
        assert [c for c in device_calls(log) if c[0] == "step_many"] == [("step_many", (0, 1)), ("step_many", (2,))]
        assert len(made) == 3 and bs.solved == [True, True, True]
        del log[:]
        bs.solve_many(three_problems(), warm=True)
        assert device_calls(log) == [(0, "restart warm"), (1, "restart warm"), (2, "restart warm"), ("step_many", (0, 1)), ("step_many", (2,))]


def test_a_warm_call_names_the_problem_whose_slot_stored_no_z_mid(recorded):
    log, made = recorded
    mesh = sc.problems(NAME)[0]
    with ss.BatchSession(N_TIME, mesh, max_batch=2) as bs:
        bs.solve_many(three_problems()[:2])
        bs.solvers[1]._last_quiet = True
        del log[:]
        with pytest.raises(ValueError, match="BatchSession.solve_many: problem 1: restart: the last iteration stored no z_mid"):
            bs.solve_many(three_problems()[:2], warm=True)
        assert not device_calls(log)      # (refused before the first member restarted)


# ---- AlmSolver.restart -------------------------------------------------------------------------------------------------------------------
def test_restart_refuses_a_batch_member_without_the_sessions_route(monkeypatch):
    member = sc.recording_solver(monkeypatch.setattr, batched=True)
    _, _, p2 = sc.problems(NAME)
    with pytest.raises(ValueError, match=r"restart: the solver is stepped by a batch \(solver_socp_many\); sessions over batches are not supported"):
        member.restart(*p2)
    with pytest.raises(ValueError, match="restart: a member of a batch moves with all holders of its factor"):
        member.restart(*p2, batch_member=True, vertices=sc.problems(NAME)[0]["vertices"])
    assert not [c for c in member.dev.calls if c.startswith("restart") or c == "move_vertices"]
    assert member.restart(*p2, warm=False, batch_member=True) == 0.25
    assert [c for c in member.dev.calls if c.startswith("restart")] == ["restart cold"] and member.batched


# ---- torch ---------------------------------------------------------------------------------------------------------------------------------
def test_the_torch_function_checks_its_batch_session_arguments_first():
    torch = pytest.importorskip("torch")
    from dots_socp_amd import torch_cost

    mesh, (mu0, mu1), _ = sc.problems(NAME)
    m0, m1 = torch.tensor(np.stack([mu0, mu1])), torch.tensor(np.stack([mu1, mu0]))
    with pytest.raises(ValueError, match="transport_costs: 'warm' needs a session"):
        torch_cost.transport_costs(m0, m1, mesh["vertices"], mesh["triangles"], N_TIME, warm=True)
    with pytest.raises(ValueError, match="transport_costs: 'move' needs a session"):
        torch_cost.transport_costs(m0, m1, mesh["vertices"], mesh["triangles"], N_TIME, move=True)
    bs = ss.BatchSession(N_TIME, mesh)
    moved = mesh["vertices"].copy()
    moved[3, 0] += 1e-9
    with pytest.raises(ValueError, match=r"transport_costs: vertices / triangles are not the session's \(a session solves on one mesh; moved "
                                         r"vertices need a new session\)$"):
        torch_cost.transport_costs(m0, m1, moved, mesh["triangles"], N_TIME, session=bs)
    with pytest.raises(ValueError, match="move=True moves the vertices, the triangles must be the session's"):
        torch_cost.transport_costs(m0, m1, moved, np.asarray(mesh["triangles"])[:, [1, 2, 0]], N_TIME, session=bs, move=True)
    with pytest.raises(ValueError, match=f"transport_costs: n_time = {N_TIME + 1}, the session's {N_TIME}"):
        torch_cost.transport_costs(m0, m1, mesh["vertices"], mesh["triangles"], N_TIME + 1, session=bs)
    with pytest.raises(ValueError, match="'tau' is fixed for the session"):
        torch_cost.transport_costs(m0, m1, mesh["vertices"], mesh["triangles"], N_TIME, session=bs, tau=1.5)
    assert bs.solvers == [None] * 4 and bs.index == 0

"""The cases of the solve session (dots_restart, AlmSolver.restart, socp.SolveSession), shared by test_session_cpu.py and
test_hip_session.py (TEST INFRASTRUCTURE): three small meshes with a problem P1 and a neighbouring problem P2 whose mu1 has its
centre one mesh edge further, the host scalars a new AlmSolver leaves (recorded on the commit before the session existed), a stand-in
for DeviceProblem that records the calls the driver makes, and the reference difference between a cold and a host-warm solve that
bounds the warm torch function."""
import types

import numpy as np

from dots_socp_amd import meshes

TOL = 1e-3
# name -> (n_time, iteration cap).  The fp64 oracle (oracle/dots_oracle.py: solver_socp(n_time, P2, tol=1e-3, nit=1000)) stops
# after 341 iterations on "plane" and has not stopped after 1000 on "torus" and "icosphere1" (bumps on very coarse meshes): "plane"
# converges before its cap, the other two end at theirs (a run that ends at the cap compares as well as a converged one).
#     python -c "import sys; sys.path[:0] = ['tests', '.']; import session_checks as s; s.print_oracle_iterations()"
CASES = {"plane": (7, 400), "torus": (5, 200), "icosphere1": (16, 200)}
LIVE_STOP = 39      # iterations of the first run of the "live flags" case, see test_hip_session.py


def _bumps(vertices, triangles, c0, c1):
    area_t = meshes.triangle_areas(vertices, triangles)
    area_v = meshes.vertex_areas(vertices.shape[0], triangles, area_t)
    return meshes.bump_density(vertices, area_v, [c0]), meshes.bump_density(vertices, area_v, [c1])


def neighbour_of(triangles, vertex):
    """The smallest vertex that shares an edge with ``vertex``"""
    t = np.asarray(triangles)
    rows = t[np.any(t == vertex, axis=1)]
    return int(np.min(rows[rows != vertex]))


def problems(name):
    """``(mesh geometry without masses, (mu0, mu1) of P1, (mu0, mu1) of P2)``; P2 moves the centre of mu1 to a neighbouring vertex."""
    if name == "plane":
        geom, _ = meshes.example("plane", n=8)
        v, t = geom["vertices"], geom["triangles"]
        assert v.shape[0] == 90
        mu0 = np.asarray(geom["mu0"], dtype=np.float64)
        av = np.asarray(geom["area_vertices"], dtype=np.float64)
        c1 = int(np.argmin(np.sum((v - np.array([0.6, 0.6, 0.0])) ** 2, axis=1)))
        c2 = neighbour_of(t, c1)
        mu1 = meshes.gaussian_density(v, av, v[c1], 2 * 0.1 ** 2)
        mu1b = meshes.gaussian_density(v, av, v[c2], 2 * 0.1 ** 2)
    else:
        v, t = meshes.torus(12, 8) if name == "torus" else meshes.icosphere(1)
        geom, _ = meshes.make_geometry(v, t, normalize=False)
        v, t = geom["vertices"], geom["triangles"]
        c0, c1 = 0, int(np.argmax(np.sum((v - v[0]) ** 2, axis=1)))
        c2 = neighbour_of(t, c1)
        mu0, mu1 = _bumps(v, t, c0, c1)
        _, mu1b = _bumps(v, t, c0, c2)
    mesh = {k: val for k, val in geom.items() if k not in ("mu0", "mu1")}
    assert not np.array_equal(mu1, mu1b)
    return mesh, (mu0, mu1), (mu0.copy(), mu1b)


def geometry(name, which=2):
    mesh, p1, p2 = problems(name)
    mu0, mu1 = p1 if which == 1 else p2
    return {**mesh, "mu0": mu0, "mu1": mu1}


def print_oracle_iterations():
    from conftest import load_oracle

    O = load_oracle()
    for name, (n_time, _cap) in CASES.items():
        _, hist = O.solver_socp(n_time, geometry(name), tol=TOL, nit=1000)
        print(name, n_time, int(hist.kkt_iteration[-1]) + 1)


# ---- the host scalars of a new AlmSolver, on the stand-in below -------------------------------------------------------------------
SCALARS = ("r", "prim_scale", "dual_scale", "boundary_scale", "const_d", "scale_z", "norm_d", "norm_boundary", "congestion", "congestion0",
           "prim_gap", "tau", "eps")
VARIANTS = {"default": {}, "constant_scaling": {"is_constant_scaling": True}, "congestion": {"congestion": 0.01}}
# Recorded on the commit before AlmSolver.__init__'s tail became _start_run, with
#     python -c "import sys; sys.path[:0] = ['tests', '.']; import session_checks as s; s.print_recorded_scalars()"
# (float.hex of every scalar in SCALARS, then the names of the device calls in order)
RECORDED = {'default': ({'r': '0x1.0000000000000p+0',
              'prim_scale': '0x1.0000000000000p+0',
              'dual_scale': '0x1.0000000000000p+0',
              'boundary_scale': '0x1.0000000000000p+0',
              'const_d': '0x1.0000000000000p+1',
              'scale_z': '0x1.0000000000000p+1',
              'norm_d': '0x1.c000000000000p+1',
              'norm_boundary': '0x1.4000000000000p-1',
              'congestion': '0x0.0p+0',
              'congestion0': '0x0.0p+0',
              'prim_gap': '0x1.0000000000000p+1',
              'tau': '0x1.e666666666666p+0',
              'eps': '0x0.0p+0'},
             ['set_params', 'set_params', 'setup_frontal', 'scale_z', 'set_params']),
 'constant_scaling': ({'r': '0x1.0000000000000p+0',
                       'prim_scale': '0x1.c000000000000p+1',
                       'dual_scale': '0x1.f536bde0d4f6bp+6',
                       'boundary_scale': '0x1.05825724a5bafp-7',
                       'const_d': '0x1.2492492492492p-1',
                       'scale_z': '0x1.0000000000000p+1',
                       'norm_d': '0x1.0000000000000p+0',
                       'norm_boundary': '0x1.46e2ecedcf29ap-8',
                       'congestion': '0x0.0p+0',
                       'congestion0': '0x0.0p+0',
                       'prim_gap': '0x1.0000000000000p+1',
                       'tau': '0x1.e666666666666p+0',
                       'eps': '0x0.0p+0'},
                      ['set_params',
                       'set_params',
                       'setup_frontal',
                       'scale_z',
                       'set_params',
                       'upload',
                       'norm_square phi 1',
                       'norm_square phi 2',
                       'upload',
                       'scale_arrays',
                       'scale_arrays',
                       'set_params',
                       'adjust_penalty',
                       'set_params']),
 'congestion': ({'r': '0x1.0000000000000p+0',
                 'prim_scale': '0x1.0000000000000p+0',
                 'dual_scale': '0x1.0000000000000p+0',
                 'boundary_scale': '0x1.0000000000000p+0',
                 'const_d': '0x1.0000000000000p+1',
                 'scale_z': '0x1.0000000000000p+1',
                 'norm_d': '0x1.c000000000000p+1',
                 'norm_boundary': '0x1.4000000000000p-1',
                 'congestion': '0x1.47ae147ae147bp-7',
                 'congestion0': '0x1.47ae147ae147bp-7',
                 'prim_gap': '0x1.5e2d58d8b3bcep+0',
                 'tau': '0x1.e666666666666p+0',
                 'eps': '0x0.0p+0'},
                ['set_params', 'set_params', 'setup_frontal', 'scale_z', 'set_params'])}


class RecordingDevice:
    """Stands in for DeviceProblem where only the driver's host side is looked at: fixed parameters and norms, every call recorded."""
    instances = []

    def __init__(self, n_time, geometry, **kw):
        V = int(np.asarray(geometry["vertices"]).shape[0])
        self.T, self.V, self.F, self.slab, self.device = int(n_time), V, int(np.asarray(geometry["triangles"]).shape[0]), None, 0
        self.params = types.SimpleNamespace(r=1.0, scale_z=1.0, const_d=1.0, norm_d=1.75, norm_boundary=0.625, congestion=0.0, tau=1.9, eps=0.0,
                                            prim_scale=1.0, dual_scale=1.0, boundary_scale=1.0, cg_tol=1e-8, cg_max_iter=20000)
        mass = 0.5 + np.arange(V) / (2.0 * V)
        self.plan = types.SimpleNamespace(perm_vert=None, mass_vert=mass, mu0=np.asarray(geometry["mu0"], dtype=np.float64),
                                          mu1=np.asarray(geometry["mu1"], dtype=np.float64))
        self.calls, self.closed = [], False
        RecordingDevice.instances.append(self)

    def set_params(self, **kw):
        self.calls.append("set_params")
        for k, v in kw.items():
            setattr(self.params, k, v)

    def shape(self, name):
        return (self.T + 1, self.V)

    def norm_square(self, name, part=0):
        self.calls.append(f"norm_square {name} {part}")
        return 2.0 ** -12 * (1 + part)      # (small: the initial constant scaling then does rescale)

    def close(self):
        self.closed = True

    def restart(self, mu0, mu1, mode="cold", factors=None, device_pointers=False):
        self.calls.append(f"restart {mode}")
        self.restart_args = (np.array(mu0), np.array(mu1), mode, None if factors is None else tuple(factors))
        self.plan.mu0, self.plan.mu1 = np.array(mu0, dtype=np.float64), np.array(mu1, dtype=np.float64)
        for k in ("r", "scale_z", "const_d", "prim_scale", "dual_scale", "boundary_scale"):
            setattr(self.params, k, 1.0)
        self.params.norm_d, self.params.congestion = 1.75, 0.0
        self.params.norm_boundary = 0.3125      # (another problem's: half the first one's)
        return 0.25

    def __getattr__(self, name):      # every other call: recorded, returns None (or a zero array for a download)
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*a, **kw):
            self.calls.append(name)
            return np.zeros(self.shape("phi")) if name == "download" else None
        return call


def host_scalars(alm):
    return {k: float(getattr(alm, k)).hex() for k in SCALARS}


def recording_solver(monkeypatch_setattr, name="plane", **options):
    """An AlmSolver of P1 of ``name`` on the RecordingDevice (``monkeypatch_setattr``: pytest's monkeypatch.setattr, or setattr)."""
    import importlib

    ss = importlib.import_module("dots_socp_amd.socp.solver_socp")
    monkeypatch_setattr(ss, "DeviceProblem", RecordingDevice)
    return ss.AlmSolver(CASES[name][0], geometry(name, 1), tol=TOL, nit=CASES[name][1], **options)


def print_recorded_scalars():
    out = {}
    for key, options in VARIANTS.items():
        alm = recording_solver(setattr, **options)
        out[key] = (host_scalars(alm), list(alm.dev.calls))
    import pprint

    pprint.pprint(out, width=150, sort_dicts=False)


# ---- the device calls of the four drivers, in order ------------------------------------------------------------------------------------
def driver_calls(monkeypatch_setattr):
    """One fixed script through solver_socp, solver_socp_many, SolveSession and BatchSession on the RecordingDevice: returns ``(log,
    stats)``.  ``log``: the calls create, share_frontal, setup_frontal, upload, restart, move_vertices, move_vertices_many, step (one
    solver's loop), step_many (a lockstep group), finalize and close in the order the drivers make them, each with the number of its
    device (the order of creation within a driver: a session's slot) and, where it has one, the problem (the letter of its end masses
    in ``named`` below) and cold / warm.  ``stats``: ``(driver, solver_stats)`` of every result in the order returned, times masked.
    The lockstep iteration is replaced by one that runs every member for a scripted number of rounds, so that slots refill unevenly;
    ``AlmSolver.iterate`` by one step that ends the run; ``finalize`` by an empty record that logs tau, nit and tol.
    test_driver_calls_cpu.py holds what this returned before the drivers shared their intake, slot loop and admission:
        python -c "import sys; sys.path[:0] = ['tests', '.']; import session_checks as s; s.print_driver_calls()"
    """
    import importlib

    ss = importlib.import_module("dots_socp_amd.socp.solver_socp")
    mesh, (mu0, mu1), (_, mu1b) = problems("plane")
    n_time, V = CASES["plane"][0], mesh["vertices"].shape[0]
    named = {"A": (mu0, mu1), "B": (mu0, mu1b), "C": (mu1, mu0), "D": (mu1b, mu0), "E": (mu1, mu1b)}
    P = {k: dict(mu0=a, mu1=b) for k, (a, b) in named.items()}
    moved = np.array(mesh["vertices"], dtype=np.float64)
    moved[:, 2] += 0.02 * np.sin(2.0 * np.pi * moved[:, 0])
    log, made, script = [], [], []

    def letter(a, b):
        return next((k for k, (x, y) in named.items() if np.array_equal(x, a) and np.array_equal(y, b)), "?")

    class Calls(list):
        def __init__(self, tag):
            super().__init__()
            self.tag = tag

        def append(self, name):
            super().append(name)
            if name in ("setup_frontal", "upload"):
                log.append((name, self.tag))

    class Device(RecordingDevice):
        def __init__(self, n_time, geometry, **kw):
            super().__init__(n_time, geometry, **kw)
            made.append(self)
            self.tag = len(made) - 1
            self.calls = Calls(self.tag)
            log.append(("create", self.tag, letter(geometry["mu0"], geometry["mu1"])))

        def share_frontal(self, owner):
            log.append(("share_frontal", self.tag, owner.tag))

        def restart(self, mu0, mu1, mode="cold", factors=None, device_pointers=False):
            log.append(("restart", self.tag, letter(mu0, mu1), mode))
            return super().restart(mu0, mu1, mode, factors, device_pointers)

        def apply_operator(self, *a, **kw):      # (an init_solution of phi alone derives the other arrays from it)
            return np.zeros(1)

        def move_vertices(self, vertices, device_pointers=False):
            log.append(("move_vertices", self.tag))
            return (0.125, 0.25, 0.5)

        def close(self):
            log.append(("close", self.tag))
            super().close()

    def lockstep(solvers, max_batch):
        running = [a for a in solvers if not a.finished]
        for at in range(0, len(running), max_batch):
            log.append(("step_many", tuple(a.dev.tag for a in running[at:at + max_batch])))
        for a in running:
            if a.counter_main < 0:      # (a run that has not stepped yet takes the next scripted length)
                a.rounds_left = script.pop(0) if script else 1
            a.counter_main, a._last_quiet = a.counter_main + 1, False
            a.rounds_left -= 1
            a.finished = a.rounds_left == 0

    def iterate(self):
        log.append(("step", self.dev.tag))
        self.counter_main, self._last_quiet, self.finished = self.counter_main + 1, False, True
        return True

    def finalize(self, **kw):
        log.append(("finalize", self.dev.tag, letter(self.geometry["mu0"], self.geometry["mu1"]), self.tau, self.nit, self.tol))
        return {"checkpoints": None}, types.SimpleNamespace(solver_stats={})

    def move_vertices_many(devices, vertices, device_pointers=False):
        log.append(("move_vertices_many", tuple(d.tag for d in devices)))
        return (0.125, 0.25, 0.5)

    monkeypatch_setattr(ss, "DeviceProblem", Device)
    monkeypatch_setattr(ss, "_lockstep", lockstep)
    monkeypatch_setattr(ss.AlmSolver, "iterate", iterate)
    monkeypatch_setattr(ss.AlmSolver, "finalize", finalize)
    monkeypatch_setattr(importlib.import_module("dots_socp_amd.device"), "move_vertices_many", move_vertices_many)

    stats = []

    def masked(d):
        return {k: ({kk: ("t" if kk.startswith("setup_seconds") and vv else vv) for kk, vv in v.items()} if isinstance(v, dict) else v)
                for k, v in d.items()}

    def run(driver, call, stops=()):
        del made[:]
        script[:] = list(stops)
        log.append(("driver", driver))
        results = call()
        for _, hist in ([results] if isinstance(results, tuple) else results):
            stats.append((driver, masked(hist.solver_stats)))

    run("solver_socp", lambda: ss.solver_socp(n_time, {**mesh, **P["A"]}, tol=TOL, nit=9))
    refill = dict(P["C"], tau=1.7, init_solution={"phi": np.ones((n_time + 1, V))})
    run("solver_socp_many", lambda: ss.solver_socp_many(n_time, mesh, [P["A"], P["B"], refill, P["D"], dict(P["E"], nit=11)], max_batch=2),
        stops=[3, 1, 2, 2, 1])
    with ss.SolveSession(n_time, {**mesh, **P["E"]}, tol=TOL, nit=9) as s:
        run("SolveSession first", lambda: s.solve(*named["A"]))
        run("SolveSession warm", lambda: s.solve(*named["B"], nit=11))
        run("SolveSession vertices", lambda: s.solve(*named["C"], vertices=moved))
        run("SolveSession cold", lambda: s.solve(*named["D"], warm=False))
    with ss.BatchSession(n_time, mesh, max_batch=2, slots=3, tau=1.8) as bs:
        run("BatchSession cold", lambda: bs.solve_many([P["A"], P["B"], dict(P["C"], nit=11), P["D"]]), stops=[1, 2, 1, 1])
        run("BatchSession warm", lambda: bs.solve_many([P["B"], dict(P["A"], tol=TOL)], warm=True), stops=[2, 1])
        run("BatchSession vertices", lambda: bs.solve_many([P["E"], P["D"], P["C"], P["B"], P["A"]], vertices=moved), stops=[2, 1, 1, 1, 1])
    with ss.BatchSession(n_time, {**mesh, **P["E"]}, max_batch=2, slots=3) as bs:
        run("BatchSession first vertices", lambda: bs.solve_many([P["A"], dict(mu1=mu1b)], vertices=moved), stops=[1, 1])
    log.append(("driver", "end"))
    return log, stats


def print_driver_calls():
    import pprint

    from dots_socp_amd.socp.solver_socp import BATCH_TIME_NOTE

    log, stats = driver_calls(setattr)
    print("NOTE = " + repr(BATCH_TIME_NOTE))
    print("LOG = ", end="")
    pprint.pprint(log, width=150, compact=True)
    print("STATS = [")
    for entry in stats:
        print("    " + repr(entry).replace(repr(BATCH_TIME_NOTE), "NOTE") + ",")
    print("]")


# ---- the bar of the warm torch function ----------------------------------------------------------------------------------------------
# |cost(fresh cold) - cost(fresh host-warm)| and the largest absolute difference of each gradient between the same two solves of P2
# at TOL (host-warm: init_solution = the whole solution of P1), both of which exist without a session; measured by
#     PYTHONPATH=. python tests/session_checks.py reference      (on the GPU; prints this dict)
# The session's warm result may differ from the cold one by at most 4 times these (the margin covers the spread between cases).
# ("torus" and "icosphere1" end at their caps far from TOL: their two iterates differ by as much as the figures say.)
WARM_REFERENCE = {'plane': {'cost': 2.3451110460155633e-05, 'mu0': 0.009117831542691815, 'mu1': 0.022013224163800804, 'vertices': 3.19491719944156e-05},
                  'torus': {'cost': 0.04472922473724772, 'mu0': 0.5458193439821681, 'mu1': 0.5873697469557448, 'vertices': 0.21146769762771156},
                  'icosphere1': {'cost': 0.19405032240770526, 'mu0': 0.6936394309603489, 'mu1': 0.5683792688008453, 'vertices': 0.6678337407662772}}
WARM_MARGIN = 4.0


def measure_warm_reference():
    import torch

    from dots_socp_amd import torch_cost
    from dots_socp_amd.socp import solver_socp

    out = {}
    for name, (n_time, cap) in CASES.items():
        mesh, p1, p2 = problems(name)
        first, _ = solver_socp(n_time, {**mesh, "mu0": p1[0], "mu1": p1[1]}, tol=TOL, nit=cap)
        init = {k: v for k, v in first.items() if k != "checkpoints"}
        res = []
        for extra in ({}, {"init_solution": init}):
            m0, m1 = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in p2)
            x = torch.tensor(mesh["vertices"], dtype=torch.float64, requires_grad=True)
            c = torch_cost.transport_cost(m0, m1, x, mesh["triangles"], n_time, tol=TOL, nit=cap, **extra)
            c.backward()
            res.append((float(c.detach()), m0.grad.numpy(), m1.grad.numpy(), x.grad.numpy()))
        a, b = res
        out[name] = {"cost": abs(a[0] - b[0]), "mu0": float(np.max(np.abs(a[1] - b[1]))), "mu1": float(np.max(np.abs(a[2] - b[2]))),
                     "vertices": float(np.max(np.abs(a[3] - b[3])))}
    return out


if __name__ == "__main__":
    import pprint
    import sys

    if sys.argv[1:] == ["reference"]:
        pprint.pprint(measure_warm_reference(), width=150, sort_dicts=False)

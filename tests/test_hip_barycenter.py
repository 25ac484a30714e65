"""GPU tests of the barycentre: dots_barycenter_update against its specification (barycenter.update_host) on random inputs, its
refusals, one and four outer steps of socp.barycenter against barycenter_host over SolveSession on the same device, the plane's exact
barycentres, what crosses to the host and what is built after step 0, and the barycentre of one measure."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import barycenter_checks as bc
from conftest import has_gpu
from dots_socp_amd import _lib, barycenter

ss = importlib.import_module("dots_socp_amd.socp.solver_socp")      # (the package exports the function of this name)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

POTENTIALS = {"potentials": True, "stress": False}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


_contexts = {}


@pytest.fixture(scope="module")
def context():
    """One context per mesh of the update test (nothing is solved on them), closed when the module is done."""
    from dots_socp_amd.device import DeviceProblem

    def get(name):
        if name not in _contexts:
            _contexts[name] = DeviceProblem(1, bc.update_geometry(name), lap_solver="spacetime_pcg", reorder="nd")
        return _contexts[name]
    yield get
    for dev in _contexts.values():
        dev.close()
    _contexts.clear()


def on_device(dev, a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=torch.device("cuda", dev.device)).clone()


@pytest.mark.parametrize("n", bc.UPDATE_N)
@pytest.mark.parametrize("name", list(bc.UPDATE_MESHES))
def test_the_update_equals_its_specification(name, n, context):
    import torch

    dev = context(name)
    V = dev.V
    if name == "torus_nd":
        assert not np.array_equal(dev.plan.perm_vert, np.arange(V))
    nu, potentials, weights, eta, mass = bc.update_inputs(name, n)
    want, s_want = barycenter.update_host(nu, potentials, weights, eta, mass)
    assert s_want["change"] > 0.05 * mass and s_want["gmax"] * eta > 0.5      # an update that does nothing cannot pass
    bound = bc.update_bounds(V, want, s_want)
    phi = [on_device(dev, p) for p in potentials]
    runs = []
    for _ in range(2):
        nu_d, ordered = on_device(dev, nu), torch.full((V,), float("nan"), dtype=torch.float64, device=phi[0].device)
        before = dev.debug_counter(9)
        s = dev.barycenter_update(phi, weights, eta, mass, nu_d, ordered)
        assert dev.debug_counter(9) == before and dev.barycenter_ms > 0.0      # (the call takes no context: its four scalars are not a context's copies)
        runs.append((nu_d.cpu().numpy(), ordered.cpu().numpy(), s))
    got, ordered, s = runs[0]
    print(name, n, "max |nu - host| / bound", float(np.max(np.abs(got - want) / bound["nu"])),
          {k: (abs(s[k] - s_want[k]) / bound[k] if bound[k] else abs(s[k] - s_want[k])) for k in s})
    assert np.all(np.abs(got - want) <= bound["nu"])
    for k in ("sum", "change", "gmax", "min"):
        assert abs(s[k] - s_want[k]) <= bound[k], (k, s[k], s_want[k])
    perm = np.arange(V) if dev.plan.perm_vert is None else dev.plan.perm_vert
    assert np.array_equal(bits(ordered), bits(got[perm]))      # device vertex i is caller vertex perm[i]
    assert np.array_equal(bits(runs[1][0]), bits(got)) and np.array_equal(bits(runs[1][1]), bits(ordered))
    assert all(bits(runs[1][2][k]) == bits(s[k]) for k in s)
    for p, host in zip(phi, potentials):
        assert np.array_equal(bits(p.cpu().numpy()), bits(host))      # the potentials are read only
    # without the second numbering
    alone = on_device(dev, nu)
    assert dev.barycenter_update(phi, weights, eta, mass, alone) == s and np.array_equal(bits(alone.cpu().numpy()), bits(got))


def test_refusals_leave_nu_untouched(context):
    import torch

    from dots_socp_amd import device

    dev = context("torus_nd")
    V = dev.V
    nu, potentials, weights, eta, mass = bc.update_inputs("torus_nd", 2)
    phi = [on_device(dev, p) for p in potentials]
    nu_d = on_device(dev, nu)
    ordered = torch.full((V,), -1.0, dtype=torch.float64, device=nu_d.device)
    row = torch.arange(V, dtype=torch.int32, device=nu_d.device)
    need = int(dev.lib.dots_barycenter_scratch(V))
    assert need == 96 + 16 + 6 * 1 + 4 and dev.lib.dots_barycenter_scratch(0) == -1 and dev.lib.dots_barycenter_scratch(1040) == 1040 + 16 + 6 * 5 + 4
    scratch = torch.zeros(need + V, dtype=torch.float64, device=nu_d.device)
    pointers = (C.c_void_p * 17)(*([phi[0].data_ptr(), phi[1].data_ptr()] + [phi[0].data_ptr()] * 15))
    scalars = np.full(4, np.nan)

    def desc(**change):
        d = _lib.BarycenterDesc()
        d.n, d.device, d.n_vertices = 2, dev.device, V
        d.phi0, d.weights = pointers, np.ascontiguousarray(weights).ctypes.data_as(C.POINTER(C.c_double))
        d.eta, d.mass, d.nu, d.scratch, d.scalars = eta, mass, nu_d.data_ptr(), scratch.data_ptr(), scalars.ctypes.data_as(C.POINTER(C.c_double))
        d.stream = torch.cuda.current_stream(nu_d.device).cuda_stream
        keep = []
        for k, v in change.items():
            if k == "weights" and isinstance(v, list):
                keep.append(np.ascontiguousarray(v, dtype=np.float64))
                v = keep[-1].ctypes.data_as(C.POINTER(C.c_double))
            setattr(d, k, v)
        return d, keep

    no_potentials = C.cast(None, C.POINTER(C.c_void_p))
    no_doubles = C.cast(None, C.POINTER(C.c_double))
    one_null = (C.c_void_p * 2)(phi[0].data_ptr(), None)
    cases = [("n = 0", dict(n=0)), ("n = 17", dict(n=17)), ("n < 0", dict(n=-1)), ("V = 0", dict(n_vertices=0)), ("no potentials", dict(phi0=no_potentials)),
             ("a null potential", dict(phi0=one_null)), ("no weights", dict(weights=no_doubles)), ("no nu", dict(nu=None)), ("no scratch", dict(scratch=None)),
             ("no scalars", dict(scalars=no_doubles)), ("weight nan", dict(weights=[0.5, np.nan])), ("weight inf", dict(weights=[np.inf, 0.5])),
             ("eta nan", dict(eta=np.nan)), ("eta inf", dict(eta=-np.inf)), ("mass nan", dict(mass=np.nan)), ("mass inf", dict(mass=np.inf)),
             ("a map without a target", dict(vertex_row=row.data_ptr())),
             ("nu and its second numbering overlap", dict(nu_device_order=nu_d.data_ptr() + 8 * (V - 1))),
             ("scratch and nu overlap", dict(scratch=nu_d.data_ptr() - 8 * (need - 1))),
             ("scratch and the second numbering overlap", dict(nu_device_order=scratch.data_ptr() + 8 * (need - 1)))]
    for what, change in cases:
        d, keep = desc(**change)
        assert dev.lib.dots_barycenter_update(C.byref(d)) == _lib.ERR_ARGUMENT, what
        assert "barycenter_update" in dev.lib.dots_last_error().decode(), what
    assert dev.lib.dots_barycenter_update(None) == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert np.array_equal(bits(nu_d.cpu().numpy()), bits(nu)) and np.all(np.isnan(scalars)) and float(scratch.abs().sum()) == 0.0      # nothing launched
    # the wrapper's own checks
    with pytest.raises(ValueError, match="contiguous float64 tensors"):
        dev.barycenter_update(phi, weights, eta, mass, nu_d.to(torch.float32))
    with pytest.raises(ValueError, match="contiguous float64 tensors"):
        dev.barycenter_update([p.cpu() for p in phi], weights, eta, mass, nu_d)
    with pytest.raises(ValueError, match="weights must have shape"):
        dev.barycenter_update(phi, weights[:1], eta, mass, nu_d)
    with pytest.raises(ValueError, match="vertex_row must be"):
        device.barycenter_update(phi, weights, eta, mass, nu_d, ordered, row.to(torch.int64))
    # a map with entries that are no rows writes nothing outside: those vertices are left out of the second numbering
    bad = row.clone()
    bad[0], bad[1] = -1, V
    d, keep = desc(nu_device_order=ordered.data_ptr(), vertex_row=bad.data_ptr())
    assert dev.lib.dots_barycenter_update(C.byref(d)) == 0 and np.all(np.isfinite(scalars))
    got, second = nu_d.cpu().numpy(), ordered.cpu().numpy()
    assert np.array_equal(bits(second[2:]), bits(got[2:])) and np.array_equal(second[:2], [-1.0, -1.0])
    assert np.array_equal(scratch[need:].cpu().numpy(), np.zeros(V))      # the scratch is used to its stated length only
    want, _ = barycenter.update_host(nu, potentials, weights, eta, mass)
    assert np.all(np.abs(got - want) <= bc.update_bounds(V, want, {"sum": 1.0, "change": 1.0, "gmax": 1.0, "min": 1.0})["nu"])


def test_a_time_slab_has_no_update():
    from dots_socp_amd.device import DeviceProblem

    with DeviceProblem(3, bc.update_geometry("plane8"), lap_solver="modal_pcg", reorder="nd", time_slab=(0, 2)) as dev:
        nu, potentials, weights, eta, mass = bc.update_inputs("plane8", 1)
        nu_d = on_device(dev, nu)
        with pytest.raises(ValueError, match="time slabs"):
            dev.barycenter_update([on_device(dev, potentials[0])], weights, eta, mass, nu_d)
        assert np.array_equal(bits(nu_d.cpu().numpy()), bits(nu))


# ---- the driver against its slow twin --------------------------------------------------------------------------------------------------
SURFACES = {"torus": (5, 200), "icosphere1": (16, 200)}      # n_time, iteration cap: at tol 1e-3 the solves of bumps on these coarse meshes
TOL = 1e-3                                                   # end at the cap (tests/session_checks.py), so both loops take the same steps
ETA = 0.25                                                   # the surfaces have diameter 2.8 and 2, not 1: potentials of order 1


class Recorded:
    """``DeviceProblem.barycenter_update`` with a record of what every call received and of what the contexts had copied to the host"""

    def __init__(self, monkeypatch):
        from dots_socp_amd.device import DeviceProblem

        self.calls, self.made, self.plans, self.factors = [], [], [], []
        inner, rec = DeviceProblem.barycenter_update, self

        def update(dev, potentials, weights, eta, mass, nu, nu_device_order=None):
            potentials_host = [p.cpu().numpy() for p in potentials]
            nu_before = nu.cpu().numpy()
            s = inner(dev, potentials, weights, eta, mass, nu, nu_device_order)
            rec.calls.append({"potentials": potentials_host, "nu_before": nu_before, "nu": nu.cpu().numpy(), "eta": eta, "scalars": s,
                              "d2h": sum(d.debug_counter(9) for d in rec.made), "made": len(rec.made), "plans": len(rec.plans), "factors": len(rec.factors)})
            return s

        class Counted(ss.DeviceProblem):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                rec.made.append(self)

            def setup_frontal(self, *a, **kw):
                rec.factors.append(1)
                return super().setup_frontal(*a, **kw)

        import dots_socp_amd.geometry as geo

        build_plan = geo.build_plan

        def counted_plan(*a, **kw):
            rec.plans.append(1)
            return build_plan(*a, **kw)

        monkeypatch.setattr(DeviceProblem, "barycenter_update", update)
        monkeypatch.setattr(ss, "DeviceProblem", Counted)
        monkeypatch.setattr(geo, "build_plan", counted_plan)


def session_twin(n_time, mesh, measures, device_masses, **options):
    """``(solve, close)``: ``solve(nu, mu_k)`` of barycenter_host on one SolveSession per measure -- cold on its first solve, then from
    its last iterate, as the driver's slot k runs.  ``device_masses``: from the second solve on the masses go in as tensors on the
    device, so that the restart sums them there as the driver's does."""
    import torch

    from dots_socp_amd.socp import SolveSession

    sessions = [SolveSession(n_time, mesh, **options) for _ in measures]

    def solve(nu, mu):
        k = next(i for i, m in enumerate(measures) if m is mu or np.array_equal(m, mu))
        s = sessions[k]
        if device_masses and s.alm is not None:
            where = torch.device("cuda", s.alm.dev.device)
            nu, mu = torch.as_tensor(nu, device=where), torch.as_tensor(mu, device=where)
        sol, hist = s.solve(nu, mu, warm=True, outputs=(), sensitivity=POTENTIALS)
        return float(hist.history["Transportation cost"][-1]), sol["sensitivity"]["phi0"]

    def close():
        for s in sessions:
            s.close()
    return solve, close


@pytest.mark.parametrize("name", list(SURFACES))
def test_the_driver_equals_the_loop_over_sessions(name, monkeypatch):
    from dots_socp_amd import socp

    n_time, cap = SURFACES[name]
    mesh = bc.surface_geometry(name)
    measures = bc.bump_measures(mesh, 3)
    weights = [0.5, 0.3, 0.2]
    options = dict(tol=TOL, nit=cap)
    rec = Recorded(monkeypatch)
    got = socp.barycenter(n_time, mesh, measures, weights, steps=4, eta=ETA, **options)
    solve, close = session_twin(n_time, mesh, measures, device_masses=True, **options)
    try:
        want = barycenter.barycenter_host(solve, measures, weights, mesh["area_vertices"], 4, ETA)
    finally:
        close()
    first = rec.calls[0]
    # one outer step: the solves are reproducible, so costs and potentials are the twin's bits, and nu is within the update's bound
    twin_first = twin_step0(n_time, mesh, measures, weights, options)
    assert got["objective"][0] == want["objective"][0] == twin_first["objective"]
    for k in range(3):
        assert np.array_equal(bits(first["potentials"][k]), bits(twin_first["potentials"][k])), k
    bound = bc.update_bounds(mesh["vertices"].shape[0], twin_first["nu"], twin_first["scalars"])
    assert first["scalars"]["gmax"] * first["eta"] > 0.05      # the step moves nu
    assert np.all(np.abs(first["nu"] - twin_first["nu"]) <= bound["nu"])
    # four steps
    print(name, "objective", got["objective"], want["objective"], "nu", bc.rel_l1(got["nu"], want["nu"]), "iterations", got["iterations"])
    assert len(got["objective"]) == 4 and got["eta"] == want["eta"]
    assert np.all(np.abs(np.array(got["objective"]) - np.array(want["objective"])) <= 1e-8)
    assert bc.rel_l1(got["nu"], want["nu"]) <= 1e-6
    assert np.all(got["nu"] > 0.0) and abs(math.fsum(got["nu"]) - 1.0) <= 1e-13
    assert got["costs"].shape == (3,) and len(got["iterations"]) == 4 and all(i > 0 for i in got["iterations"])


def twin_step0(n_time, mesh, measures, weights, options):
    """Step 0 of barycenter_host over fresh sessions, with its potentials"""
    kept = []
    solve, close = session_twin(n_time, mesh, measures, device_masses=False, **options)

    def keeping(nu, mu):
        cost, phi0 = solve(nu, mu)
        kept.append(np.array(phi0))
        return cost, phi0
    try:
        r = barycenter.barycenter_host(keeping, measures, weights, mesh["area_vertices"], 1, ETA)
    finally:
        close()
    return {"objective": r["objective"][0], "potentials": kept, "nu": r["nu"], "scalars": r["scalars"][0]}


# ---- the plane: the exact barycentres --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights,t,oracle_l1", (((0.5, 0.5), 0.5, bc.ORACLE_HALF_L1), ((0.25, 0.75), 0.75, bc.ORACLE_QUARTER_L1)))
def test_the_plane_barycentre_is_the_displacement_interpolation(weights, t, oracle_l1):
    from dots_socp_amd import socp

    geom, measures = bc.plane_case()
    r = socp.barycenter(bc.PLANE_T, geom, measures, weights, steps=bc.PLANE_STEPS, eta=bc.PLANE_ETA, tol=bc.PLANE_TOL)
    distance = bc.rel_l1(r["nu"], bc.plane_exact(geom, t))
    print(weights, "objective", r["objective"], "eta", r["eta"], "distance", distance, "iterations", r["iterations"])
    assert distance <= bc.ORACLE_MARGIN * oracle_l1
    if t == 0.5:
        assert abs(r["objective"][-1] - bc.ORACLE_HALF_OBJECTIVE) <= 1e-5
    assert np.all(r["nu"] > 0.0) and abs(math.fsum(r["nu"]) - 1.0) <= 1e-13


def test_one_measure_returns_the_measure():
    from dots_socp_amd import socp

    geom, measures = bc.plane_case()
    r = socp.barycenter(bc.PLANE_T, geom, [measures[1]], steps=10, eta=bc.PLANE_ETA, tol=bc.PLANE_TOL, to_device=True)
    assert r["nu"].is_cuda
    distance = bc.rel_l1(r["nu"].cpu().numpy(), measures[1])
    print("K = 1: objective", r["objective"], "distance to the measure", distance)
    assert distance <= bc.ORACLE_MARGIN * bc.ORACLE_ONE_L1


# ---- what crosses to the host, what is built ---------------------------------------------------------------------------------------------
def test_after_step_0_only_scalars_cross_and_nothing_is_built(monkeypatch):
    """Over steps 1 .. 4 of a K = 3 run dots_debug_counter 9 of the contexts does not grow (it counts the copies of downloads and
    read-outs; the residuals and costs of the solves come through the mailbox and pinned scalars every solve uses and are not arrays);
    the driver itself copies the four scalars of each update, 32 bytes a step, which the update -- a call without a context -- hands
    back in its own descriptor; and no plan, factor or context is made."""
    from dots_socp_amd import socp

    mesh = bc.surface_geometry("torus")
    rec = Recorded(monkeypatch)
    restarts = []
    inner = ss.DeviceProblem.restart

    def restart(dev, mu0, mu1, mode="cold", factors=None, device_pointers=False, device_order=False):
        restarts.append((mode, device_pointers, device_order))
        return inner(dev, mu0, mu1, mode, factors, device_pointers, device_order)
    monkeypatch.setattr(ss.DeviceProblem, "restart", restart)
    r = socp.barycenter(5, mesh, bc.bump_measures(mesh, 3), steps=5, eta=ETA, tol=TOL, nit=60)
    assert len(rec.calls) == 5 and len(r["objective"]) == 5
    assert rec.calls[4]["d2h"] == rec.calls[0]["d2h"] and r["solver_stats"]["bytes_to_host"][1:] == [32] * 4
    assert [(c["made"], c["plans"], c["factors"]) for c in rec.calls] == [(3, 1, 1)] * 5
    assert restarts == [("warm", True, True)] * 12      # every later solve reads its masses where they lie, in the contexts' numbering
    assert [s["warm"] for s in r["solver_stats"]["session"]] == [True] * 3

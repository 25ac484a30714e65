"""GPU tests of the cost gradients (dots_sensitivity) through the C ABI: the kernels against the specification
(sensitivity.potentials_host, stress_host) bit for bit on uploaded random states (the meshes of flow_checks.py, horizons on both
sides of a pitch boundary and at a long-horizon pitch, the "nd" numbering, factors other than 1, every output alone and all
together, host and device outputs), the state hygiene of the entry point, its refusals, the solver options and the torch function."""
import ctypes as C

import numpy as np
import pytest

import flow_checks as fc
import sensitivity_checks as sc
from conftest import has_gpu
from dots_socp_amd import _lib, meshes, sensitivity

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")
PARTS = ("phi0", "phiT", "stress")


def same(a, b):
    """== on the bits (a NaN or a signed zero would differ)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(np.ascontiguousarray(a).view(np.int64),
                                                                                       np.ascontiguousarray(b).view(np.int64))


def raw_call(dev, parts, factor_phi, factor_mu, mass):
    """dots_sensitivity with exactly the outputs ``parts``; the others stay NULL"""
    shapes = {"phi0": (dev.V,), "phiT": (dev.V,), "stress": (dev.F, 3, 6)}
    out = {k: np.full(shapes[k], np.nan) for k in parts}
    d = _lib.SensitivityDesc()
    d.factor_phi, d.factor_mu = factor_phi, factor_mu
    d.mass_vertex = mass.ctypes.data_as(C.POINTER(C.c_double))
    for k in parts:
        setattr(d, k, out[k].ctypes.data)
    _lib.check(dev.lib.dots_sensitivity(dev._h, C.byref(d)), "dots_sensitivity")
    return out


@pytest.mark.parametrize("n_time", sc.HORIZONS)
@pytest.mark.parametrize("name", sc.MESHES)
def test_kernels_equal_the_specification_bit_for_bit(name, n_time):
    """No solve: phi and mu are uploaded, dots_sensitivity is set against the specification on the same arrays, downloaded."""
    from dots_socp_amd.device import DeviceProblem

    v, t = fc.mesh_of(name)
    dev = DeviceProblem(n_time, fc.geometry_of(name), lap_solver="spacetime_pcg", reorder="nd")
    try:
        if name == "torus":      # the device numbering differs from the caller's, for vertices and triangles
            assert not np.array_equal(dev.plan.perm_tri, np.arange(dev.F)) and not np.array_equal(dev.plan.perm_vert, np.arange(dev.V))
        assert dev._state_pitch() == {1: 8, 2: 8, 31: 32, 32: 64, 127: 128, 300: 512}[n_time]
        mu, phi = sc.random_state(name, n_time)
        dev.upload("mu", mu)
        dev.upload("phi", phi)
        mu_d, phi_d = dev.download("mu"), dev.download("phi")
        assert same(mu_d, mu) and same(phi_d, phi)
        mass = sc.vertex_masses(v, t)
        want = dict(zip(PARTS, (*sensitivity.potentials_host(phi_d, sc.FACTOR_PHI),
                                sensitivity.stress_host(mu_d, phi_d, t, mass, sc.FACTOR_MU, sc.FACTOR_PHI))))
        assert np.all(want["stress"][:, :, 0] > 0.0) and not same(want["phi0"], want["phiT"])      # a kernel that does nothing cannot pass
        before = dev.debug_counter(9)
        got = dev.sensitivity(sc.FACTOR_PHI, sc.FACTOR_MU, mass)      # all outputs together
        assert set(got) == set(PARTS) and all(same(got[k], want[k]) for k in PARTS), [k for k in PARTS if not same(got[k], want[k])]
        assert dev.sensitivity_bytes == dev.debug_counter(9) - before == 8 * (2 * dev.V + 18 * dev.F)      # only the outputs cross
        for k in PARTS:                                                # each output alone
            alone = raw_call(dev, (k,), sc.FACTOR_PHI, sc.FACTOR_MU, mass)
            assert same(alone[k], want[k]), k
        assert set(dev.sensitivity(sc.FACTOR_PHI, sc.FACTOR_MU, mass, stress=False)) == {"phi0", "phiT"}
        only = dev.sensitivity(sc.FACTOR_PHI, sc.FACTOR_MU, mass, potentials=False)
        assert set(only) == {"stress"} and same(only["stress"], want["stress"]) and dev.sensitivity_bytes == 8 * 18 * dev.F
        # without masses of the caller's: the context's own (the plan's, device numbering)
        own = np.empty(dev.V)
        own[dev.plan.perm_vert] = dev.plan.mass_vert
        assert same(dev.sensitivity(sc.FACTOR_PHI, sc.FACTOR_MU, potentials=False)["stress"],
                    sensitivity.stress_host(mu_d, phi_d, t, own, sc.FACTOR_MU, sc.FACTOR_PHI))
        # device outputs: torch tensors on the context's device, nothing crosses to the host
        on_dev = dev.sensitivity(sc.FACTOR_PHI, sc.FACTOR_MU, mass, to_device=True)
        assert dev.sensitivity_bytes == 0 and all(a.is_cuda and same(a.cpu().numpy(), want[k]) for k, a in on_dev.items()) and set(on_dev) == set(PARTS)
        for n in ("mu", "phi"):                                        # the state is where it was
            assert same(dev.download(n), {"mu": mu, "phi": phi}[n])
    finally:
        dev.close()


def stepped(n_time, geom, lap_solver="spacetime_pcg", steps=2, seed=0):
    """A context a few ALM steps away from a random upload of phi, mu, E and the vertex multipliers."""
    from dots_socp_amd.device import DeviceProblem

    dev = DeviceProblem(n_time, geom, lap_solver="modal_pcg" if lap_solver == "modal_direct" else lap_solver)
    if lap_solver == "modal_direct":
        dev.setup_frontal()
    else:
        dev.set_params(cg_tol=1e-2, cg_max_iter=4)      # (what the solve returns does not matter here: any state will do)
    rng = np.random.default_rng(seed + 7 * n_time)
    for name in ("phi", "mu", "E", "beta_fst", "beta_end", "lambda_c"):
        dev.upload(name, rng.standard_normal(dev.shape(name)))
    if steps:
        dev.step(steps)
    return dev


@pytest.mark.parametrize("lap_solver", ["spacetime_pcg", "modal_direct"])
def test_sensitivity_leaves_the_state_untouched(lap_solver):
    """k steps, the call, k steps leave the twelve arrays as 2 k steps without it do -- with the hints of the driver's loop set, and
    with a penalty division pending at the call: the call carries it out, and the next iterate is the one without the call."""
    geom = meshes.example("torus", nu=8, nv=6)[0]
    mass = geom["area_vertices"] / 3.0
    a, b = (stepped(20, geom, lap_solver=lap_solver, steps=0, seed=5) for _ in range(2))
    try:
        direct = lap_solver == "modal_direct"
        for dev in (a, b):
            dev.step_flags(carry=direct, kkt_sums=direct)
            dev.step(3)
        before = {n: a.download(n) for n in STATE}
        a.sensitivity(0.5, 3.0, mass)
        for n in STATE:
            assert same(before[n], a.download(n)), n
        for dev in (a, b):
            dev.step(1)
        a.sensitivity(0.5, 3.0, mass)      # (between two steps, nothing read in between)
        for dev in (a, b):
            dev.step(2)
            dev.adjust_penalty(1.7)        # (left to the next iteration's kernels ...)
        got = a.sensitivity(0.5, 3.0, mass)      # (... or to this call, which must carry it out first)
        mu, phi = a.download("mu"), a.download("phi")
        assert same(got["stress"], sensitivity.stress_host(mu, phi, geom["triangles"], mass, 3.0, 0.5))
        assert same(got["phiT"], sensitivity.potentials_host(phi, 0.5)[1])
        for dev in (a, b):
            dev.step(2)
        for n in STATE:
            assert same(a.download(n), b.download(n)), n
    finally:
        a.close()
        b.close()


def test_refusals_leave_the_context_usable():
    from dots_socp_amd.device import DeviceProblem

    geom = meshes.example("plane", n=4)[0]
    mass = geom["area_vertices"] / 3.0
    dev = stepped(6, geom)
    try:
        assert dev.lib.dots_sensitivity(dev._h, None) == _lib.ERR_ARGUMENT      # a NULL desc
        d = _lib.SensitivityDesc()
        d.factor_phi = d.factor_mu = 1.0
        assert dev.lib.dots_sensitivity(dev._h, C.byref(d)) == _lib.ERR_ARGUMENT      # nothing asked for
        out = np.empty(dev.V)
        d.phi0 = out.ctypes.data
        d.factor_mu = np.inf
        assert dev.lib.dots_sensitivity(dev._h, C.byref(d)) == _lib.ERR_ARGUMENT      # a factor that is not finite
        with pytest.raises(ValueError, match="nothing asked for"):
            dev.sensitivity(potentials=False, stress=False)
        with pytest.raises(ValueError, match="shape"):
            dev.sensitivity(mass_vertex=mass[:-1])
        dev.step(1)                                                              # the context still steps
        got = dev.sensitivity(1.0, 1.0, mass)
        assert same(got["stress"], sensitivity.stress_host(dev.download("mu"), dev.download("phi"), geom["triangles"], mass))
    finally:
        dev.close()
    slab = DeviceProblem(7, geom, lap_solver="modal_pcg", time_slab=(0, 2))
    try:
        with pytest.raises(ValueError, match="time slabs"):
            slab.sensitivity()
        d = _lib.SensitivityDesc()
        d.factor_phi = d.factor_mu = 1.0
        d.phi0 = out.ctypes.data
        assert slab.lib.dots_sensitivity(slab._h, C.byref(d)) == _lib.ERR_STATE
        assert slab.download("mu").shape == slab.shape("mu")
    finally:
        slab.close()


# ---------------------------------------------------------------------------- through the solver
SOLVE = dict(tol=sc.PLANE_TOL, nit=sc.PLANE_NIT)


@pytest.fixture(scope="module")
def solved():
    """The plane example of the oracle tests, solved once: ``(geometry, solution with phi, mu and the sensitivity, history)``."""
    from dots_socp_amd.socp import solver_socp

    geom = sc.plane_geometry()
    sol, hist = solver_socp(sc.PLANE_T, geom, outputs=("phi", "mu"), sensitivity=True, **SOLVE)
    return geom, sol, hist


def test_solver_returns_the_sensitivity_of_its_solution(solved):
    """``solution["sensitivity"]`` is the specification on the recovered phi and mu of the same solve, bit for bit; K is the returned
    cost to the parity bar; a batch returns what the single calls return."""
    from dots_socp_amd.socp import solver_socp, solver_socp_many

    geom, sol, hist = solved
    sens, t, mass = sol["sensitivity"], geom["triangles"], geom["area_vertices"] / 3.0
    assert set(sens) == {"phi0", "phiT", "stress", "grad_mu0", "grad_mu1", "n_time", "ms", "bytes"} and sens["n_time"] == sc.PLANE_T
    p0, pT = sensitivity.potentials_host(sol["phi"])
    assert same(sens["phi0"], p0) and same(sens["phiT"], pT) and same(sens["stress"], sensitivity.stress_host(sol["mu"], sol["phi"], t, mass))
    g0, g1 = sensitivity.potential_gradients(p0, pT)
    assert same(sens["grad_mu0"], g0) and same(sens["grad_mu1"], g1)
    assert sens["bytes"] == 8 * (2 * 90 + 18 * 144)
    cost = float(hist.history["Transportation cost"][-1])
    K = sensitivity.kinetic_energy(sens["stress"], geom["vertices"], t, sc.PLANE_T)
    print(f"K = {K:.12f}, cost = {cost:.12f}, relative {sc.relative(K, cost):.2e}; device {sens['ms']:.3f} ms")
    assert sc.relative(K, cost) <= sc.BOUND_COST
    plain, _ = solver_socp(sc.PLANE_T, geom, outputs=("phi",), **SOLVE)      # without the option nothing changes
    assert "sensitivity" not in plain and same(plain["phi"], sol["phi"])
    swapped = dict(mu0=geom["mu1"], mu1=geom["mu0"])
    single, _ = solver_socp(sc.PLANE_T, {**geom, **swapped}, outputs=(), sensitivity={"to_device": False}, **SOLVE)
    many = solver_socp_many(sc.PLANE_T, geom, [dict(SOLVE), dict(SOLVE, **swapped)], outputs=(), sensitivity=True)
    for (got, _), ref in zip(many, (sens, single["sensitivity"])):
        assert all(same(got["sensitivity"][k], ref[k]) for k in PARTS + ("grad_mu0", "grad_mu1"))
    assert not same(many[0][0]["sensitivity"]["stress"], many[1][0]["sensitivity"]["stress"])


def test_drivers_hand_the_sensitivity_to_the_finest_level():
    """``sensitivity`` through the other drivers: the plug-ins pass it on, the cascades ask the finest level; without it nothing
    changes."""
    from dots_socp_amd import socp

    geom = meshes.example("sphere", level=2)[0]
    kw = dict(nit=40, tol=1e-3)
    plain, _ = socp.solver_cascade(31, geom, **kw)
    sol, _ = socp.solver_cascade(31, geom, sensitivity=True, **kw)
    assert "sensitivity" not in plain and same(plain["mu"], sol["mu"]) and same(plain["E"], sol["E"])
    sens = sol["sensitivity"]
    V, F = geom["vertices"].shape[0], geom["triangles"].shape[0]
    assert sens["n_time"] == 31 and sens["stress"].shape == (F, 3, 6) and sens["phiT"].shape == (V,) and np.all(sens["stress"][:, :, 0] >= 0.0)
    levels = meshes.refine_levels(meshes.example("sphere", level=1)[0], 2)
    sol, _ = socp.solver_raw_mesh_cascade(15, levels, sensitivity={"stress": False}, **kw)
    assert set(sol["sensitivity"]) == {"phi0", "phiT", "grad_mu0", "grad_mu1", "n_time", "ms", "bytes"}
    assert sol["sensitivity"]["phi0"].shape == (levels[-1]["vertices"].shape[0],)
    with_congestion, _ = socp.solver(15, geom, congestion=0.05, sensitivity={"stress": False}, **kw)      # the potentials are still returned
    assert abs(with_congestion["sensitivity"]["grad_mu1"].mean()) < 1e-12 and np.any(with_congestion["sensitivity"]["grad_mu1"] != 0.0)


def test_device_outputs_equal_the_host_arrays(solved):
    from dots_socp_amd.socp.solver_socp import AlmSolver

    geom, sol, _ = solved
    alm = AlmSolver(sc.PLANE_T, geom, **SOLVE)
    try:
        for _ in range(sc.PLANE_NIT):
            if alm.iterate():
                break
        host = alm.sensitivity()
        dev = alm.sensitivity(to_device=True)
        assert dev["bytes"] == 0 and host["bytes"] > 0
        for k in PARTS:
            assert dev[k].is_cuda and same(dev[k].cpu().numpy(), host[k]), k
        for k, part in (("grad_mu0", "phi0"), ("grad_mu1", "phiT")):
            # the gauge is fixed in Python: on the device torch sums the mean in another order than numpy does, which moves it by at
            # most V roundings of the largest entry -- and every entry of the gradient with it, plus its own rounding
            bound = (host[part].size + 1) * np.finfo(np.float64).eps * np.abs(host[part]).max()
            assert dev[k].is_cuda and np.abs(dev[k].cpu().numpy() - host[k]).max() <= bound, k
        for k in PARTS + ("grad_mu0", "grad_mu1"):
            assert same(host[k], sol["sensitivity"][k]), k      # (the fixture's run again: the solver is deterministic)
        with pytest.raises(ValueError, match="nothing asked for"):
            alm.sensitivity(potentials=False, stress=False)
    finally:
        alm.close()


def test_torch_backward_is_cost_gradients(solved):
    """The backward of ``transport_cost`` is ``cost_gradients`` of the same solve; one central difference of the device's cost in mu1
    (the direction and eps of the oracle test) is held to the oracle test's bound."""
    import torch

    from dots_socp_amd.torch_cost import transport_cost, transport_costs

    geom, sol, hist = solved
    v, t = geom["vertices"], geom["triangles"]
    mu0, mu1, x = (torch.tensor(a, requires_grad=True) for a in (geom["mu0"], geom["mu1"], v))
    cost = transport_cost(mu0, mu1, x, t, sc.PLANE_T, **SOLVE)
    assert cost.dtype == torch.float64 and cost.shape == () and cost.item() == float(hist.history["Transportation cost"][-1])
    (2.0 * cost).backward()
    g0, g1, gx = sensitivity.cost_gradients(sol["sensitivity"], v, t)
    assert same(mu0.grad.numpy(), 2.0 * g0) and same(mu1.grad.numpy(), 2.0 * g1) and same(x.grad.numpy(), 2.0 * gx)
    assert np.any(gx != 0.0) and gx.shape == v.shape

    def device_cost(g):
        with torch.no_grad():
            return float(transport_cost(g["mu0"], g["mu1"], g["vertices"], t, sc.PLANE_T, **SOLVE))

    d = sc.density_direction(geom["mu1"])
    fd = sc.central_difference(device_cost, geom, sc.EPS_DENSITY, mu1=d)
    print(f"d cost / d mu1 on the device: gradient {float(g1 @ d):.9e}, finite difference {fd:.9e}, relative {sc.relative(float(g1 @ d), fd):.2e}")
    assert sc.relative(float(g1 @ d), fd) <= sc.BOUND_DENSITY
    # a batch on one factor: the first pair is the problem above
    m0 = torch.tensor(np.stack([geom["mu0"], geom["mu1"]]), requires_grad=True)
    m1 = torch.tensor(np.stack([geom["mu1"], geom["mu0"]]))
    costs = transport_costs(m0, m1, v, t, sc.PLANE_T, **SOLVE)
    assert costs.shape == (2,) and costs[0].item() == cost.item()
    costs[0].backward()
    assert same(m0.grad[0].numpy(), g0) and not m0.grad[1].any()

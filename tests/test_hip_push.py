"""GPU tests of the push-forward (dots_flow_push) through the C ABI: the fixed-point sums against the specification
flow.push_forward_host bit for bit on every case of flow_checks.py, colliding particles, dropped contributions, a pending penalty
division and the state hygiene of the entry point, its refusals, the pushed measure of a solved problem against the exact
transport, and the drivers."""
import ctypes as C

import numpy as np
import pytest

import flow_checks as fc
import push_checks as pc
from conftest import has_gpu
from dots_socp_amd import _lib, flow, meshes
from push_checks import same

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")
OUTPUTS = ("triangle", "weights", "status", "rested", "crossings")
TRACE = ("triangles_at", "weights_at")


def assert_pushed(got, want, what=""):
    pc.assert_pushed_equals(got["mass_at"], got["attr_at"], got["dropped"], want, what)


@pytest.mark.parametrize("name", list(fc.CASES))
def test_sums_equal_the_specification_bit_for_bit(name):
    """No solve: the state is uploaded, dots_flow_push is set against push_forward_host on the host trajectory of the same arrays --
    ``==`` on every sum, for 0, 1 and 4 attributes of both signs, the last layer and all of them; what it returns per particle is
    what dots_flow_map returns; only the outputs cross to the host."""
    from dots_socp_amd.device import DeviceProblem

    _, T, _, seed, max_crossings, _ = fc.CASES[name]
    v, t = fc.mesh_of(name)
    V = v.shape[0]
    dev = DeviceProblem(T, fc.geometry_of(name), lap_solver="spacetime_pcg")      # (the default reordering)
    try:
        if name == "torus":
            assert not np.array_equal(dev.plan.perm_vert, np.arange(dev.V))      # (the sums are gathered through a permutation)
        mu, E = fc.random_state(name)
        dev.upload("mu", mu)
        dev.upload("E", E)
        hat, nbr = fc.caller_hat(dev.plan), flow.triangle_neighbours(t)
        tri, w = fc.particles(name)
        P = tri.shape[0]
        host = fc.host_reference(dev.download("mu"), dev.download("E"), t, hat, nbr, tri, w, fc.FLOOR, max_crossings)
        plain = dev.flow_map(tri, w, nbr, fc.FLOOR, max_crossings=max_crossings)
        for A in pc.ATTRIBUTE_COUNTS:
            mass, attributes = pc.carried(P, A, seed)
            for layers in pc.LAYERS:
                want = pc.specification(host, t, V, mass, attributes, layers)
                assert want["dropped"] == 0 and np.any(want["integers"])
                got = dev.flow_push(tri, w, nbr, fc.FLOOR, mass, attributes, layers=layers, max_crossings=max_crossings)
                assert_pushed(got, want, (name, A, layers))
                assert got["dropped"] == 0
                for key in OUTPUTS:
                    assert same(got[key], plain[key]) and same(got[key], host[key]), (name, A, layers, key)
                L = T + 1 if layers == "all" else 1
                assert got["mass_at"].shape == (L, V) and dev.flow_push_bytes == P * 40 + (1 + A) * L * V * 8 + 8
        # with the trajectory, and the exponents given
        mass, attributes = pc.carried(P, 1, seed)
        k = flow.push_scales(mass, attributes, w)
        got = dev.flow_push(tri, w, nbr, fc.FLOOR, mass, attributes, exponents=k - 7, layers="all", max_crossings=max_crossings, trajectory=True)
        assert_pushed(got, pc.specification(host, t, V, mass, attributes, "all", exponents=k - 7), (name, "exponents"))
        for key in OUTPUTS + TRACE:
            assert same(got[key], host[key]), (name, key)
        assert same(got["exponents"], k - 7)
    finally:
        dev.close()


def test_colliding_particles_add_up_in_every_order():
    """A thousand particles at one point of a state below the floor (nobody moves): four workgroups with a ragged tail add to three
    words per layer and channel.  Integer sums: the specification's bits, the same in a second run and with the particles reversed."""
    from dots_socp_amd.device import DeviceProblem

    name = "tetrahedron"
    v, t = fc.mesh_of(name)
    T, P = fc.CASES[name][1], 1000
    dev = DeviceProblem(T, fc.geometry_of(name), lap_solver="spacetime_pcg")
    try:
        mu, E = fc.random_state(name)
        mu = mu * (0.5 * fc.FLOOR / mu.max())
        dev.upload("mu", mu)
        dev.upload("E", E)
        hat, nbr = fc.caller_hat(dev.plan), flow.triangle_neighbours(t)
        tri, w = np.full(P, 2, dtype=np.int32), np.tile(np.array([[0.2, 0.3, 0.5]]), (P, 1))
        host = fc.host_reference(dev.download("mu"), dev.download("E"), t, hat, nbr, tri, w, fc.FLOOR, 16)
        assert np.all(host["triangle"] == 2) and same(host["weights"], w) and np.all(host["crossings"] == 0)
        mass, attributes = pc.carried(P, 4, 1)
        want = pc.specification(host, t, v.shape[0], mass, attributes, "all")
        got = dev.flow_push(tri, w, nbr, fc.FLOOR, mass, attributes, layers="all")
        assert_pushed(got, want)
        elsewhere = np.setdiff1d(np.arange(v.shape[0]), t[2])
        assert np.all(got["mass_at"][:, elsewhere] == 0.0) and np.all(got["attr_at"][:, :, elsewhere] == 0.0)
        assert np.all(got["mass_at"][:, t[2]] > 0.0) and np.all(got["attr_at"][:, :, t[2]] != 0.0)
        np.testing.assert_allclose(got["mass_at"].sum(axis=1), mass.sum(), rtol=1e-14)
        again = dev.flow_push(tri, w, nbr, fc.FLOOR, mass, attributes, layers="all")
        back = dev.flow_push(tri[::-1], w[::-1], nbr, fc.FLOOR, mass[::-1], attributes[:, ::-1], layers="all")
        for other in (again, back):
            assert same(other["mass_at"], got["mass_at"]) and same(other["attr_at"], got["attr_at"]) and other["dropped"] == 0
    finally:
        dev.close()


def test_contributions_that_are_not_numbers_are_dropped_and_counted():
    """One NaN in E of a triangle that carries velocity: the weights of the particles that pass through it become NaN (NaN arithmetic
    only, nothing faults); their contributions are dropped and counted as the specification counts them, the others are summed."""
    from dots_socp_amd.device import DeviceProblem

    name = "strip"
    v, t = fc.mesh_of(name)
    T = fc.CASES[name][1]
    dev = DeviceProblem(T, fc.geometry_of(name), lap_solver="spacetime_pcg")
    try:
        mu, E = fc.random_state(name)
        rho = fc.density_on_triangles(mu, t)
        f = int(np.argmax(rho[0] > fc.FLOOR))
        assert rho[0, f] > fc.FLOOR
        E[1, f, 0] = np.nan
        dev.upload("mu", mu)
        dev.upload("E", E)
        E_d = dev.download("E")
        assert same(E_d, E)
        hat, nbr = fc.caller_hat(dev.plan), flow.triangle_neighbours(t)
        tri, w = fc.particles(name, 257)
        host = fc.host_reference(dev.download("mu"), E_d, t, hat, nbr, tri, w, fc.FLOOR, 16)
        lost = np.isnan(host["weights_at"]).any(axis=2)
        assert np.any(lost[-1]) and not np.all(lost[-1]) and not np.any(lost[0])
        mass, attributes = pc.carried(257, 1, 2)
        for layers in pc.LAYERS:
            want = pc.specification(host, t, v.shape[0], mass, attributes, layers)
            assert want["dropped"] >= 2 * int(lost[-1].sum()) and np.all(np.isfinite(want["mass"]))
            got = dev.flow_push(tri, w, nbr, fc.FLOOR, mass, attributes, layers=layers, trajectory=True)
            assert_pushed(got, want, layers)
            assert same(got["weights_at"], host["weights_at"])
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


def starts_on(geom, n=300, seed=4):
    v, t = geom["vertices"], geom["triangles"]
    rng = np.random.default_rng(seed)
    vt, vw = flow.vertex_starts(t, v.shape[0])
    x = 0.05 + rng.random((n, 3))
    return (np.concatenate([vt, rng.integers(0, t.shape[0], n).astype(np.int32)]), np.concatenate([vw, x / x.sum(axis=1, keepdims=True)]),
            flow.triangle_neighbours(t))


def check_against_host(dev, geom, floor=0.05, layers="all"):
    """The device push first -- it must carry out what is pending itself --, then the specification on the downloads."""
    tri, w, nbr = starts_on(geom)
    mass, attributes = pc.carried(tri.shape[0], 1, 3)
    got = dev.flow_push(tri, w, nbr, floor, mass, attributes, layers=layers, trajectory=True)
    mu, E = dev.download("mu"), dev.download("E")
    assert np.any(mu > floor) and np.any(E != 0.0)
    host = flow.flow_map_host(mu, E, geom["triangles"], fc.caller_hat(dev.plan), nbr, tri, w, floor, trajectory=True)
    assert np.any(host["crossings"] > 0)
    for key in OUTPUTS + TRACE:
        assert same(got[key], host[key]), key
    assert_pushed(got, pc.specification(host, geom["triangles"], geom["vertices"].shape[0], mass, attributes, layers))


@pytest.mark.parametrize("lap_solver", ["spacetime_pcg", "modal_direct"])
def test_push_carries_out_a_pending_division_and_leaves_the_state_untouched(lap_solver):
    """After a step that leaves a penalty division pending the push equals the specification on the downloaded arrays; then k steps,
    the push, k steps leave the twelve arrays as 2 k steps without it do -- with the hints of the driver's loop set."""
    geom = meshes.example("torus", nu=8, nv=6)[0]
    a, b = (stepped(20, geom, lap_solver=lap_solver, steps=0, seed=5) for _ in range(2))
    try:
        direct = lap_solver == "modal_direct"
        tri, w, nbr = starts_on(geom)
        mass, attributes = pc.carried(tri.shape[0], 1, 3)
        for dev in (a, b):
            dev.step_flags(carry=direct, kkt_sums=direct)
            dev.step(3)
            dev.adjust_penalty(1.7)      # (left to the next iteration's kernels: the push must carry it out first)
        check_against_host(a, geom)
        before = {n: a.download(n) for n in STATE}
        for n in STATE:
            b.download(n)      # (the same division, carried out by a download)
        a.flow_push(tri, w, nbr, 0.05, mass, attributes, layers="all", trajectory=True)
        for n in STATE:
            assert same(before[n], a.download(n)), n
        for dev in (a, b):
            dev.step(1)
        a.flow_push(tri, w, nbr, 0.05, mass)      # (between two steps, nothing read in between)
        for dev in (a, b):
            dev.step(2)
        for n in STATE:
            assert same(a.download(n), b.download(n)), n
    finally:
        a.close()
        b.close()


def raw_desc(tri, w, nbr, mass, attributes, k, out):
    """A complete dots_flow_push_desc over the given arrays (``out``: the dict of output arrays, kept alive by the caller)."""
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    d = _lib.FlowPushDesc()
    d.map.n_particles, d.map.max_crossings, d.map.floor = tri.shape[0], 16, 0.05
    d.map.start_triangle, d.map.start_weights, d.map.neighbours = tri.ctypes.data_as(i32), w.ctypes.data_as(f64), nbr.ctypes.data_as(i32)
    d.mass, d.n_attributes, d.all_layers = mass.ctypes.data_as(f64), attributes.shape[0], 0
    d.attributes, d.scale_exponent = attributes.ctypes.data_as(f64), k.ctypes.data_as(i32)
    d.mass_at, d.attr_at = out["mass_at"].ctypes.data_as(f64), out["attr_at"].ctypes.data_as(f64)
    return d


def test_refusals_leave_the_context_usable():
    from dots_socp_amd.device import DeviceProblem

    geom = meshes.example("plane", n=4)[0]
    dev = stepped(6, geom)
    try:
        tri, w, nbr = starts_on(geom, n=20)
        P, F, V = tri.shape[0], dev.F, dev.V
        mass, attributes = pc.carried(P, 2, 4)
        k = flow.push_scales(mass, attributes, w)

        def refused(**change):
            kw = dict(start_triangle=tri, start_weights=w, neighbours=nbr, floor=0.05, mass=mass, attributes=attributes, exponents=k, max_crossings=16)
            kw.update(change)
            with pytest.raises(_lib.HipLibraryError) as err:
                dev.flow_push(**kw)
            assert err.value.status == _lib.ERR_ARGUMENT, change

        def changed(a, index, value):
            a = a.copy()
            a[index] = value
            return a

        # what dots_flow_map refuses
        assert dev.lib.dots_flow_push(dev._h, None) == _lib.ERR_ARGUMENT      # a NULL desc
        refused(start_triangle=tri[:0], start_weights=w[:0], mass=mass[:0], attributes=attributes[:, :0])      # n_particles < 1
        refused(start_triangle=changed(tri, 3, F))
        refused(start_triangle=changed(tri, 3, -1))
        refused(neighbours=changed(nbr, (2, 1), F))
        refused(neighbours=changed(nbr, (2, 1), -2))
        inner = np.argwhere(nbr >= 0)[0]
        wrong = next(g for g in range(F) if g != inner[0] and g not in nbr[inner[0]])
        refused(neighbours=changed(nbr, tuple(inner), wrong))
        refused(neighbours=changed(nbr, tuple(inner), inner[0]))
        refused(start_weights=changed(w, (5, 2), -1e-300))
        refused(start_weights=changed(w, (5, 2), np.inf))
        refused(start_weights=changed(w, (5, 2), np.nan))
        refused(max_crossings=0)
        refused(max_crossings=256)
        refused(floor=np.nan)
        # what the particles carry
        refused(mass=changed(mass, 7, np.inf))
        refused(mass=changed(mass, 7, np.nan))
        refused(attributes=changed(attributes, (1, 7), -np.inf))
        refused(mass=changed(mass, 7, 1e200), attributes=changed(attributes, (1, 7), 1e200), exponents=np.array([0, 0, -900]))      # the product
        # the exponents
        refused(exponents=changed(k, 0, 1001))
        refused(exponents=changed(k, 2, -1001))
        for c in range(3):
            refused(exponents=changed(k, c, k[c] + 2))      # four times the bound of push_scales: above 2^61
        # NULL pointers and the number of attributes, on a description that is complete otherwise
        out = {"mass_at": np.empty((1, V)), "attr_at": np.empty((2, 1, V))}
        assert dev.lib.dots_flow_push(dev._h, C.byref(raw_desc(tri, w, nbr, mass, attributes, k, out))) == 0
        for field in ("mass", "scale_exponent", "mass_at", "attributes", "attr_at"):
            d = raw_desc(tri, w, nbr, mass, attributes, k, out)
            setattr(d, field, None)
            assert dev.lib.dots_flow_push(dev._h, C.byref(d)) == _lib.ERR_ARGUMENT, field
        for field in ("start_triangle", "start_weights", "neighbours"):
            d = raw_desc(tri, w, nbr, mass, attributes, k, out)
            setattr(d.map, field, None)
            assert dev.lib.dots_flow_push(dev._h, C.byref(d)) == _lib.ERR_ARGUMENT, field
        for n_attributes in (-1, 5):
            d = raw_desc(tri, w, nbr, mass, attributes, k, out)
            d.n_attributes = n_attributes
            assert dev.lib.dots_flow_push(dev._h, C.byref(d)) == _lib.ERR_ARGUMENT, n_attributes
        # twice the bound is within the slack of the library's own sum, and the context still serves a correct call
        dev.step(1)
        got = dev.flow_push(tri, w, nbr, 0.05, mass, attributes, exponents=k + 1, layers="all", trajectory=True)
        host = flow.flow_map_host(dev.download("mu"), dev.download("E"), geom["triangles"], fc.caller_hat(dev.plan), nbr, tri, w, 0.05, trajectory=True)
        assert_pushed(got, pc.specification(host, geom["triangles"], V, mass, attributes, "all", exponents=k + 1))
        check_against_host(dev, geom)
    finally:
        dev.close()
    slab = DeviceProblem(7, geom, lap_solver="modal_pcg", time_slab=(0, 2))
    try:
        with pytest.raises(ValueError, match="time slabs"):
            slab.flow_push(tri, w, nbr, 0.05, mass)
        assert slab.lib.dots_flow_push(slab._h, C.byref(raw_desc(tri, w, nbr, mass, attributes, k, out))) == _lib.ERR_STATE
        assert slab.download("mu").shape == slab.shape("mu")
    finally:
        slab.close()


def test_pushed_measure_of_the_translated_bump():
    """The plane example moves a bump from (0.4, 0.4) to (0.6, 0.6).  Four particles per triangle (3 680 on 504 vertices) carry mu0
    forward; every layer of the pushed measure sums to 1 (the weights are never renormalised, and no particle that carries mass
    stops).  The fp64 oracle (the same arguments: 1 000 iterations) with flow_map_host and push_forward_host on its own iterate gives
    a relative L1 distance of 0.0552 between the last layer and mu1, and of 0.0381 between all the layers and the exact
    displacement interpolation at the nodes l / T (evaluate.compare_with_exact_transportation: the reference's norms, the time
    step inside); the bounds are 1.5 times these, 0.0828 and 0.0572 -- room for an iterate that agrees with the oracle's to 1e-6
    but not in its bits, not for another definition.  Its rested mass is 9.5e-6, its stopped mass 0.  (Run to convergence, 1 248
    iterations, the oracle gives 0.0551 and 0.0380 with a rested mass of 2.3e-6; with one particle per vertex 0.0566 and 0.0330
    after 1 000 iterations.)"""
    from dots_socp_amd import evaluate
    from dots_socp_amd.socp import solver
    from dots_socp_amd.socp.solver_socp import AlmSolver

    T = 15
    geom, scale = meshes.example("plane", n=20)
    spec = {"starts": ("triangles", 2), "push": {"layers": "all"}}
    sol, _ = solver(T, geom, tol=1e-4, flow_map=spec)
    fm = sol["flow_map"]
    pushed = fm["pushed"]
    V = geom["vertices"].shape[0]
    assert pushed["mass"].shape == (T + 1, V) and pushed["attributes"] is None and fm["triangle"].shape == (4 * geom["triangles"].shape[0],)
    exact = evaluate.plane_exact_transportation(np.linspace(0.0, 1.0, T + 1), geom["vertices"] / scale, geom["area_vertices"])
    to_exact = evaluate.compare_with_exact_transportation(pushed["mass"], exact, geom)
    print(f"pushed measure of the plane example: layer sums off by {np.max(np.abs(pushed['mass'].sum(axis=1) - 1.0)):.2e}, L1 to mu1 "
          f"{pushed['to_mu1']['l1']:.4f}, L1 to the exact interpolation {to_exact['l1']:.4f}, rested mass {pushed['rested_mass']:.2e}, stopped "
          f"mass {pushed['stopped_mass']:.2e}, dropped {pushed['dropped']}; device {fm['ms']:.3f} ms, {fm['bytes']} bytes")
    assert np.max(np.abs(pushed["mass"].sum(axis=1) - 1.0)) < 1e-12 and pushed["dropped"] == 0
    assert pushed["to_mu1"] == evaluate.compare_with_exact_transportation(pushed["mass"][-1], geom["mu1"], geom)
    assert pushed["to_mu1"]["l1"] < TO_MU1_BOUND and to_exact["l1"] < TO_EXACT_BOUND
    assert pushed["rested_mass"] < 1e-4 and pushed["stopped_mass"] == 0
    # the same call's result equals the specification on the downloaded trajectory, bit for bit
    alm = AlmSolver(T, geom, tol=1e-4)
    try:
        for _ in range(1000):
            if alm.iterate():
                break
        solution, _ = alm.finalize(read_out={"dot_units": True, "centred": True}, flow_map=dict(spec, trajectory=True))
        got = solution["flow_map"]
        for key in OUTPUTS:
            assert same(got[key], fm[key]), key      # (the plug-in's run again: the solver is deterministic)
        assert same(got["pushed"]["mass"], pushed["mass"]) and same(got["pushed"]["exponents"], pushed["exponents"])
        t = geom["triangles"]
        tri, w = flow.triangle_starts(t, 2)
        mass = flow.start_masses(geom["mu0"], geom["area_vertices"], geom["area_triangles"], t, tri, w, 2)
        assert abs(mass.sum() - 1.0) < 1e-14 and same(got["pushed"]["exponents"], flow.push_scales(mass, None, w))
        want = flow.push_forward_host(got, t, V, mass, None, got["pushed"]["exponents"], "all")
        assert same(got["pushed"]["mass"], want["mass"]) and want["dropped"] == 0
        assert got["pushed"]["rested_mass"] == float(np.sum(mass[got["rested"] > 0]))
    finally:
        alm.close()


TO_MU1_BOUND, TO_EXACT_BOUND = 1.5 * 0.0552, 1.5 * 0.0381      # 1.5 times the oracle's figures (see the docstring above)


def test_drivers_hand_the_push_to_the_finest_level():
    """``push`` through the other drivers: the cascades push on the finest level, a batch for every problem; mu and E do not change,
    and without ``push`` the flow map has the keys it had."""
    from dots_socp_amd import socp

    geom = meshes.example("sphere", level=2)[0]
    V = geom["vertices"].shape[0]
    kw = dict(nit=40, tol=1e-3)
    plain, _ = socp.solver_cascade(31, geom, flow_map={"starts": "vertices"}, **kw)
    assert set(plain["flow_map"]) == set(OUTPUTS) | {"positions", "ms", "bytes"}
    sol, _ = socp.solver_cascade(31, geom, flow_map={"starts": "vertices", "push": {"layers": "all", "attributes": geom["vertices"].T}}, **kw)
    assert same(plain["mu"], sol["mu"]) and same(plain["E"], sol["E"])
    fm = sol["flow_map"]
    assert set(fm) == set(plain["flow_map"]) | {"pushed"}
    for key in OUTPUTS:
        assert same(fm[key], plain["flow_map"][key]), key
    pushed = fm["pushed"]
    assert set(pushed) == {"mass", "attributes", "dropped", "exponents", "rested_mass", "stopped_mass", "to_mu1"}
    assert pushed["mass"].shape == (32, V) and pushed["attributes"].shape == (3, 32, V) and pushed["exponents"].shape == (4,)
    assert pushed["dropped"] == 0 and np.max(np.abs(pushed["mass"][0] - geom["mu0"])) < 1e-15      # (layer 0: the starts)
    np.testing.assert_allclose(pushed["mass"].sum(axis=1), geom["mu0"].sum(), rtol=1e-12)
    coarse = meshes.example("sphere", level=1)[0]
    levels = meshes.refine_levels(coarse, 2)
    plain, _ = socp.solver_raw_mesh_cascade(15, levels, **kw)
    sol, _ = socp.solver_raw_mesh_cascade(15, levels, flow_map={"starts": "triangles", "push": True}, **kw)
    assert "flow_map" not in plain and same(plain["mu"], sol["mu"]) and same(plain["E"], sol["E"])
    fine = levels[-1]
    assert sol["flow_map"]["pushed"]["mass"].shape == (1, fine["vertices"].shape[0])
    assert sol["flow_map"]["triangle"].shape == (fine["triangles"].shape[0],)
    problems = [dict(kw), dict(kw, mu0=geom["mu1"], mu1=geom["mu0"])]
    plain = socp.solver_raw_many(15, geom, problems)
    results = socp.solver_raw_many(15, geom, problems, flow_map={"starts": "vertices", "push": True})
    for (p_sol, _), (sol, _) in zip(plain, results):
        assert same(p_sol["mu"], sol["mu"]) and same(p_sol["E"], sol["E"])
        assert sol["flow_map"]["pushed"]["mass"].shape == (1, V) and sol["flow_map"]["pushed"]["dropped"] == 0
    assert not same(results[0][0]["flow_map"]["pushed"]["mass"], results[1][0]["flow_map"]["pushed"]["mass"])

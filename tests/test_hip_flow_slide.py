"""GPU tests of the sliding mode of the flow map (dots_flow_slide) through the C ABI: the kernels against the specification
flow.flow_map_host(..., slide=True, areas) and flow.push_forward_host bit for bit on uploaded random states, the state hygiene of the
entry point, its refusals, dots_flow_trace beside it unchanged, and the option through the solver's plug-in."""
import ctypes as C

import numpy as np
import pytest

import flow_checks as fc
import push_checks as pc
import slide_checks as sl
import span_checks as sc
from conftest import has_gpu
from dots_socp_amd import _lib, flow, meshes
from push_checks import same

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")
OUTPUTS = ("triangle", "weights", "status", "rested", "crossings", "slides", "steps")
LAYERS = ("triangles_at", "weights_at")


def uploaded(name):
    """A context of the case with its random state uploaded (nothing is solved), and what the specification needs"""
    from dots_socp_amd.device import DeviceProblem

    v, t = fc.mesh_of(name)
    dev = DeviceProblem(fc.CASES[name][1], fc.geometry_of(name), lap_solver="spacetime_pcg")      # (the default reordering)
    try:
        mu, E = fc.random_state(name)
        dev.upload("mu", mu)
        dev.upload("E", E)
        mu_d, E_d = dev.download("mu"), dev.download("E")
        assert same(mu_d, mu) and same(E_d, E)
        return dev, t, v.shape[0], mu_d, E_d, fc.caller_hat(dev.plan), sl.caller_areas(dev.plan), flow.triangle_neighbours(t)
    except BaseException:
        dev.close()
        raise


def assert_same_map(got, want, keys, n=None, what=""):
    for key in keys:
        ref = want[key] if n is None else (want[key][:, :n] if key in LAYERS else want[key][:n])
        assert same(got[key], ref), (what, key)


@pytest.mark.parametrize("name", sl.DEVICE_CASES)
def test_kernel_equals_the_specification_bit_for_bit(name):
    """No solve: the state is uploaded, dots_flow_slide is set against flow_map_host(slide=True) on the same arrays, downloaded, over
    the whole horizon forward and backward and over an interior span, at the counts of flow_checks.COUNTS.  One host run of the
    largest count is the reference of every count, every distinct start traced once."""
    _, T, _, _, max_crossings, _ = fc.CASES[name]
    dev, t, V, mu, E, hat, areas, nbr = uploaded(name)
    try:
        if name == "torus":
            assert dev.plan.perm_tri is not None and not np.array_equal(dev.plan.perm_tri, np.arange(dev.F))
        assert dev._state_pitch() == (512 if T == 257 else 8)
        tri, w = fc.particles(name)
        assert tri.shape[0] == max(fc.COUNTS)
        for span in [s for n, s in sl.SPANS if n == name]:
            n = abs(span[1] - span[0])
            tally = {}
            host = sl.host_reference(mu, E, t, hat, areas, nbr, tri, w, fc.FLOOR, max_crossings, span, tally=tally)
            off = sc.host_reference(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings, span)
            # the inputs slide, and the slides change the map: a kernel without the rule cannot pass
            if (name, span) in sl.NO_SLIDES:
                assert not np.any(host["slides"] > 0) and same(host["weights"], off["weights"])
            else:
                assert np.any(host["slides"] > 0) and np.any(sl.moved(host, off)) and np.any(host["action"] != off["action"]), (span, tally)
                assert n != T or (tally["done"] > 0 and tally["passed_on"] > 0), (span, tally)
            for count in fc.COUNTS:
                before = dev.debug_counter(9)
                got = dev.flow_trace(tri[:count], w[:count], nbr, fc.FLOOR, span, action=True, max_crossings=max_crossings, trajectory=True, slide=True)
                assert got["triangles_at"].shape == (n + 1, count)
                assert_same_map(got, host, OUTPUTS + LAYERS + ("action",), count, (name, span, count))
                assert dev.flow_trace_bytes == dev.debug_counter(9) - before == count * (6 * 4 + 24 + 8) + (n + 1) * count * (4 + 24)
        got = dev.flow_map(tri, w, nbr, fc.FLOOR, max_crossings=max_crossings, slide=True)      # the whole horizon, as DeviceProblem.flow_map asks for it
        host = sl.host_reference(mu, E, t, hat, areas, nbr, tri, w, fc.FLOOR, max_crossings, (0, T))
        assert set(got) == set(OUTPUTS)
        assert_same_map(got, host, OUTPUTS, None, name)
        assert dev.flow_map_bytes == tri.shape[0] * 48
    finally:
        dev.close()


@pytest.mark.parametrize("span", [(0, 5), (4, 1)])
def test_push_on_slide_trajectories_equals_the_specification_in_any_order(span):
    """The deposits on the layers of a slide trace against push_forward_host on the specification's slide trajectory, bit for bit, with
    0 and 3 attributes, the last layer and all of them; and the same sums for the particles in reversed order."""
    name = "torus"
    max_crossings = fc.CASES[name][4]
    n = abs(span[1] - span[0])
    dev, t, V, mu, E, hat, areas, nbr = uploaded(name)
    try:
        tri, w = fc.particles(name)
        P = tri.shape[0]
        host = sl.host_reference(mu, E, t, hat, areas, nbr, tri, w, fc.FLOOR, max_crossings, span)
        off = sc.host_reference(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings, span)
        back = slice(None, None, -1)
        for A in (0, 3):
            mass, attributes = pc.carried(P, A, 2)
            for layers in pc.LAYERS:
                want = pc.specification(host, t, V, mass, attributes, layers)
                assert want["dropped"] == 0 and np.any(want["integers"])
                assert not same(want["mass"], pc.specification(off, t, V, mass, attributes, layers)["mass"])      # (the slides move mass)
                got = dev.flow_trace(tri, w, nbr, fc.FLOOR, span, action=True, mass=mass, attributes=attributes, layers=layers, max_crossings=max_crossings,
                                     slide=True)
                pc.assert_pushed_equals(got["mass_at"], got["attr_at"], got["dropped"], want, (span, A, layers))
                L = n + 1 if layers == "all" else 1
                assert got["mass_at"].shape == (L, V) and dev.flow_trace_bytes == P * 56 + (1 + A) * L * V * 8 + 8
                assert_same_map(got, host, OUTPUTS + ("action",))
                turned = dev.flow_trace(tri[back], w[back], nbr, fc.FLOOR, span, mass=mass[back], attributes=None if A == 0 else attributes[:, back],
                                        exponents=got["exponents"], layers=layers, max_crossings=max_crossings, slide=True)
                pc.assert_pushed_equals(turned["mass_at"], turned["attr_at"], turned["dropped"], want, (span, A, layers, "reversed"))
                assert same(turned["slides"], host["slides"][back])
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


def check_against_host(dev, geom, span, floor=0.05):
    """The device trace first -- it must carry out what is pending itself --, then the specification on the downloads."""
    tri, w, nbr = starts_on(geom)
    mass, attributes = pc.carried(tri.shape[0], 1, 3)
    got = dev.flow_trace(tri, w, nbr, floor, span, action=True, mass=mass, attributes=attributes, layers="all", trajectory=True, slide=True)
    mu, E = dev.download("mu"), dev.download("E")
    assert np.any(mu > floor) and np.any(E != 0.0)
    host = flow.flow_map_host(mu, E, geom["triangles"], fc.caller_hat(dev.plan), nbr, tri, w, floor, trajectory=True, span=span, action=True, slide=True,
                              areas=sl.caller_areas(dev.plan))
    assert np.any(host["crossings"] > 0) and np.any(host["slides"] > 0) and np.any(host["action"] > 0.0)
    assert_same_map(got, host, OUTPUTS + LAYERS + ("action",))
    want = pc.specification(host, geom["triangles"], geom["vertices"].shape[0], mass, attributes, "all")
    pc.assert_pushed_equals(got["mass_at"], got["attr_at"], got["dropped"], want)


def test_slide_carries_out_a_pending_division_and_leaves_the_state_untouched():
    """On the direct solver, with the hints of the driver's loop set (carried sums, a launch ahead): after a step that leaves a penalty
    division pending the slide trace equals the specification on the downloaded arrays; then k steps, the trace, k steps leave the
    twelve arrays as 2 k steps without it do."""
    geom = meshes.example("torus", nu=8, nv=6)[0]
    a, b = (stepped(20, geom, lap_solver="modal_direct", steps=0, seed=5) for _ in range(2))
    try:
        tri, w, nbr = starts_on(geom)
        mass, _ = pc.carried(tri.shape[0], 0, 3)
        for dev in (a, b):
            dev.step_flags(carry=True, kkt_sums=True)
            dev.step(3)
            dev.adjust_penalty(1.7)      # (left to the next iteration's kernels: the trace must carry it out first)
        check_against_host(a, geom, (13, 4))
        before = {n: a.download(n) for n in STATE}
        for n in STATE:
            b.download(n)      # (the same division, carried out by a download)
        a.flow_trace(tri, w, nbr, 0.05, (20, 0), action=True, mass=mass, layers="all", trajectory=True, slide=True)
        for n in STATE:
            assert same(before[n], a.download(n)), n
        for dev in (a, b):
            dev.step(1)
        a.flow_trace(tri, w, nbr, 0.05, (3, 17), action=True, slide=True)      # (between two steps, nothing read in between)
        for dev in (a, b):
            dev.step(2)
        for n in STATE:
            assert same(a.download(n), b.download(n)), n
    finally:
        a.close()
        b.close()


def test_slide_on_a_modal_pcg_context():
    geom = meshes.example("torus", nu=8, nv=6)[0]
    dev = stepped(12, geom, lap_solver="modal_pcg", steps=2)
    try:
        check_against_host(dev, geom, (0, 12))
    finally:
        dev.close()


def test_refusals_leave_the_context_usable():
    geom = meshes.example("plane", n=4)[0]
    dev = stepped(6, geom)
    try:
        tri, w, nbr = starts_on(geom, n=20)
        P = tri.shape[0]
        out = {"triangle": np.empty(P, dtype=np.int32), "weights": np.empty((P, 3)), "status": np.empty(P, dtype=np.int32),
               "rested": np.empty(P, dtype=np.int32), "crossings": np.empty(P, dtype=np.int32), "action": np.empty(P),
               "slides": np.empty(P, dtype=np.int32), "steps": np.empty(P, dtype=np.int32)}
        i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)

        def desc(node_from, node_to, slides=True, steps=True):
            d = _lib.FlowSlideDesc()
            m = d.trace.map
            m.n_particles, m.max_crossings, m.floor = P, 16, 0.05
            m.start_triangle, m.start_weights, m.neighbours = tri.ctypes.data_as(i32), w.ctypes.data_as(f64), nbr.ctypes.data_as(i32)
            m.triangle, m.weights = out["triangle"].ctypes.data_as(i32), out["weights"].ctypes.data_as(f64)
            m.status, m.rested, m.crossings = (out[key].ctypes.data_as(i32) for key in ("status", "rested", "crossings"))
            d.trace.node_from, d.trace.node_to, d.trace.action = node_from, node_to, out["action"].ctypes.data_as(f64)
            if slides:
                d.slides = out["slides"].ctypes.data_as(i32)
            if steps:
                d.steps = out["steps"].ctypes.data_as(i32)
            return d

        assert dev.lib.dots_flow_slide(dev._h, None) == _lib.ERR_ARGUMENT      # a NULL desc
        before = dev.debug_counter(9)
        assert dev.lib.dots_flow_slide(dev._h, C.byref(desc(6, 0, slides=False))) == _lib.ERR_ARGUMENT      # a NULL slides
        for nodes in ((-1, 3), (7, 0), (0, 7), (3, 3)):      # a bad span
            assert dev.lib.dots_flow_slide(dev._h, C.byref(desc(*nodes))) == _lib.ERR_ARGUMENT, nodes
        d = desc(6, 0)
        d.trace.map.weights = None      # what dots_flow_map refuses, on a description that is complete otherwise
        assert dev.lib.dots_flow_slide(dev._h, C.byref(d)) == _lib.ERR_ARGUMENT
        assert dev.debug_counter(9) == before      # (nothing ran)
        out["steps"][:] = -7
        assert dev.lib.dots_flow_slide(dev._h, C.byref(desc(6, 0, steps=False))) == 0      # steps may be NULL
        assert np.all(out["steps"] == -7) and np.all(out["slides"] >= 0) and dev.debug_counter(9) - before == P * (4 * 4 + 24 + 8 + 4)
        dev.step(1)                                                                          # and the context still steps
        check_against_host(dev, geom, (6, 0))
        check_against_host(dev, geom, (2, 5))
    finally:
        dev.close()
    from dots_socp_amd.device import DeviceProblem

    slab = DeviceProblem(7, geom, lap_solver="modal_pcg", time_slab=(0, 2))
    try:
        with pytest.raises(ValueError, match="time slabs"):
            slab.flow_map(tri, w, nbr, 0.05, slide=True)
        assert slab.lib.dots_flow_slide(slab._h, C.byref(desc(6, 0))) == _lib.ERR_STATE
        assert slab.download("mu").shape == slab.shape("mu")
    finally:
        slab.close()


def test_dots_flow_trace_beside_it_is_unchanged():
    """The kernels of dots_flow_trace share the template with the new flag: on the same inputs they still equal
    flow_map_host(slide=False), and not the slide's result."""
    name = "torus"
    T, max_crossings = fc.CASES[name][1], fc.CASES[name][4]
    dev, t, V, mu, E, hat, areas, nbr = uploaded(name)
    try:
        tri, w = fc.particles(name)
        host = sc.host_reference(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings, (0, T))
        got = dev.flow_trace(tri, w, nbr, fc.FLOOR, (0, T), action=True, max_crossings=max_crossings, trajectory=True)
        assert "slides" not in got
        assert_same_map(got, host, OUTPUTS[:5] + LAYERS + ("action",))
        slid = dev.flow_trace(tri, w, nbr, fc.FLOOR, (0, T), action=True, max_crossings=max_crossings, trajectory=True, slide=True)
        assert not same(slid["weights"], got["weights"]) and int(slid["rested"].sum()) * 2 <= int(got["rested"].sum())
    finally:
        dev.close()


def test_the_option_through_the_plug_in_and_a_batch():
    """solver(15, plane n = 20, nit = 30) with {"slide": True, "push": True}: the map equals the specification on the arrays the device
    holds (the solver's own loop stopped after the same 30 iterations: it is deterministic), bit for bit, and the particles that rest
    carry less than a fifth of the mass they carry without "slide" (the fp64 oracle: 4.46e-3 against 9.82e-2).  A batch hands the
    option to every member."""
    from dots_socp_amd import socp
    from dots_socp_amd.socp.solver_socp import AlmSolver

    geom = meshes.example("plane", n=20)[0]
    v, t = geom["vertices"], geom["triangles"]
    spec = {"starts": "vertices", "slide": True, "push": True}
    sol, _ = socp.solver(15, geom, nit=30, flow_map=spec)
    plain, _ = socp.solver(15, geom, nit=30, flow_map={"starts": "vertices", "push": True})
    fm, off = sol["flow_map"], plain["flow_map"]
    assert same(sol["mu"], plain["mu"]) and same(sol["E"], plain["E"])
    assert set(fm) == set(off) | {"slides", "steps", "span", "nodes"} and fm["span"] == (0, 15)
    assert set(fm["pushed"]) == set(off["pushed"]) | {"slid_mass"}
    rested, rested_off = fm["pushed"]["rested_mass"], off["pushed"]["rested_mass"]
    print(f"plane example after 30 iterations: rested mass {rested_off:.3e} -> {rested:.3e}, slid mass {fm['pushed']['slid_mass']:.3e}, "
          f"to_mu1 l1 {off['pushed']['to_mu1']['l1']:.4f} -> {fm['pushed']['to_mu1']['l1']:.4f}; device ms {off['ms']:.3f} -> {fm['ms']:.3f}")
    assert rested_off > 0.0 and rested < rested_off / 5.0
    assert fm["pushed"]["slid_mass"] > 0.0 and abs(fm["pushed"]["mass"].sum() - geom["mu0"].sum()) < 1e-12
    alm = AlmSolver(15, geom, nit=30)
    try:
        for _ in range(30):
            if alm.iterate():
                break
        solution, _ = alm.finalize(read_out={"dot_units": True, "centred": True}, flow_map=dict(spec, trajectory=True))
        got = solution["flow_map"]
        assert_same_map(got, fm, OUTPUTS)      # (the plug-in's run again)
        dev = alm.dev
        mu, E = dev.download("mu"), dev.download("E")
        tri, w = flow.vertex_starts(t, v.shape[0])
        floor = 1e-3 * float(np.max(geom["mu0"] / (geom["area_vertices"] / 3.0))) / (alm.r * alm.dual_scale)
        want = flow.flow_map_host(mu, E, t, fc.caller_hat(dev.plan), flow.triangle_neighbours(t), tri, w, floor, trajectory=True, slide=True,
                                  areas=sl.caller_areas(dev.plan))
        assert np.any(want["slides"] > 0)
        assert_same_map(got, want, OUTPUTS + LAYERS)
        pushed = pc.specification(want, t, v.shape[0], geom["mu0"], None, "end")
        pc.assert_pushed_equals(got["pushed"]["mass"], got["pushed"]["attributes"], got["pushed"]["dropped"], pushed)
    finally:
        alm.close()
    small = meshes.example("sphere", level=2)[0]
    kw = dict(nit=40, tol=1e-3)
    problems = [dict(kw), dict(kw, mu0=small["mu1"], mu1=small["mu0"])]
    without = socp.solver_raw_many(15, small, problems, flow_map={"starts": "vertices"})
    results = socp.solver_raw_many(15, small, problems, flow_map={"starts": "vertices", "slide": True})
    for (p_sol, _), (s_sol, _) in zip(without, results):
        assert same(p_sol["mu"], s_sol["mu"]) and same(p_sol["E"], s_sol["E"])
        assert np.any(s_sol["flow_map"]["slides"] > 0) and int(s_sol["flow_map"]["rested"].sum()) < int(p_sol["flow_map"]["rested"].sum())
    assert not same(results[0][0]["flow_map"]["weights"], results[1][0]["flow_map"]["weights"])

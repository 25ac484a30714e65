"""GPU tests of the trace between two time nodes (dots_flow_trace) through the C ABI: the kernels against the specification
flow.flow_map_host(..., span, action) and flow.push_forward_host bit for bit on uploaded random states, against dots_flow_map and
dots_flow_push over the whole horizon, a pending penalty division and the state hygiene of the entry point, its refusals, and the
backward map, the round trip and the action of a solved problem against the figures of the fp64 oracle."""
import ctypes as C

import numpy as np
import pytest

import flow_checks as fc
import push_checks as pc
import span_checks as sc
from conftest import has_gpu
from dots_socp_amd import _lib, flow, meshes
from push_checks import same

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")
OUTPUTS = ("triangle", "weights", "status", "rested", "crossings")
LAYERS = ("triangles_at", "weights_at")
COUNTS = (1, 65, 1000)
SPANS = [("tetrahedron", (1, 0)), ("icosphere1", (3, 0)), ("icosphere1", (1, 2)), ("torus", (5, 0)), ("torus", (1, 4)), ("torus", (4, 1)),
         ("plane4", (7, 0)), ("plane4", (6, 1)), ("icosphere0_257", (257, 0))]


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
        return dev, t, v.shape[0], mu_d, E_d, fc.caller_hat(dev.plan), flow.triangle_neighbours(t)
    except BaseException:
        dev.close()
        raise


def assert_same_map(got, want, keys, n=None, what=""):
    for key in keys:
        ref = want[key] if n is None else (want[key][:, :n] if key in LAYERS else want[key][:n])
        assert same(got[key], ref), (what, key)


@pytest.mark.parametrize("name,span", SPANS, ids=[f"{n}-{a}-{b}" for n, (a, b) in SPANS])
def test_kernel_equals_the_specification_bit_for_bit(name, span):
    """No solve: the state is uploaded, dots_flow_trace is set against flow_map_host at the span, with the action, on the same arrays,
    downloaded.  One host run of the largest count is the reference of every count, every distinct start traced once
    (span_checks.host_reference); icosphere0_257 has a pool of 64 interior starts, three crossings before a rest and a pitch of 512."""
    _, T, is_open, _, max_crossings, _ = fc.CASES[name]
    n = abs(span[1] - span[0])
    dev, t, V, mu, E, hat, nbr = uploaded(name)
    try:
        if name == "torus":
            assert dev.plan.perm_tri is not None and not np.array_equal(dev.plan.perm_tri, np.arange(dev.F))
        assert dev._state_pitch() == (512 if T == 257 else 8)
        tri, w = fc.particles(name)
        assert tri.shape[0] == max(COUNTS)
        host = sc.host_reference(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings, span)
        # the inputs exercise every rule: a kernel that does nothing cannot pass
        seen = sc.exercised(name, mu, t, host, span)
        assert all(seen.values()) and ("stopped" in seen) == is_open, seen
        assert np.any(host["triangle"] != tri) and np.any(host["weights"] != w) and np.any(host["action"] > 0.0)
        if span[1] < span[0]:      # (and backward is not forward over the same intervals)
            other = sc.host_reference(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings, (span[1], span[0]), action=False)
            assert not same(other["weights"], host["weights"])
        for count in COUNTS:
            before = dev.debug_counter(9)
            got = dev.flow_trace(tri[:count], w[:count], nbr, fc.FLOOR, span, action=True, max_crossings=max_crossings, trajectory=True)
            assert got["triangles_at"].shape == (n + 1, count)
            assert_same_map(got, host, OUTPUTS + LAYERS + ("action",), count, (name, span, count))
            assert dev.flow_trace_bytes == dev.debug_counter(9) - before == count * (4 * 4 + 24 + 8) + (n + 1) * count * (4 + 24)      # only the outputs cross
        got = dev.flow_trace(tri, w, nbr, fc.FLOOR, span, max_crossings=max_crossings)      # without the trajectory and the action
        assert set(got) == set(OUTPUTS)
        assert_same_map(got, host, OUTPUTS, None, (name, span))
        assert dev.flow_trace_bytes == tri.shape[0] * 40
    finally:
        dev.close()


def test_the_whole_horizon_equals_flow_map_and_flow_push():
    """dots_flow_map and dots_flow_push pinned to dots_flow_trace with (0, T) and no action on the same inputs, through the three entry
    points: one kernel family behind them, the same bits -- outputs, layers, mass_at, attr_at and dropped, with 0 and 3 attributes,
    the last layer and all of them -- and the same bytes to the host."""
    name = "torus"
    T, max_crossings = fc.CASES[name][1], fc.CASES[name][4]
    dev, t, V, mu, E, hat, nbr = uploaded(name)
    try:
        tri, w = fc.particles(name)
        plain = dev.flow_map(tri, w, nbr, fc.FLOOR, max_crossings=max_crossings, trajectory=True)
        got = dev.flow_trace(tri, w, nbr, fc.FLOOR, (0, T), max_crossings=max_crossings, trajectory=True)
        assert set(got) == set(plain) and np.any(plain["crossings"] > 0)
        assert_same_map(got, plain, OUTPUTS + LAYERS)
        assert dev.flow_trace_bytes == dev.flow_map_bytes
        for A in (0, 3):
            mass, attributes = pc.carried(tri.shape[0], A, 1)
            for layers in pc.LAYERS:
                want = dev.flow_push(tri, w, nbr, fc.FLOOR, mass, attributes, layers=layers, max_crossings=max_crossings, trajectory=True)
                got = dev.flow_trace(tri, w, nbr, fc.FLOOR, (0, T), mass=mass, attributes=attributes, layers=layers, max_crossings=max_crossings,
                                     trajectory=True)
                assert set(got) == set(want) and np.any(want["mass_at"] != 0.0)
                assert_same_map(got, want, OUTPUTS + LAYERS, None, (A, layers))
                assert same(got["mass_at"], want["mass_at"]) and got["dropped"] == want["dropped"] and same(got["exponents"], want["exponents"])
                assert got["attr_at"] is None if A == 0 else same(got["attr_at"], want["attr_at"])
                assert dev.flow_trace_bytes == dev.flow_push_bytes
    finally:
        dev.close()


@pytest.mark.parametrize("span", [(5, 0), (4, 1)])
def test_push_at_a_span_equals_the_specification_and_split_calls_add(span):
    """The deposits on the layers of a backward and of a partial trace against push_forward_host, bit for bit, the last layer (the state
    at node_to) and all n + 1; two calls over the two halves of the particles with the exponents of the whole add to it exactly
    (exponents 8 below push_scales: every sum stays below 2^53, so the doubles hold the integers)."""
    name = "torus"
    max_crossings = fc.CASES[name][4]
    n = abs(span[1] - span[0])
    dev, t, V, mu, E, hat, nbr = uploaded(name)
    try:
        tri, w = fc.particles(name)
        P = tri.shape[0]
        host = sc.host_reference(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings, span)
        for A in (0, 3):
            mass, attributes = pc.carried(P, A, 2)
            for layers in pc.LAYERS:
                want = pc.specification(host, t, V, mass, attributes, layers)
                assert want["dropped"] == 0 and np.any(want["integers"])
                got = dev.flow_trace(tri, w, nbr, fc.FLOOR, span, action=True, mass=mass, attributes=attributes, layers=layers, max_crossings=max_crossings)
                pc.assert_pushed_equals(got["mass_at"], got["attr_at"], got["dropped"], want, (span, A, layers))
                L = n + 1 if layers == "all" else 1
                assert got["mass_at"].shape == (L, V) and dev.flow_trace_bytes == P * 48 + (1 + A) * L * V * 8 + 8
                assert_same_map(got, host, OUTPUTS + ("action",))
        mass, attributes = pc.carried(P, 3, 2)
        k = flow.push_scales(mass, attributes, w) - 8
        whole = dev.flow_trace(tri, w, nbr, fc.FLOOR, span, mass=mass, attributes=attributes, exponents=k, layers="all", max_crossings=max_crossings)
        pc.assert_pushed_equals(whole["mass_at"], whole["attr_at"], whole["dropped"], pc.specification(host, t, V, mass, attributes, "all", exponents=k))
        half = P // 2 + 7
        parts = [dev.flow_trace(tri[s], w[s], nbr, fc.FLOOR, span, mass=mass[s], attributes=attributes[:, s], exponents=k, layers="all",
                                max_crossings=max_crossings) for s in (slice(0, half), slice(half, P))]
        assert same(parts[0]["mass_at"] + parts[1]["mass_at"], whole["mass_at"]) and same(parts[0]["attr_at"] + parts[1]["attr_at"], whole["attr_at"])
        assert np.any(parts[0]["mass_at"] != 0.0) and np.any(parts[1]["attr_at"] != 0.0)
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
    got = dev.flow_trace(tri, w, nbr, floor, span, action=True, mass=mass, attributes=attributes, layers="all", trajectory=True)
    mu, E = dev.download("mu"), dev.download("E")
    assert np.any(mu > floor) and np.any(E != 0.0)
    host = flow.flow_map_host(mu, E, geom["triangles"], fc.caller_hat(dev.plan), nbr, tri, w, floor, trajectory=True, span=span, action=True)
    assert np.any(host["crossings"] > 0) and np.any(host["action"] > 0.0)
    assert_same_map(got, host, OUTPUTS + LAYERS + ("action",))
    want = pc.specification(host, geom["triangles"], geom["vertices"].shape[0], mass, attributes, "all")
    pc.assert_pushed_equals(got["mass_at"], got["attr_at"], got["dropped"], want)


def test_trace_carries_out_a_pending_division_and_leaves_the_state_untouched():
    """On the direct solver, with the hints of the driver's loop set: after a step that leaves a penalty division pending the trace
    equals the specification on the downloaded arrays; then k steps, the trace, k steps leave the twelve arrays as 2 k steps without
    it do."""
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
        a.flow_trace(tri, w, nbr, 0.05, (20, 0), action=True, mass=mass, layers="all", trajectory=True)
        for n in STATE:
            assert same(before[n], a.download(n)), n
        for dev in (a, b):
            dev.step(1)
        a.flow_trace(tri, w, nbr, 0.05, (3, 17), action=True)      # (between two steps, nothing read in between)
        for dev in (a, b):
            dev.step(2)
        for n in STATE:
            assert same(a.download(n), b.download(n)), n
    finally:
        a.close()
        b.close()


def test_refusals_leave_the_context_usable():
    geom = meshes.example("plane", n=4)[0]
    dev = stepped(6, geom)
    try:
        tri, w, nbr = starts_on(geom, n=20)
        P = tri.shape[0]
        out = {"triangle": np.empty(P, dtype=np.int32), "weights": np.empty((P, 3)), "status": np.empty(P, dtype=np.int32),
               "rested": np.empty(P, dtype=np.int32), "crossings": np.empty(P, dtype=np.int32), "action": np.empty(P)}
        i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)

        def desc(node_from, node_to):
            d = _lib.FlowTraceDesc()
            d.map.n_particles, d.map.max_crossings, d.map.floor = P, 16, 0.05
            d.map.start_triangle, d.map.start_weights, d.map.neighbours = tri.ctypes.data_as(i32), w.ctypes.data_as(f64), nbr.ctypes.data_as(i32)
            d.map.triangle, d.map.weights = out["triangle"].ctypes.data_as(i32), out["weights"].ctypes.data_as(f64)
            d.map.status, d.map.rested, d.map.crossings = (out[key].ctypes.data_as(i32) for key in ("status", "rested", "crossings"))
            d.node_from, d.node_to, d.action = node_from, node_to, out["action"].ctypes.data_as(f64)
            return d

        assert dev.lib.dots_flow_trace(dev._h, None) == _lib.ERR_ARGUMENT      # a NULL desc
        before = dev.debug_counter(9)
        for nodes in ((-1, 3), (3, -1), (7, 0), (0, 7), (2 ** 31 - 1, 0), (0, 0), (6, 6), (3, 3)):      # outside 0 .. 6, or no interval
            assert dev.lib.dots_flow_trace(dev._h, C.byref(desc(*nodes))) == _lib.ERR_ARGUMENT, nodes
        d = desc(6, 0)
        d.map.weights = None      # what dots_flow_map refuses, on a description that is complete otherwise
        assert dev.lib.dots_flow_trace(dev._h, C.byref(d)) == _lib.ERR_ARGUMENT
        d = desc(6, 0)
        d.map.n_particles = 0
        assert dev.lib.dots_flow_trace(dev._h, C.byref(d)) == _lib.ERR_ARGUMENT
        assert dev.debug_counter(9) == before      # (nothing ran)
        with pytest.raises(ValueError, match="span"):      # (the wrapper refuses them before the call)
            dev.flow_trace(tri, w, nbr, 0.05, (0, 7))
        assert dev.lib.dots_flow_trace(dev._h, C.byref(desc(6, 0))) == 0      # the complete description is served
        dev.step(1)                                                            # and the context still steps
        check_against_host(dev, geom, (6, 0))
        check_against_host(dev, geom, (2, 5))
    finally:
        dev.close()
    from dots_socp_amd.device import DeviceProblem

    slab = DeviceProblem(7, geom, lap_solver="modal_pcg", time_slab=(0, 2))
    try:
        with pytest.raises(ValueError, match="time slabs"):
            slab.flow_trace(tri, w, nbr, 0.05, (7, 0))
        assert slab.lib.dots_flow_trace(slab._h, C.byref(desc(6, 0))) == _lib.ERR_STATE
        assert slab.download("mu").shape == slab.shape("mu")
    finally:
        slab.close()


def test_backward_map_round_trip_and_action_of_the_translated_bump():
    """The plane example moves a bump from (0.4, 0.4) to (0.6, 0.6); one solve, then several flow_map calls.  The fp64 oracle with the
    specification (test_flow_span_cpu.py asserts these on it) gives: backward from the 65 vertices that carry a tenth of the largest
    density of mu1 or more, an error against the translation by (-0.2, -0.2, 0) of 0.0307 at worst and 0.0114 on average, none of them
    resting or stopping -- the bounds are 1.5 times these, 0.0461 and 0.0171: room for an iterate that agrees with the oracle's to 1e-6
    but not in its bits, not for another definition --; the 69 dense vertices of mu0 traced forward and then backward from their end
    points return to 6.0e-16 (bound 1e-12); sum(mass * action) / (2 * cost) is 0.9419 forward with mu0 and 0.9420 backward with mu1
    (bound: within 0.01 of 0.9419 -- such an iterate moves it in the sixth digit, another definition would not fit).
    Measured on an MI355X: backward 0.0307 and 0.0114, round trip 4.3e-16, ratios 0.941916 and 0.941965 at a cost of 0.038163."""
    from dots_socp_amd.socp.solver_socp import AlmSolver

    T = 15
    geom, scale = meshes.example("plane", n=20)
    v, t = geom["vertices"], geom["triangles"]
    alm = AlmSolver(T, geom, tol=1e-4, nit=5000)
    try:
        for _ in range(5000):
            if alm.iterate():
                break
        _, hist = alm.finalize(download=False)
        cost = float(hist.history["Transportation cost"][-1])
        calls = []

        def trace(starts, span, action):
            calls.append(alm.flow_map(starts=starts, span=span, action=action))
            return calls[-1]

        fig = sc.plane_figures(trace, geom, scale, cost)
        print(f"plane example on the device: backward error over {fig['dense_mu1']} vertices: max {fig['backward_max']:.4f}, mean {fig['backward_mean']:.4f}; "
              f"round trip of {fig['dense_mu0']} vertices {fig['round_trip']:.1e}; action / (2 cost): forward {fig['ratio_forward']:.6f}, backward "
              f"{fig['ratio_backward']:.6f}; cost {cost:.6f}; device ms {[round(c['ms'], 3) for c in calls]}")
        assert fig["dense_mu0"] == sc.PLANE_DENSE_MU0 and fig["dense_mu1"] == sc.PLANE_DENSE_MU1
        assert fig["backward_clean"] and fig["round_trip_clean"]
        assert fig["backward_max"] < 0.0461 and fig["backward_mean"] < 0.0171
        assert fig["round_trip"] <= 1e-12
        assert abs(fig["ratio_forward"] - 0.9419) <= 0.01 and abs(fig["ratio_backward"] - 0.9419) <= 0.01
        # what the result holds at a span, and the push back onto mu0
        forward, backward = calls[0], calls[1]
        assert forward["span"] == (0, T) and np.array_equal(forward["nodes"], np.arange(T + 1)) and "action" not in calls[2]
        assert backward["span"] == (T, 0) and np.array_equal(backward["nodes"], np.arange(T, -1, -1)) and "pushed" not in backward
        got = alm.flow_map(starts="vertices", span=(T, 0), action=True, trajectory=True, push={"layers": "all"})
        assert_same_map(got, backward, OUTPUTS + ("action",))
        assert got["positions_at"].shape == (T + 1, v.shape[0], 3) and same(got["positions_at"][0], v) and same(got["positions_at"][-1], got["positions"])
        pushed = got["pushed"]
        assert "to_mu1" not in pushed and pushed["mass"].shape == (T + 1, v.shape[0]) and pushed["dropped"] == 0
        assert np.max(np.abs(pushed["mass"][0] - geom["mu1"])) < 1e-15 and np.max(np.abs(pushed["mass"].sum(axis=1) - 1.0)) < 1e-12
        print(f"mu1 pushed back: L1 to mu0 {pushed['to_mu0']['l1']:.4f}")
        mid = alm.flow_map(starts="vertices", span=(7, T), push={"mass": geom["mu0"]})
        assert set(mid["pushed"]) >= {"to_mu1"} and "to_mu0" not in mid["pushed"] and np.array_equal(mid["nodes"], np.arange(7, T + 1))
        with pytest.raises(ValueError, match="interior node 7"):
            alm.flow_map(starts="vertices", span=(7, 0), push=True)
        # the backward map as a texture pull: the source coordinates pulled onto the target are the landing points
        assert same(flow.pull_back(v, backward, t), flow.positions(v, t, backward["triangle"], backward["weights"]))
        # and the same calls equal the specification on the downloaded arrays, bit for bit
        dev = alm.dev
        mu, E = dev.download("mu"), dev.download("E")
        tri, w = flow.vertex_starts(t, v.shape[0])
        floor = 1e-3 * float(np.max(geom["mu0"] / (geom["area_vertices"] / 3.0))) / (alm.r * alm.dual_scale)
        want = flow.flow_map_host(mu, E, t, fc.caller_hat(dev.plan), flow.triangle_neighbours(t), tri, w, floor, trajectory=True, span=(T, 0), action=True)
        assert_same_map(got, want, OUTPUTS + LAYERS + ("action",))
    finally:
        alm.close()

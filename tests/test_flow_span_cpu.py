"""The trace between two time nodes on the host (dots_socp_amd/flow.py: flow_map_host with ``span`` and ``action``, pull_back,
push_forward_host at a span): the default keeps its bits, spans compose, backward traces undo forward ones, the action of a known
motion, the option checks, and the figures of the plane example on the fp64 oracle that bound the device in test_hip_flow_span.py."""
import hashlib
import math

import numpy as np
import pytest

import flow_checks as fc
import span_checks as sc
from dots_socp_amd import flow, meshes
from dots_socp_amd.geometry import hat_gradients

SHORT = [name for name in fc.CASES if fc.CASES[name][1] <= 7]
KEYS = ("triangle", "weights", "status", "rested", "crossings", "triangles_at", "weights_at")

# sha256 over the arrays of KEYS, in that order, of flow_map_host(..., trajectory=True) on flow_checks.particles(name, 200) as it was
# before it took a span (computed with the function of the commit before)
BEFORE = {
    "tetrahedron": "afa0818b4a1c39f4520046da31137048e7e4dc40d36942ca3f2213d0f7a79579",
    "strip": "72b458326e7723bbe1562e4164cc808d77980ccd2587cf1f76e8d52b5c4fd2e1",
    "icosphere1": "0cb9b5fe7b1087eda199b064cda6ae1b2b341c35c3b9b8353c6ba287c354c1c3",
    "torus": "6a71a9210fa875b0684dbe0a610a74e21b2750ed7b3ac3e8b48d2ee19e187b68",
    "plane4": "74c8f100982561c0c60e5e23cfd9a4b7df893fc92b23d35759a6d13e67bb7a08",
}


def case(name, count=200):
    v, t = fc.mesh_of(name)
    _, hat = hat_gradients(v, t)
    mu, E = fc.random_state(name)
    tri, w = fc.particles(name, count)
    return v, t, hat, flow.triangle_neighbours(t), mu, E, tri, w


def digest(result):
    h = hashlib.sha256()
    for key in KEYS:
        h.update(np.ascontiguousarray(result[key]).tobytes())
    return h.hexdigest()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", SHORT)
def test_the_default_keeps_its_bits_and_the_whole_span_equals_it(name):
    v, t, hat, nbr, mu, E, tri, w = case(name)
    T, mc = fc.CASES[name][1], fc.CASES[name][4]
    plain = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings=mc, trajectory=True)
    assert set(plain) == set(KEYS) and digest(plain) == BEFORE[name]
    whole = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings=mc, trajectory=True, span=(0, T), action=True)
    assert set(whole) == set(KEYS) | {"action"} and digest(whole) == BEFORE[name]
    assert whole["action"].shape == (tri.shape[0],) and np.all(whole["action"] >= 0.0) and np.any(whole["action"] > 0.0)
    short = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings=mc, span=(0, T))
    assert set(short) == set(KEYS[:5]) and all(same(short[key], plain[key]) for key in KEYS[:5])


@pytest.mark.parametrize("name", ["icosphere1", "torus", "plane4"])
def test_spans_compose(name):
    """(0, k) and then (k, T) from its end points is (0, T), bit for bit, for every particle that the first leg did not stop (a stopped
    one stays where it is in one trace and would set off again as a new start); the counters and the actions add."""
    v, t, hat, nbr, mu, E, tri, w = case(name)
    T, mc = fc.CASES[name][1], fc.CASES[name][4]
    kw = dict(max_crossings=mc, trajectory=True, action=True)
    whole = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, span=(0, T), **kw)
    for k in (1, T - 1):
        first = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, span=(0, k), **kw)
        assert first["triangles_at"].shape == (k + 1, tri.shape[0]) and same(first["triangles_at"], whole["triangles_at"][:k + 1])
        assert same(first["weights_at"], whole["weights_at"][:k + 1])
        second = flow.flow_map_host(mu, E, t, hat, nbr, first["triangle"], first["weights"], fc.FLOOR, span=(k, T), **kw)
        assert second["weights_at"].shape == (T - k + 1, tri.shape[0], 3)
        on = first["status"] == 0
        assert int(on.sum()) > tri.shape[0] // 2 and (name != "plane4" or not np.all(on))
        for key in ("triangle", "weights", "status"):
            assert same(second[key][on], whole[key][on]), (k, key)
        assert same(second["triangles_at"][:, on], whole["triangles_at"][k:, on]) and same(second["weights_at"][:, on], whole["weights_at"][k:, on])
        for key in ("rested", "crossings"):
            assert np.array_equal((first[key] + second[key])[on], whole[key][on]), (k, key)
        assert np.max(np.abs((first["action"] + second["action"])[on] - whole["action"][on])) <= 1e-15
        for key in ("triangle", "weights", "rested", "crossings", "action"):      # (the stopped ones: the whole trace ends where the first leg did)
            assert same(first[key][~on], whole[key][~on]), (k, key)
        assert np.all(whole["status"][~on] == 1)


@pytest.mark.parametrize("name", list(sc.BACKWARD_RULES) + ["strip"])
def test_backward_cases_exercise_every_rule(name):
    """What test_hip_flow_span.py relies on: the backward trace over (T, 0) of every case holds a rest, a floored triangle, two free
    crossings in one interval and, on the open plane, a stop at the boundary; the strip stops but never rests."""
    v, t, hat, nbr, mu, E, tri, w = case(name, max(fc.COUNTS))
    T, mc = fc.CASES[name][1], fc.CASES[name][4]
    host = sc.host_reference(mu, E, t, hat, nbr, tri, w, fc.FLOOR, mc, (T, 0))
    seen = sc.exercised(name, mu, t, host, (T, 0))
    if name == "strip":
        assert seen["stopped"] and not seen["rested"], seen
    else:
        assert seen == sc.BACKWARD_RULES[name], seen
    assert host["triangles_at"].shape == (T + 1, tri.shape[0])
    forward = sc.host_reference(mu, E, t, hat, nbr, tri, w, fc.FLOOR, mc, (0, T))
    assert not same(forward["weights"], host["weights"])


@pytest.mark.parametrize("name,at_least", [("tetrahedron", 200), ("icosphere1", 40)])
def test_backward_undoes_forward_where_nothing_is_floored(name, at_least):
    """floor = 0.0 (a floored triangle is a sink: with FLOOR the particles do not return).  Every particle that neither rests nor stops
    going forward neither rests nor stops on the way back, returns to its start and has spent the same action.  The reference gives
    286 such particles on the tetrahedron and 50 on icosphere1, each back to 7e-16."""
    v, t, hat, nbr, mu, E, tri, w = case(name, 400)
    T, mc = fc.CASES[name][1], fc.CASES[name][4]
    forward = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, 0.0, max_crossings=mc, span=(0, T), action=True)
    free = (forward["status"] == 0) & (forward["rested"] == 0)
    assert int(free.sum()) >= at_least
    back = flow.flow_map_host(mu, E, t, hat, nbr, forward["triangle"][free], forward["weights"][free], 0.0, max_crossings=mc, span=(T, 0), action=True)
    assert np.all(back["status"] == 0) and np.all(back["rested"] == 0)
    home = flow.positions(v, t, back["triangle"], back["weights"])
    off = np.max(np.linalg.norm(home - flow.positions(v, t, tri, w)[free], axis=1))
    print(f"{name}: {int(free.sum())} particles return to {off:.1e}")
    assert off <= 1e-12
    assert np.max(np.abs(back["action"] - forward["action"][free])) <= 1e-12 and np.any(forward["action"][free] > 0.1)


def test_constant_velocity_spends_its_speed_squared_and_goes_back():
    """mu = 1 and E = (a, b, 0) on the plane: the action of a particle is |u|^2 times the time it moved -- all of the span if it stays
    inside, the part before it stopped otherwise (the distance it covered over the speed) --, and backward it moves by -(a, b, 0)."""
    v, t = meshes.plane(6)
    a, b, T = 0.13, 0.21, 4
    _, hat = hat_gradients(v, t)
    nbr = flow.triangle_neighbours(t)
    tri, w = flow.vertex_starts(t, v.shape[0])
    mu, E = np.ones((T, v.shape[0])), np.broadcast_to(np.array([a, b, 0.0]), (T + 1, t.shape[0], 3)).copy()
    uu = a * a + b * b
    for span, sign in (((0, T), 1.0), ((T, 0), -1.0), ((1, 3), 1.0), ((3, 1), -1.0)):
        out = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, floor=0.0, span=span, action=True)
        duration = abs(span[1] - span[0]) / T
        moved = flow.positions(v, t, out["triangle"], out["weights"]) - v
        inside = out["status"] == 0
        assert 5 < int(inside.sum()) < v.shape[0] and np.all(out["rested"] == 0)
        assert np.max(np.abs(moved[inside] - sign * duration * np.array([a, b, 0.0]))) < 1e-13
        assert np.max(np.abs(out["action"][inside] - uu * duration)) < 1e-15
        spent = np.linalg.norm(moved[~inside], axis=1) / math.sqrt(uu)      # the time before the stop
        assert np.all(spent < duration) and np.max(np.abs(out["action"][~inside] - uu * spent)) < 1e-14


def test_pull_back_interpolates_at_the_landing_points():
    t = np.array([[0, 1, 2], [1, 3, 2]])
    result = {"triangle": np.array([1, 0, 1], dtype=np.int32), "weights": np.array([[0.5, 0.25, 0.25], [0.0, 1.0, 0.0], [0.125, 0.125, 0.75]])}
    x = np.array([[1.0, -1.0], [2.0, 10.0], [4.0, 100.0], [8.0, 1000.0]])
    want = np.array([[0.5 * 2 + 0.25 * 8 + 0.25 * 4, 0.5 * 10 + 0.25 * 1000 + 0.25 * 100], [2.0, 10.0],
                     [0.125 * 2 + 0.125 * 8 + 0.75 * 4, 0.125 * 10 + 0.125 * 1000 + 0.75 * 100]])
    assert np.array_equal(flow.pull_back(x, result, t), want)
    assert np.array_equal(flow.pull_back(x[:, 1], result, t), want[:, 1])
    v, tri = meshes.plane(3)
    starts = flow.vertex_starts(tri, v.shape[0])
    assert np.array_equal(flow.pull_back(v, {"triangle": starts[0], "weights": starts[1]}, tri), v)      # (a map that stays pulls a field onto itself)
    with pytest.raises(ValueError, match="pull_back"):
        flow.pull_back(x, {"triangle": result["triangle"], "weights": result["weights"][:2]}, t)


@pytest.mark.parametrize("span", [(5, 0), (4, 1), (1, 4)])
@pytest.mark.parametrize("layers", ["end", "all"])
def test_push_at_a_span_equals_a_direct_sum_in_python_integers(span, layers):
    name = "torus"
    v, t, hat, nbr, mu, E, tri, w = case(name, 120)
    V, n = v.shape[0], abs(span[1] - span[0])
    host = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, trajectory=True, span=span)
    rng = np.random.default_rng(5)
    mass, attributes = 0.1 + rng.random(120), rng.standard_normal((2, 120))
    k = flow.push_scales(mass, attributes, w)
    got = flow.push_forward_host(host, t, V, mass, attributes, k, layers)
    L = n + 1 if layers == "all" else 1
    assert got["mass"].shape == (L, V) and got["attributes"].shape == (2, L, V) and got["dropped"] == 0
    tri_at, w_at = (host["triangles_at"], host["weights_at"]) if layers == "all" else (host["triangle"][None], host["weights"][None])
    g = np.concatenate([mass[None], mass[None] * attributes])
    want = np.zeros((3, L, V), dtype=object)
    for c in range(3):
        q = np.rint((g[c][None, :, None] * w_at) * math.ldexp(1.0, int(k[c]))).astype(np.int64).astype(object)
        for corner in range(3):
            np.add.at(want[c], (np.arange(L)[:, None], t[tri_at][:, :, corner]), q[:, :, corner])
    assert np.array_equal(got["integers"].astype(object), want) and any(int(x) != 0 for x in want.reshape(-1))
    for c in range(3):
        out = got["mass"] if c == 0 else got["attributes"][c - 1]
        assert np.array_equal(out, want[c].astype(np.float64) * math.ldexp(1.0, -int(k[c])))


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the HIP library fails the test: the refusals must come first."""
    from dots_socp_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", refuse)


def test_bad_span_requests_are_refused_before_the_library(no_library):
    from dots_socp_amd import socp
    from dots_socp_amd.socp.solver_socp import FLOW_MAP_KEYS, check_flow_map

    assert "span" in FLOW_MAP_KEYS and "action" in FLOW_MAP_KEYS
    geom, _ = meshes.example("sphere", level=1)
    points = (np.zeros(3, dtype=np.int32), np.full((3, 3), 1.0 / 3.0))
    bad = [({"span": 3}, "span"), ({"span": (0,)}, "span"), ({"span": (0, 1, 2)}, "span"), ({"span": (0.0, 15)}, "span"), ({"span": (True, 3)}, "span"),
           ({"span": (4, 4)}, "equals"), ({"span": (-1, 4)}, "outside"), ({"span": (0, 16)}, "outside"), ({"span": (16, 0)}, "outside"),
           ({"action": "yes"}, "action"), ({"action": 1}, "action"),
           ({"span": (7, 15), "push": True}, "interior node 7"), ({"span": (7, 0), "push": {"layers": "all"}}, "interior node 7"),
           ({"span": (15, 0), "starts": points, "push": True}, "mass per particle")]
    for spec, match in bad:
        for plug_in in (socp.solver, socp.solver_raw, socp.solver_cascade):
            with pytest.raises(ValueError, match=match):
                plug_in(15, geom, flow_map=spec)
        with pytest.raises(ValueError, match=match):
            socp.solver_raw_many(15, geom, [{}], flow_map=spec)
        with pytest.raises(ValueError, match=match):
            socp.solver_mesh_cascade(15, [geom, geom], flow_map=spec)
        with pytest.raises(ValueError, match=match):
            check_flow_map(spec, n_time=15)
    for spec in ({"span": (15, 0)}, {"action": True}, {"span": (3, 9), "action": True}):
        with pytest.raises(ValueError, match="time slabs"):
            socp.solver(15, geom, flow_map=spec, time_slab=(0, 2))
    # without n_time the range is left to the solver, the rest is refused all the same
    assert check_flow_map({"span": (0, 16)}) == {"span": (0, 16)}
    with pytest.raises(ValueError, match="interior node 7"):
        check_flow_map({"span": (7, 15), "push": True})
    with pytest.raises(ValueError, match="equals"):
        check_flow_map({"span": (4, 4)})
    good = [{"span": (15, 0)}, {"span": (0, 15), "action": True}, {"span": (15, 0), "push": True}, {"span": (0, 7), "push": {"layers": "all"}},
            {"span": (7, 3), "action": True, "push": {"mass": np.ones(42)}}, {"span": (7, 15), "starts": points, "push": {"mass": np.ones(3)}},
            {"action": True}, {"span": None, "action": False}, {"span": [np.int64(2), 5]}]
    for spec in good:
        assert check_flow_map(spec, n_time=15) == spec
    for span in ((0, 0), (3, 8), (8.0, 3), "all"):
        with pytest.raises(ValueError, match="span"):
            flow.flow_map_host(np.ones((7, 4)), np.zeros((8, 4, 3)), fc.tetrahedron()[1], np.zeros((4, 3, 3)), np.zeros((4, 3), dtype=np.int32),
                               [0], [[1.0, 0.0, 0.0]], 0.0, span=span)


@pytest.fixture(scope="module")
def plane_by_the_oracle():
    """The plane example solved by the fp64 oracle (run to convergence: 1 248 iterations, about 15 s) and traced by the specification."""
    from conftest import load_oracle

    geom, scale = meshes.example("plane", n=20)
    sol, hist = load_oracle().solver_socp(15, geom, tol=1e-4, nit=5000)
    v, t = geom["vertices"], geom["triangles"]
    _, hat = hat_gradients(v, t)
    nbr = flow.triangle_neighbours(t)
    floor = 1e-3 * float(np.max(geom["mu0"] / (geom["area_vertices"] / 3.0)))      # (the default of AlmSolver.flow_map)

    def trace(starts, span, action):
        return flow.flow_map_host(sol["mu"], sol["E"], t, hat, nbr, starts[0], starts[1], floor, span=span, action=action)

    return sc.plane_figures(trace, geom, scale, hist.history["Transportation cost"][-1])


def test_plane_figures_of_the_oracle(plane_by_the_oracle):
    """The figures the device test's bounds rest on, at the printed digits +- 1 in the last: the backward map against the translation
    by (-0.2, -0.2, 0), the round trip of the dense vertices of mu0, and sum(mass * action) / (2 * cost) in both directions."""
    fig = plane_by_the_oracle
    print(fig)
    assert fig["dense_mu0"] == sc.PLANE_DENSE_MU0 and fig["dense_mu1"] == sc.PLANE_DENSE_MU1
    assert fig["backward_clean"] and fig["round_trip_clean"]
    for got, printed in ((fig["backward_max"], sc.PLANE_BACKWARD_MAX), (fig["backward_mean"], sc.PLANE_BACKWARD_MEAN),
                         (fig["ratio_forward"], sc.PLANE_ACTION_RATIO_FORWARD), (fig["ratio_backward"], sc.PLANE_ACTION_RATIO_BACKWARD)):
        assert abs(round(got, 4) - printed) < 1.5e-4, (got, printed)
    assert fig["round_trip"] <= 1e-15      # (6.0e-16, in the units of the geometry's vertices)

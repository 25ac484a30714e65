"""The sliding mode of the flow map on the host (dots_socp_amd/flow.py: flow_map_host with ``slide`` and ``areas``): off keeps its bits,
the known answer on two triangles that push a particle at each other, the invariants on the random cases, spans and the push with
slides, the option checks, and the figures of the plane example on the fp64 oracle."""
import math

import numpy as np
import pytest

import flow_checks as fc
import slide_checks as sl
from dots_socp_amd import flow, meshes
from dots_socp_amd.geometry import hat_gradients
from test_flow_span_cpu import BEFORE, KEYS, digest, same


@pytest.mark.parametrize("name", sl.SHORT)
def test_off_keeps_its_bits(name):
    v, t, areas, hat, nbr, mu, E, tri, w = sl.case(name)
    mc = fc.CASES[name][4]
    for kw in ({}, {"slide": False}, {"slide": False, "areas": areas}, {"slide": False, "areas": areas, "tally": {}}):
        off = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings=mc, trajectory=True, **kw)
        assert set(off) == set(KEYS) and digest(off) == BEFORE[name], kw
    on = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings=mc, trajectory=True, slide=True, areas=areas)
    assert set(on) == set(KEYS) | {"slides", "steps"} and digest(on) != BEFORE[name]
    assert on["slides"].dtype == np.int32 and on["steps"].dtype == np.int32 and on["slides"].shape == on["steps"].shape == (tri.shape[0],)


@pytest.mark.parametrize("a,b,p,r", [(0.5, 0.3, 0.2, 0.4), (0.5, 0.3, -0.3, -0.1)])
def test_known_answer_on_two_triangles(a, b, p, r):
    """The end point is the entry point plus (b p + a r) / (a + b) times the time left, along the edge; the action is the two legs'
    time * speed^2.  The two choices slide towards vertex 2 and towards vertex 1."""
    args, areas, entry, left, end, act = sl.strip_problem(a, b, p, r)
    v, t = fc.strip()
    off = flow.flow_map_host(*args, action=True)
    assert off["rested"][0] == 1 and off["crossings"][0] == 16
    assert np.max(np.abs(flow.positions(v, t, off["triangle"], off["weights"])[0] - entry)) <= 1e-14      # (it rests where it entered)
    tally = {}
    on = flow.flow_map_host(*args, action=True, slide=True, areas=areas, tally=tally)
    got = flow.positions(v, t, on["triangle"], on["weights"])[0]
    speed = (b * p + a * r) / (a + b)
    assert (speed > 0.0) == (p > 0.0) and abs(speed) * left > 0.1      # (the slide is no rounding matter, and the two choices differ in sign)
    print(f"end point off by {np.max(np.abs(got - end)):.1e}, action by {abs(on['action'][0] - act):.1e}")
    assert np.max(np.abs(got - end)) <= 1e-14
    assert on["slides"][0] == 1 and on["rested"][0] == 0 and on["status"][0] == 0 and on["crossings"][0] == 1 and on["steps"][0] == 2
    assert on["triangle"][0] == 1 and on["weights"][0, 1] == 0.0      # (on the edge, in the triangle entered: no weight on vertex 3)
    assert abs(on["action"][0] - act) <= 1e-14
    assert tally == {"done": 1, "passed_on": 0, "vertex_rest": 0, "cap": 0}


def test_a_slide_into_a_vertex_of_two_triangles_rests_there():
    """p large: the slide reaches vertex 2 before the interval ends; triangle 1 moves the particle on along the edge (r > 0) but not
    round the vertex (r < b), and there is no third triangle: it rests at the vertex with the weights exactly (1, 0) on the edge."""
    a, b, p, r = 0.5, 0.3, 3.0, 0.2
    args, areas, entry, left, end, _ = sl.strip_problem(a, b, p, r, start=(0.02, 0.49, 0.49))
    assert np.dot(end - np.array([0.0, 1.0, 0.0]), sl.STRIP_TANGENT) > 0.1      # (unbounded, the slide would pass vertex 2)
    tally = {}
    on = flow.flow_map_host(*args, slide=True, areas=areas, tally=tally)
    assert on["slides"][0] == 1 and on["rested"][0] == 1 and on["status"][0] == 0
    assert on["triangle"][0] == 1 and on["weights"][0].tolist() == [0.0, 0.0, 1.0]      # triangle 1 = (1, 3, 2): all of it on vertex 2
    assert tally == {"done": 0, "passed_on": 0, "vertex_rest": 1, "cap": 0}


CAPPED = [(name, fc.CASES[name][4]) for name in sl.SHORT] + [("torus", 2)]


@pytest.fixture(scope="module")
def tallies():
    return {}


@pytest.mark.parametrize("name,mc", CAPPED, ids=[f"{n}-{c}" for n, c in CAPPED])
def test_invariants_on_the_random_cases(name, mc, tallies):
    v, t, areas, hat, nbr, mu, E, tri, w = sl.case(name)
    T = fc.CASES[name][1]
    off = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings=mc, trajectory=True)
    tally = {}
    on = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings=mc, trajectory=True, slide=True, areas=areas, tally=tally)
    tallies[(name, mc)] = tally
    moved = int(sl.moved(on, off).sum())
    print(f"{name} cap {mc}: rested {int(off['rested'].sum())} -> {int(on['rested'].sum())}, slides {int(on['slides'].sum())} {tally}, "
          f"most turns {int(on['steps'].max())}, moved {moved}")
    assert np.all(np.isfinite(on["weights_at"])) and np.all(on["weights_at"] >= 0.0)
    sums = sl.weight_sums(on["weights_at"])
    assert np.max(np.abs(sums - sums[0])) <= 1e-12
    assert np.all(on["steps"] <= T * (mc + 1) + on["slides"]) and np.all(on["steps"] >= 1)
    assert sum(tally.values()) == int(on["slides"].sum()) > 0
    assert 2 * int(on["rested"].sum()) <= int(off["rested"].sum())
    if mc == 16:
        assert tally["done"] > 0 and tally["passed_on"] > 0 and tally["vertex_rest"] > 0, tally
        if name in sl.MOVED:
            assert moved >= 100


def test_every_way_a_slide_ends_occurs(tallies):
    """(after the cases above: the cap inside step 3a is not reached at 16, the torus at a cap of 2 reaches it)"""
    assert set(tallies) == set(CAPPED)
    total = {key: sum(t[key] for t in tallies.values()) for key in flow.SLIDE_ENDS}
    assert all(total[key] > 0 for key in flow.SLIDE_ENDS), total
    assert tallies[("torus", 2)]["cap"] > 0


@pytest.mark.parametrize("name", ["icosphere1", "torus", "plane4"])
def test_spans_compose_and_backward_slides(name):
    """(0, k) and then (k, T) from its end points is (0, T), bit for bit, for every particle the first leg did not stop; the counters
    add.  A backward span runs, slides, and is not the forward one."""
    v, t, areas, hat, nbr, mu, E, tri, w = sl.case(name)
    T, mc = fc.CASES[name][1], fc.CASES[name][4]
    kw = dict(max_crossings=mc, trajectory=True, action=True, slide=True, areas=areas)
    whole = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, span=(0, T), **kw)
    plain = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings=mc, trajectory=True, slide=True, areas=areas)
    assert all(same(plain[key], whole[key]) for key in plain) and np.any(whole["slides"] > 0)
    for k in (1, T - 1):
        first = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, span=(0, k), **kw)
        assert same(first["triangles_at"], whole["triangles_at"][:k + 1]) and same(first["weights_at"], whole["weights_at"][:k + 1])
        second = flow.flow_map_host(mu, E, t, hat, nbr, first["triangle"], first["weights"], fc.FLOOR, span=(k, T), **kw)
        on = first["status"] == 0
        assert int(on.sum()) > tri.shape[0] // 2
        for key in ("triangle", "weights", "status"):
            assert same(second[key][on], whole[key][on]), (k, key)
        assert same(second["triangles_at"][:, on], whole["triangles_at"][k:, on]) and same(second["weights_at"][:, on], whole["weights_at"][k:, on])
        for key in ("rested", "crossings", "slides", "steps"):
            assert np.array_equal((first[key] + second[key])[on], whole[key][on]), (k, key)
        assert np.max(np.abs((first["action"] + second["action"])[on] - whole["action"][on])) <= 1e-14
    back = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, span=(T, 0), **kw)
    assert back["triangles_at"].shape == (T + 1, tri.shape[0]) and int(back["slides"].sum()) > 10 and not same(back["weights"], whole["weights"])
    off = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, max_crossings=mc, span=(T, 0))
    assert 2 * int(back["rested"].sum()) <= int(off["rested"].sum())


@pytest.mark.parametrize("span", [(0, 5), (5, 0), (1, 4)])
@pytest.mark.parametrize("layers", ["end", "all"])
def test_push_on_a_slide_trajectory_equals_a_direct_sum_in_python_integers(span, layers):
    v, t, areas, hat, nbr, mu, E, tri, w = sl.case("torus", 120)
    V, n = v.shape[0], abs(span[1] - span[0])
    host = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, trajectory=True, span=span, slide=True, areas=areas)
    assert np.any(host["slides"] > 0)
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


def test_bad_slide_requests_are_refused_before_the_library(no_library):
    from dots_socp_amd import socp
    from dots_socp_amd.socp.solver_socp import FLOW_MAP_KEYS, check_flow_map

    assert "slide" in FLOW_MAP_KEYS
    geom, _ = meshes.example("sphere", level=1)
    for value in (1, 0, "yes", None, [True]):
        spec = {"slide": value}
        for plug_in in (socp.solver, socp.solver_raw, socp.solver_cascade):
            with pytest.raises(ValueError, match="slide"):
                plug_in(15, geom, flow_map=spec)
        with pytest.raises(ValueError, match="slide"):
            socp.solver_raw_many(15, geom, [{}], flow_map=spec)
        with pytest.raises(ValueError, match="slide"):
            socp.solver_mesh_cascade(15, [geom, geom], flow_map=spec)
        with pytest.raises(ValueError, match="slide"):
            check_flow_map(spec, n_time=15)
    with pytest.raises(ValueError, match="time slabs"):
        socp.solver(15, geom, flow_map={"slide": True}, time_slab=(0, 2))
    for spec in ({"slide": True}, {"slide": False}, {"slide": np.True_, "span": (15, 0), "action": True}, {"slide": True, "push": {"layers": "all"}}):
        assert check_flow_map(spec, n_time=15) == spec
    v, t = fc.tetrahedron()
    args = (np.ones((7, 4)), np.zeros((8, 4, 3)), t, np.zeros((4, 3, 3)), np.zeros((4, 3), dtype=np.int32), [0], [[1.0, 0.0, 0.0]], 0.0)
    for areas in (None, np.ones(3), np.ones((4, 1))):
        with pytest.raises(ValueError, match="areas"):
            flow.flow_map_host(*args, slide=True, areas=areas)
    assert "slides" not in flow.flow_map_host(*args, slide=False)


@pytest.fixture(scope="module")
def plane_by_the_oracle():
    """The plane example on the fp64 oracle after 30 iterations and run to convergence (1 248 iterations, about 15 s), each traced by
    the specification without and with slide from the vertex starts with the default floor."""
    from conftest import load_oracle

    geom, scale = meshes.example("plane", n=20)
    v, t = geom["vertices"], geom["triangles"]
    areas, hat = hat_gradients(v, t)
    nbr = flow.triangle_neighbours(t)
    tri, w = flow.vertex_starts(t, v.shape[0])
    floor = 1e-3 * float(np.max(geom["mu0"] / (geom["area_vertices"] / 3.0)))      # (the default of AlmSolver.flow_map)
    density = geom["mu0"] / (geom["area_vertices"] / 3.0)
    dense = density > 0.1 * density.max()
    out = {"dense": int(dense.sum())}
    for label, nit in (("early", 30), ("converged", 5000)):
        sol, _ = load_oracle().solver_socp(15, geom, tol=1e-4, nit=nit)
        for slide in (False, True):
            res = flow.flow_map_host(sol["mu"], sol["E"], t, hat, nbr, tri, w, floor, slide=slide, areas=areas)
            error = np.linalg.norm((flow.positions(v, t, res["triangle"], res["weights"]) - v) / scale - np.array([0.2, 0.2, 0.0]), axis=1)[dense]
            out[(label, slide)] = {"rested_mass": sl.plane_rested_mass(res, geom["mu0"]), "max": float(error.max()), "mean": float(error.mean())}
    return out


def test_plane_figures_of_the_oracle(plane_by_the_oracle):
    """After 30 iterations the particles that rest carry 9.82e-2 of the mass without slide and 4.46e-3 with it: below a fifth.  On the
    converged solve the worst and the mean error of the map over the 69 dense vertices are 0.0312 and 0.0120 with and without slide
    (+- 1 in the last digit)."""
    fig = plane_by_the_oracle
    print(fig)
    assert fig["dense"] == 69
    off, on = fig[("early", False)]["rested_mass"], fig[("early", True)]["rested_mass"]
    assert off > 0.0 and on < off / 5.0
    assert abs(off / sl.PLANE_RESTED_MASS_30[0] - 1.0) < 5e-3 and abs(on / sl.PLANE_RESTED_MASS_30[1] - 1.0) < 5e-3      # (the printed digits)
    for slide in (False, True):
        got = fig[("converged", slide)]
        assert abs(round(got["max"], 4) - sl.PLANE_FORWARD_MAX) < 1.5e-4 and abs(round(got["mean"], 4) - sl.PLANE_FORWARD_MEAN) < 1.5e-4, (slide, got)
    assert fig[("converged", True)]["rested_mass"] <= fig[("converged", False)]["rested_mass"] <= 1e-6

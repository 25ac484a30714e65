"""The push-forward on the host (dots_socp_amd/flow.py): the specification push_forward_host -- conservation, independence of the order of
the particles, exact addition of parts, dropped contributions --, the exponents of push_scales, the starts on sub-triangles with
their masses, and the refusal of bad ``push`` requests before the library is loaded.  The device side is test_hip_push.py."""
import math
from fractions import Fraction

import numpy as np
import pytest

import push_checks as pc
from dots_socp_amd import flow, meshes


@pytest.fixture(scope="module")
def traced():
    return pc.small_trajectory()


@pytest.mark.parametrize("layers", pc.LAYERS)
def test_every_layer_conserves_what_the_particles_carry(traced, layers):
    """sum_v mass_at[l] equals sum_p m_p wsum_p(l) to within P quanta of 2^-k (a contribution is off by half a quantum at most, and the
    product g * l by a relative 2^-53) -- in exact arithmetic: the integer sums against rationals."""
    host, t, V = traced
    P = host["triangle"].shape[0]
    mass, attributes = pc.carried(P, 4)
    out = pc.specification(host, t, V, mass, attributes, layers)
    k = flow.push_scales(mass, attributes, host["weights_at"][0])
    assert out["dropped"] == 0 and out["integers"].shape == (5, out["mass"].shape[0], V) and out["issued"] > 0
    g = np.concatenate([mass[None], mass[None] * attributes])
    w_at = host["weights_at"] if layers == "all" else host["weights_at"][-1:]
    for c in range(5):
        for l in range(w_at.shape[0]):
            exact = sum(Fraction(float(g[c, p])) * sum(Fraction(float(x)) for x in w_at[l, p]) for p in range(P)) * Fraction(2) ** int(k[c])
            assert abs(sum(int(s) for s in out["integers"][c, l]) - exact) <= P, (c, l)
    # the floating-point result is the integers, scaled back
    assert pc.same(out["mass"], out["integers"][0].astype(np.float64) * math.ldexp(1.0, -int(k[0])))
    assert pc.same(out["attributes"][3], out["integers"][4].astype(np.float64) * math.ldexp(1.0, -int(k[4])))
    assert abs(out["mass"][-1].sum() - math.fsum(mass * host["weights"].sum(axis=1))) < 1e-12


def test_the_order_of_the_particles_does_not_matter(traced):
    host, t, V = traced
    P = host["triangle"].shape[0]
    mass, attributes = pc.carried(P, 4)
    k = flow.push_scales(mass, attributes, host["weights_at"][0])
    whole = flow.push_forward_host(host, t, V, mass, attributes, k, "all")
    order = np.random.default_rng(5).permutation(P)
    moved = {"triangles_at": host["triangles_at"][:, order], "weights_at": host["weights_at"][:, order]}
    again = flow.push_forward_host(moved, t, V, mass[order], attributes[:, order], k, "all")
    assert np.array_equal(whole["integers"], again["integers"]) and pc.same(whole["mass"], again["mass"]) and pc.same(whole["attributes"], again["attributes"])
    assert pc.same(flow.push_scales(mass[order], attributes[:, order], host["weights_at"][0][order]), k)      # (fsum: any order)


def test_two_halves_with_the_same_exponents_add_to_the_whole(traced):
    host, t, V = traced
    P = host["triangle"].shape[0]
    mass, attributes = pc.carried(P, 1)
    k = flow.push_scales(mass, attributes, host["weights_at"][0])
    whole = flow.push_forward_host(host, t, V, mass, attributes, k, "all")
    parts = []
    for part in (slice(0, P // 3), slice(P // 3, P)):
        cut = {"triangles_at": host["triangles_at"][:, part], "weights_at": host["weights_at"][:, part]}
        parts.append(flow.push_forward_host(cut, t, V, mass[part], attributes[:, part], k, "all"))
    assert np.array_equal(parts[0]["integers"] + parts[1]["integers"], whole["integers"])
    assert parts[0]["issued"] + parts[1]["issued"] == whole["issued"]


@pytest.mark.parametrize("level", [1, 2, 3])
def test_triangle_starts_and_their_masses(level):
    geom, _ = meshes.example("sphere", level=1)
    t, V = geom["triangles"], geom["vertices"].shape[0]
    tri, w = flow.triangle_starts(t, level)
    F = t.shape[0]
    assert tri.dtype == np.int32 and tri.shape == (F * level ** 2,) and w.shape == (F * level ** 2, 3)
    assert np.array_equal(np.bincount(tri, minlength=F), np.full(F, level ** 2))
    assert np.all(w > 0.0) and np.max(np.abs(w.sum(axis=1) - 1.0)) <= 2.0 ** -52
    assert np.unique(np.round(w[: level ** 2] * 3 * level).astype(int), axis=0).shape[0] == level ** 2      # distinct points
    if level == 1:
        assert np.array_equal(w, np.full((F, 3), 1.0 / 3.0))
    mass = flow.start_masses(geom["mu0"], geom["area_vertices"], geom["area_triangles"], t, tri, w, level)
    assert abs(mass.sum() - geom["mu0"].sum()) < 1e-15 and np.all(mass >= 0.0)
    vt, vw = flow.vertex_starts(t, V)
    assert np.array_equal(flow.start_masses(geom["mu0"], geom["area_vertices"], geom["area_triangles"], t, vt, vw), geom["mu0"])
    with pytest.raises(ValueError):
        flow.triangle_starts(t, 0)


def test_push_scales():
    w = np.array([[1.0, 0.0, 0.0], [0.25, 0.25, 0.5]])
    assert np.array_equal(flow.push_scales([0.0, 0.0], None, w), [0])                        # B = 0
    assert np.array_equal(flow.push_scales([0.5, 0.5], None, w), [60])                       # B = 1 = 2^0, an exact power of two
    assert np.array_equal(flow.push_scales([0.5, 0.5 + 2.0 ** -52], None, w), [59])          # just above it
    assert np.array_equal(flow.push_scales([2.0 ** 9, 2.0 ** 9], None, w), [50])             # B = 2^10
    assert np.array_equal(flow.push_scales([0.375, 0.375], None, w), [60])                   # 0.75: e = 0
    assert np.array_equal(flow.push_scales([1.0, 1.0], [[0.0, 0.0], [-1.0, 3.0]], w), [59, 0, 58])      # per channel, |g|
    assert np.array_equal(flow.push_scales([1.0, 0.0], None, 3.0 * w), [58])                 # weight sums above 1 count: B = 3
    assert np.array_equal(flow.push_scales([1.0, 0.0], None, 0.5 * w), [60])                 # ... below 1 do not: B = 1
    assert np.array_equal(flow.push_scales([1e-300, 1e-300], [[1e-10, 0.0]], w), [1000, 1000])       # the clip: 60 - e = 1056 and 1089
    assert np.array_equal(flow.push_scales([1e-300, 1e-300], [[1e-300, 0.0]], w), [1000, 0])          # (a product that underflows to 0)
    # (the lower clip cannot be reached: the largest finite bound is below 2^1024, and 60 - 1024 = -964)
    assert np.array_equal(flow.push_scales([1e300, 1e300], [[1.0, 1e7]], w), [60 - 998, 60 - 1020])
    assert flow.push_scales([1.0, 1.0], None, w).dtype == np.int32
    for bad in ([np.nan, 1.0], [np.inf, 1.0]):
        with pytest.raises(ValueError, match="finite"):
            flow.push_scales(bad, None, w)
    with pytest.raises(ValueError, match="finite"):
        flow.push_scales([1e200, 1.0], [[1e200, 1.0]], w)      # (the product overflows)


def test_a_weight_that_is_not_a_number_is_dropped_and_counted(traced):
    host, t, V = traced
    P = host["triangle"].shape[0]
    mass, attributes = pc.carried(P, 1)
    k = flow.push_scales(mass, attributes, host["weights_at"][0])
    clean = flow.push_forward_host(host, t, V, mass, attributes, k, "all")
    broken = {"triangles_at": host["triangles_at"], "weights_at": host["weights_at"].copy()}
    broken["weights_at"][2, 7, 1] = np.nan
    out = flow.push_forward_host(broken, t, V, mass, attributes, k, "all")
    assert out["dropped"] == 2 and clean["dropped"] == 0      # one corner, two channels
    hit = t[host["triangles_at"][2, 7], 1]
    other = np.ones((2, clean["mass"].shape[0], V), dtype=bool)
    other[:, 2, hit] = False
    assert np.array_equal(out["integers"][other], clean["integers"][other]) and np.all(np.isfinite(out["mass"]))
    assert np.all(out["integers"][:, 2, hit] != clean["integers"][:, 2, hit])
    # a contribution of 2^62 quanta or more is dropped as well; one just below is kept
    one = {"triangles_at": np.zeros((1, 1), dtype=np.int32), "weights_at": np.array([[[1.0, 0.0, 0.0]]])}
    assert flow.push_forward_host(one, t, V, [1.0], None, [62], "end")["dropped"] == 1
    kept = flow.push_forward_host(one, t, V, [1.0 - 2.0 ** -53], None, [62], "end")
    assert kept["dropped"] == 0 and kept["issued"] == 1 and kept["integers"][0, 0, t[0, 0]] == 2 ** 62 - 2 ** 9
    assert flow.push_forward_host(one, t, V, [-1.0], None, [61], "end")["integers"][0, 0, t[0, 0]] == -2 ** 61
    # ties go to the even integer
    assert flow.push_forward_host(one, t, V, [2.5], None, [0], "end")["integers"][0, 0, t[0, 0]] == 2
    assert flow.push_forward_host(one, t, V, [-3.5], None, [0], "end")["integers"][0, 0, t[0, 0]] == -4
    with pytest.raises(ValueError, match="finite"):
        flow.push_forward_host(one, t, V, [np.inf], None, [0], "end")
    with pytest.raises(ValueError, match="exponents"):
        flow.push_forward_host(one, t, V, [1.0], None, [1001], "end")


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the HIP library fails the test: the refusals must come first."""
    from dots_socp_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", refuse)


def test_bad_push_requests_are_refused_before_the_library(no_library):
    from dots_socp_amd import socp
    from dots_socp_amd.socp.solver_socp import FLOW_MAP_KEYS, check_flow_map

    assert "push" in FLOW_MAP_KEYS
    geom, _ = meshes.example("sphere", level=1)
    P = geom["vertices"].shape[0]
    bad = [({"push": "yes"}, "push must be"), ({"push": 1}, "push must be"), ({"push": {"layer": "all"}}, "unknown option"),
           ({"push": {"layers": "some"}}, "layers"), ({"push": {"layers": 3}}, "layers"),
           ({"push": {"attributes": np.zeros((5, P))}}, "attributes"), ({"push": {"attributes": np.zeros(P)}}, "attributes"),
           ({"starts": "edges", "push": True}, "starts"), ({"starts": ("triangles", 0)}, "level"), ({"starts": ("triangles", 1.5)}, "level"),
           ({"starts": ("vertices", 2)}, "level"),
           ({"starts": (np.zeros(3, dtype=np.int32), np.full((3, 3), 1.0 / 3.0)), "push": True}, "mass")]
    for spec, match in bad:
        for plug_in in (socp.solver, socp.solver_raw, socp.solver_cascade):
            with pytest.raises(ValueError, match=match):
                plug_in(15, geom, flow_map=spec)
        with pytest.raises(ValueError, match=match):
            socp.solver_raw_many(15, geom, [{}], flow_map=spec)
        with pytest.raises(ValueError, match=match):
            socp.solver_mesh_cascade(15, [geom, geom], flow_map=spec)
    with pytest.raises(ValueError, match="time slabs"):
        socp.solver(15, geom, flow_map={"push": True}, time_slab=(0, 2))
    good = [{"push": True}, {"push": None}, {"starts": "triangles", "push": {"layers": "all"}}, {"starts": ("triangles", 2), "push": {}},
            {"starts": (np.zeros(3, dtype=np.int32), np.full((3, 3), 1.0 / 3.0)), "push": {"mass": np.ones(3)}}]
    for spec in good:
        assert check_flow_map(spec) == spec

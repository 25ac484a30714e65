"""The flow map on the host (dots_socp_amd/flow.py): the neighbour table, the specification flow_map_host on states whose map is known,
the rest rule, the trajectory, and the refusal of time slabs before the library is loaded.  The device side is test_hip_flow.py."""
import numpy as np
import pytest

import flow_checks as fc
from dots_socp_amd import flow, meshes
from dots_socp_amd.geometry import hat_gradients


def fan():
    """three triangles on the edge (0, 1)"""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]])
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 1, 4]], dtype=np.int64)


@pytest.mark.parametrize("mesh,boundary_edges", [(lambda: meshes.plane(3), None), (fc.tetrahedron, 0), (fc.strip, 4)])
def test_triangle_neighbours(mesh, boundary_edges):
    v, t = mesh()
    nbr = flow.triangle_neighbours(t)
    assert nbr.shape == t.shape and nbr.dtype == np.int32
    count = {}
    for tri in t.tolist():
        for k in range(3):
            e = tuple(sorted((tri[(k + 1) % 3], tri[(k + 2) % 3])))
            count[e] = count.get(e, 0) + 1
    for f, tri in enumerate(t.tolist()):
        for k in range(3):
            a, b = tri[(k + 1) % 3], tri[(k + 2) % 3]
            g = int(nbr[f, k])
            assert (g == -1) == (count[tuple(sorted((a, b)))] == 1)      # -1 exactly on boundary edges
            if g >= 0:
                assert g != f and {a, b} <= set(t[g].tolist())
                m = [m for m in range(3) if t[g][m] not in (a, b)]
                assert len(m) == 1 and nbr[g, m[0]] == f                 # symmetric
    if boundary_edges is not None:
        assert int(np.sum(nbr < 0)) == boundary_edges
    flipped = t[:, ::-1]                                                 # orientation does not matter
    assert np.array_equal(flow.triangle_neighbours(flipped), nbr[:, ::-1])


def test_triangle_neighbours_refuses_a_fan():
    with pytest.raises(ValueError, match="3 triangles"):
        flow.triangle_neighbours(fan()[1])


def test_vertex_starts_and_positions():
    v, t = meshes.plane(3)
    tri, w = flow.vertex_starts(t, v.shape[0])
    assert tri.dtype == np.int32 and w.shape == (v.shape[0], 3)
    for i in range(v.shape[0]):
        incident = [f for f in range(t.shape[0]) if i in t[f]]
        assert tri[i] == min(incident) and t[tri[i]][int(np.argmax(w[i]))] == i and sorted(w[i]) == [0.0, 0.0, 1.0]
    assert np.array_equal(flow.positions(v, t, tri, w), v)
    with pytest.raises(ValueError, match="without a triangle"):
        flow.vertex_starts(t, v.shape[0] + 1)


def constant_state(T, V, F, velocity):
    return np.ones((T, V)), np.broadcast_to(np.asarray(velocity, dtype=np.float64), (T + 1, F, 3)).copy()


def test_constant_velocity_translates():
    """mu = 1 and E = (a, b, 0) on the plane: every particle that stays inside moves by (a, b, 0); the others stop on a boundary edge."""
    v, t = meshes.plane(6)
    a, b, T = 0.13, 0.21, 4      # (no edge direction of the tiling: 0, 60 and 120 degrees)
    _, hat = hat_gradients(v, t)
    nbr = flow.triangle_neighbours(t)
    tri, w = flow.vertex_starts(t, v.shape[0])
    mu, E = constant_state(T, v.shape[0], t.shape[0], (a, b, 0.0))
    out = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, floor=0.0)
    end = flow.positions(v, t, out["triangle"], out["weights"])
    inside = out["status"] == 0
    assert 5 < int(inside.sum()) < v.shape[0] and np.all(out["rested"] == 0)
    assert np.max(np.abs(end[inside] - v[inside] - np.array([a, b, 0.0]))) < 1e-13
    for p in np.flatnonzero(~inside):
        assert out["status"][p] == 1
        on_edge = [k for k in range(3) if out["weights"][p, k] == 0.0 and nbr[out["triangle"][p], k] < 0]
        assert on_edge, p


def test_rotation_on_the_sphere_keeps_the_weights():
    v, t = meshes.icosphere(2)
    T = 8
    _, hat = hat_gradients(v, t)
    centroid = v[t].mean(axis=1)
    spin = np.cross(np.array([0.0, 0.0, 1.0]), centroid)      # rotation about the axis, angle 1 over the unit time
    mu = np.ones((T, v.shape[0]))
    E = np.broadcast_to(spin, (T + 1,) + spin.shape).copy()
    tri, w = flow.vertex_starts(t, v.shape[0])
    out = flow.flow_map_host(mu, E, t, hat, flow.triangle_neighbours(t), tri, w, floor=0.0)
    assert np.max(np.abs(out["weights"].sum(axis=1) - 1.0)) < 1e-12
    assert np.all(out["weights"] >= 0.0) and np.all(out["status"] == 0)
    assert int(out["crossings"].max()) >= 2      # (the particles do move across the mesh)


@pytest.mark.parametrize("max_crossings", [1, 5, 16])
def test_two_triangles_that_push_at_each_other_rest(max_crossings):
    v, t = fc.strip()
    T = 3
    _, hat = hat_gradients(v, t)
    mu = np.ones((T, 4))
    E = np.empty((T + 1, 2, 3))
    E[:, 0], E[:, 1] = (1.0, 1.0, 0.0), (-1.0, -1.0, 0.0)      # both towards the shared edge x + y = 1
    start = (np.array([0], dtype=np.int32), np.array([[0.0, 0.5, 0.5]]))      # on that edge
    out = flow.flow_map_host(mu, E, t, hat, flow.triangle_neighbours(t), *start, floor=0.0, max_crossings=max_crossings)
    assert out["rested"][0] == T and out["crossings"][0] == max_crossings * T and out["status"][0] == 0
    assert np.array_equal(flow.positions(v, t, out["triangle"], out["weights"])[0], [0.5, 0.5, 0.0])      # still on the edge, in either triangle


def test_trajectory_layers_are_the_ends_of_shorter_runs():
    """Layer l is the end of a run over the first l intervals (the later ones floored: no velocity, on the same time step), bit for
    bit; layer 0 is the start; the last layer is the result."""
    name = "plane4"
    v, t = fc.mesh_of(name)
    _, hat = hat_gradients(v, t)
    nbr = flow.triangle_neighbours(t)
    mu, E = fc.random_state(name)
    tri, w = fc.particles(name, 80)
    full = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR, trajectory=True)
    T = mu.shape[0]
    assert full["triangles_at"].shape == (T + 1, 80) and full["weights_at"].shape == (T + 1, 80, 3)
    assert np.array_equal(full["triangles_at"][0], tri) and np.array_equal(full["weights_at"][0], w)
    assert np.array_equal(full["triangles_at"][T], full["triangle"]) and np.array_equal(full["weights_at"][T], full["weights"])
    plain = flow.flow_map_host(mu, E, t, hat, nbr, tri, w, fc.FLOOR)
    assert set(plain) == {"triangle", "weights", "status", "rested", "crossings"}
    for key in plain:
        assert np.array_equal(plain[key], full[key]), key
    for l in range(1, T):
        cut = mu.copy()
        cut[l:] = 0.0
        part = flow.flow_map_host(cut, E, t, hat, nbr, tri, w, fc.FLOOR)
        assert np.array_equal(part["triangle"], full["triangles_at"][l]) and np.array_equal(part["weights"], full["weights_at"][l]), l


@pytest.mark.parametrize("name", list(fc.CASES))
def test_device_cases_exercise_every_rule(name):
    """The inputs of test_hip_flow.py hold a stop at the boundary, a rest, two crossings in one interval and a floored triangle -- here
    with the hat gradients of the numpy reference (the device test asserts the same with the ones the device holds)."""
    v, t = fc.mesh_of(name)
    _, hat = hat_gradients(v, t)
    mu, E = fc.random_state(name)
    tri, w = fc.particles(name)
    nbr = flow.triangle_neighbours(t)
    host = fc.host_reference(mu, E, t, hat, nbr, tri, w, fc.FLOOR, fc.CASES[name][4])
    direct = flow.flow_map_host(mu, E, t, hat, nbr, tri[:40], w[:40], fc.FLOOR, max_crossings=fc.CASES[name][4], trajectory=True)
    for key in direct:      # (tracing every distinct start once lays out what tracing every particle gives)
        assert np.array_equal(direct[key], host[key][:, :40] if key in ("triangles_at", "weights_at") else host[key][:40]), key
    assert all(fc.exercised(name, mu, t, host).values()), fc.exercised(name, mu, t, host)


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the HIP library fails the test: the refusals must come first."""
    from dots_socp_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", refuse)


def test_plug_in_refuses_time_slabs_before_the_library(no_library):
    from dots_socp_amd import socp
    from dots_socp_amd.socp.solver_socp import check_flow_map

    geom, _ = meshes.example("sphere", level=1)
    for plug_in in (socp.solver, socp.solver_raw, socp.solver_cascade):
        with pytest.raises(ValueError, match="time slabs"):
            plug_in(15, geom, flow_map={"starts": "vertices"}, time_slab=(0, 2))
    with pytest.raises(ValueError, match="time slabs"):
        socp.solver_mesh_cascade(15, [geom, geom], flow_map={"starts": "vertices"}, time_slab=(0, 2))
    with pytest.raises(ValueError, match="unknown option"):
        socp.solver(15, geom, flow_map={"start": "vertices"})
    with pytest.raises(ValueError, match="dict"):
        socp.solver_socp(15, geom, flow_map="vertices")
    assert check_flow_map(None, time_slab=(0, 2)) is None      # the default changes nothing

"""What the tests of the trace between two time nodes (dots_flow_trace) share, on top of flow_checks.py (TEST INFRASTRUCTURE, plain
numpy): the intervals of a span, the host reference with span and action, what a traced span exercises, and the figures of the
plane example that test_flow_span_cpu.py asserts on the fp64 oracle and test_hip_flow_span.py bounds the device with."""
import numpy as np

import flow_checks as fc
from dots_socp_amd import flow

# The plane example (meshes.example("plane", n=20), T = 15, tol 1e-4) solved by the fp64 oracle and traced with flow_map_host:
PLANE_BACKWARD_MAX, PLANE_BACKWARD_MEAN = 0.0307, 0.0114      # error against the translation by (-0.2, -0.2, 0), 65 dense vertices of mu1
PLANE_ACTION_RATIO_FORWARD, PLANE_ACTION_RATIO_BACKWARD = 0.9419, 0.9420      # sum(mass * action) / (2 * cost)
PLANE_DENSE_MU0, PLANE_DENSE_MU1 = 69, 65      # vertices with a tenth of the largest density or more

# what a backward trace over (T, 0) exercises on the states and seeds of flow_checks.CASES (strip stops, but never rests)
BACKWARD_RULES = {
    "tetrahedron": {"rested": True, "two_crossings": True, "floored": True},
    "icosphere1": {"rested": True, "two_crossings": True, "floored": True},
    "torus": {"rested": True, "two_crossings": True, "floored": True},
    "plane4": {"rested": True, "two_crossings": True, "floored": True, "stopped": True},
}


def intervals(span):
    """the intervals a span traverses, in order"""
    a, b = span
    return list(range(a, b)) if b > a else list(range(a - 1, b - 1, -1))


def host_reference(mu, E, triangles, hat, nbr, tri, w, floor, max_crossings, span, action=True):
    """``flow_checks.host_reference`` at a span and with the action: every distinct start is traced once."""
    key = np.concatenate([np.asarray(tri, dtype=np.float64)[:, None], w], axis=1)
    uniq, inverse = np.unique(key, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    host = flow.flow_map_host(mu, E, triangles, hat, nbr, uniq[:, 0].astype(np.int32), np.ascontiguousarray(uniq[:, 1:]), floor,
                              max_crossings=max_crossings, trajectory=True, span=span, action=action)
    return {k: np.ascontiguousarray(a[:, inverse] if k in ("triangles_at", "weights_at") else a[inverse]) for k, a in host.items()}


def exercised(name, mu, triangles, host, span):
    """``flow_checks.exercised`` for a result traced over ``span``: layer i took the interval ``intervals(span)[i]``."""
    max_crossings = fc.CASES[name][4]
    js = intervals(span)
    n = len(js)
    rho = fc.density_on_triangles(mu, triangles)
    moving = host["status"] == 0
    floored = any(bool(np.any(moving & (rho[js[i], host["triangles_at"][i]] <= fc.FLOOR))) for i in range(n))
    free = bool(np.any(host["crossings"] - max_crossings * host["rested"] > n - host["rested"]))
    nbr = flow.triangle_neighbours(triangles)
    for i in range(n):
        f, g = host["triangles_at"][i], host["triangles_at"][i + 1]
        free = free or bool(np.any((g != f) & np.all(nbr[f] != g[:, None], axis=1)))
    out = {"rested": bool(np.any(host["rested"] > 0)), "two_crossings": free, "floored": floored}
    if fc.CASES[name][2]:
        out["stopped"] = bool(np.any(host["status"] == 1))
    return out


def dense(mass, area_vertices):
    """the vertices that carry a tenth of the largest density of ``mass`` or more"""
    density = np.asarray(mass) / (np.asarray(area_vertices) / 3.0)
    return density > 0.1 * density.max()


def plane_figures(trace, geom, scale, cost):
    """The figures of the plane example from ``trace(starts, span, action) -> result`` (``starts``: ``(triangle, weights)``; the result
    holds status, rested, triangle, weights and the action): the backward error over the dense vertices of mu1, the round trip of the
    dense vertices of mu0, and both action ratios."""
    v, t = np.asarray(geom["vertices"]), np.asarray(geom["triangles"])
    T = 15
    tri, w = flow.vertex_starts(t, v.shape[0])
    d0, d1 = dense(geom["mu0"], geom["area_vertices"]), dense(geom["mu1"], geom["area_vertices"])
    forward, backward = trace((tri, w), (0, T), True), trace((tri, w), (T, 0), True)
    at = flow.positions(v, t, backward["triangle"], backward["weights"])
    error = np.linalg.norm((at - v) / scale - np.array([-0.2, -0.2, 0.0]), axis=1)[d1]
    out = {"dense_mu0": int(d0.sum()), "dense_mu1": int(d1.sum()),
           "backward_clean": bool(np.all(backward["status"][d1] == 0) and np.all(backward["rested"][d1] == 0)),
           "backward_max": float(error.max()), "backward_mean": float(error.mean()),
           "ratio_forward": float(np.sum(geom["mu0"] * forward["action"]) / (2.0 * cost)),
           "ratio_backward": float(np.sum(geom["mu1"] * backward["action"]) / (2.0 * cost))}
    ends = (np.ascontiguousarray(forward["triangle"][d0]), np.ascontiguousarray(forward["weights"][d0]))
    back = trace(ends, (T, 0), False)
    home = flow.positions(v, t, back["triangle"], back["weights"])
    out["round_trip_clean"] = bool(np.all(forward["status"][d0] == 0) and np.all(forward["rested"][d0] == 0)
                                   and np.all(back["status"] == 0) and np.all(back["rested"] == 0))
    out["round_trip"] = float(np.max(np.linalg.norm(home - v[d0], axis=1)))
    return out

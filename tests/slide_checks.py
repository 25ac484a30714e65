"""What the tests of the sliding mode of the flow map (dots_flow_slide) share, on top of flow_checks.py and span_checks.py (TEST
INFRASTRUCTURE, plain numpy): the case list of the CPU and the GPU tests, the host reference with ``slide=True``, the triangle areas
the device holds in the caller's numbering, the two-triangle problem with a known answer, and the figures of the plane example."""
import math

import numpy as np

import flow_checks as fc
from dots_socp_amd import flow
from dots_socp_amd.geometry import hat_gradients

SHORT = [name for name in fc.CASES if fc.CASES[name][1] <= 7]      # the five cases of a few intervals
DEVICE_CASES = SHORT + ["icosphere0_257"]                          # and a pitch of 512 with a cap of 3
MOVED = ("strip", "icosphere1", "torus", "plane4")                 # at least half of 200 particles end elsewhere than without slide
# (name, span): the whole horizon forward, the whole horizon backward and one interior span where the horizon has one
SPANS = [(name, span) for name in DEVICE_CASES for span in
         {1: [(0, 1), (1, 0)], 2: [(0, 2), (2, 0), (1, 2)], 3: [(0, 3), (3, 0), (2, 1)], 5: [(0, 5), (5, 0), (1, 4)], 7: [(0, 7), (7, 0), (6, 1)],
          257: [(0, 257), (257, 0), (200, 130)]}[fc.CASES[name][1]]]

# (the strip never rests backward or over its second interval alone -- span_checks.BACKWARD_RULES --: nothing slides there, the spans run all the same)
NO_SLIDES = {("strip", (2, 0)), ("strip", (1, 2))}

# the plane example (meshes.example("plane", n=20), T = 15, vertex starts, the default floor) on the fp64 oracle
PLANE_RESTED_MASS_30 = (9.82e-2, 4.46e-3)      # after nit = 30: the mass of the particles that rest, without and with slide
PLANE_FORWARD_MAX, PLANE_FORWARD_MEAN = 0.0312, 0.0120      # converged: error against the translation by (0.2, 0.2, 0), 69 dense vertices of mu0


def case(name, count=200):
    """``(v, t, areas, hat, nbr, mu, E, tri, w)`` of a case of flow_checks on the host's own hat gradients and areas"""
    v, t = fc.mesh_of(name)
    areas, hat = hat_gradients(v, t)
    mu, E = fc.random_state(name)
    tri, w = fc.particles(name, count)
    return v, t, areas, hat, flow.triangle_neighbours(t), mu, E, tri, w


def caller_areas(plan):
    """the triangle areas the device holds (DevicePlan.area_tri, device numbering) in the caller's triangle numbering"""
    area = np.asarray(plan.area_tri, dtype=np.float64)
    if plan.perm_tri is None:
        return area
    out = np.empty_like(area)
    out[plan.perm_tri] = area
    return out


def host_reference(mu, E, triangles, hat, areas, nbr, tri, w, floor, max_crossings, span, action=True, tally=None):
    """``span_checks.host_reference`` with ``slide=True``: every distinct start is traced once (``tally`` then counts distinct starts)."""
    key = np.concatenate([np.asarray(tri, dtype=np.float64)[:, None], w], axis=1)
    uniq, inverse = np.unique(key, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    host = flow.flow_map_host(mu, E, triangles, hat, nbr, uniq[:, 0].astype(np.int32), np.ascontiguousarray(uniq[:, 1:]), floor,
                              max_crossings=max_crossings, trajectory=True, span=span, action=action, slide=True, areas=areas, tally=tally)
    return {k: np.ascontiguousarray(a[:, inverse] if k in ("triangles_at", "weights_at") else a[inverse]) for k, a in host.items()}


def weight_sums(weights):
    w = np.asarray(weights)
    return (w[..., 0] + w[..., 1]) + w[..., 2]


def moved(a, b):
    """the particles of two results that end at different places"""
    return (a["triangle"] != b["triangle"]) | np.any(a["weights"] != b["weights"], axis=1)


# ---- two triangles that push a particle at each other: the known answer ----------------------------------------------------------
# flow_checks.strip: triangle 0 = (0, 1, 2), triangle 1 = (1, 3, 2), the shared edge from vertex 1 = (1, 0) to vertex 2 = (0, 1)
STRIP_NORMAL = np.array([1.0, 1.0, 0.0]) / math.sqrt(2.0)       # from triangle 0 into triangle 1
STRIP_TANGENT = np.array([-1.0, 1.0, 0.0]) / math.sqrt(2.0)     # from vertex 1 towards vertex 2


def strip_problem(a, b, p, r, start=(0.2, 0.4, 0.4)):
    """One interval of length 1 with mu = 1 (above the floor 0.5): triangle 0 moves the particle towards the edge at normal speed ``a``
    with tangential speed ``p``, triangle 1 moves it back at normal speed ``b`` with tangential speed ``r``.  Returns the arguments of
    ``flow_map_host`` up to the floor, the areas, and the exact answer for a slide that stays on the edge: ``(args, areas, entry point,
    time left at the entry, end point, action)``."""
    v, t = fc.strip()
    areas, hat = hat_gradients(v, t)
    u0, u1 = a * STRIP_NORMAL + p * STRIP_TANGENT, -b * STRIP_NORMAL + r * STRIP_TANGENT
    E = np.empty((2, 2, 3))
    E[:, 0], E[:, 1] = u0, u1
    mu = np.ones((1, 4))
    w = np.array([start], dtype=np.float64)
    x = flow.positions(v, t, np.array([0]), w)[0]
    t_hit = float((1.0 - (x[0] + x[1])) / math.sqrt(2.0) / a)      # the edge is the line x + y = 1
    entry = x + t_hit * u0
    speed = (b * p + a * r) / (a + b)
    end = entry + speed * (1.0 - t_hit) * STRIP_TANGENT
    act = t_hit * float(u0 @ u0) + (1.0 - t_hit) * speed * speed
    args = (mu, E, t, hat, flow.triangle_neighbours(t), np.array([0], dtype=np.int32), w, 0.5)
    return args, areas, entry, 1.0 - t_hit, end, act


def plane_rested_mass(result, mu0):
    """the mass of mu0 on the vertex starts that rested at least once"""
    return float(np.sum(np.asarray(mu0)[np.asarray(result["rested"]) > 0]))

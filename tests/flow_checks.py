"""The cases of the flow map (dots_flow_map), shared by test_flow_cpu.py and test_hip_flow.py (TEST INFRASTRUCTURE, plain numpy on top of
dots_socp_amd.flow): small meshes, a random state with floored vertices, particle starts, and what a case must exercise so that a
kernel that does nothing cannot pass."""
import functools

import numpy as np

from dots_socp_amd import flow, meshes

FLOOR = 0.3
COUNTS = (1, 63, 64, 65, 257, 1000)      # one lane, around a wavefront, more than one workgroup, a ragged last workgroup


def tetrahedron():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)


def strip():
    """two triangles that share the edge (1, 2)"""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]])
    return v, np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int64)


LONG_POOL = 64      # distinct interior starts at 257 and 600 intervals, repeated like the vertex starts (see host_reference)

# name: (mesh, n_time, open surface, seed, max_crossings, distinct interior starts or None = all).  The seeds were picked on the host
# so that every case holds all of `exercised`.  The long horizons (pitches 512 and 1024) rest after 3 crossings: a rest then costs
# the host reference 4 steps instead of 17, and the cap is exercised at a second value.
CASES = {
    "tetrahedron": (tetrahedron, 1, False, 15, 16, None),
    "strip": (strip, 2, True, 29, 16, None),
    "icosphere1": (lambda: meshes.icosphere(1), 3, False, 0, 16, None),
    "torus": (lambda: meshes.torus(12, 8), 5, False, 0, 16, None),      # built with the default reordering: the device numbering differs
    "plane4": (lambda: meshes.plane(4), 7, True, 0, 16, None),
    "icosphere0_257": (lambda: meshes.icosphere(0), 257, False, 0, 3, LONG_POOL),      # pitch 512
    "icosphere0_600": (lambda: meshes.icosphere(0), 600, False, 0, 3, LONG_POOL),      # pitch 1024
}


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    v, t = CASES[name][0]()
    return np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(t, dtype=np.int64)


def geometry_of(name):
    """the geometry a DeviceProblem is built from: equal masses (the state is uploaded, nothing is solved)"""
    v, t = mesh_of(name)
    geom, _ = meshes.make_geometry(v, t, np.full(v.shape[0], 1.0 / v.shape[0]), np.full(v.shape[0], 1.0 / v.shape[0]), normalize=False)
    return geom


def random_state(name):
    """``(mu (T, V), E (T + 1, F, 3))``: mu in (0, 1] with a fifth of the entries far below FLOOR (a triangle with two of them is
    floored), E uniform and sized so that a particle moves up to about one edge per interval."""
    v, t = mesh_of(name)
    T, seed = CASES[name][1], CASES[name][3]
    rng = np.random.default_rng(1000 + seed)
    mu = 0.5 + 0.5 * (1.0 - rng.random((T, v.shape[0])))
    low = rng.random(mu.shape) < 0.2
    mu[low] = 0.05 * (1.0 - rng.random(int(low.sum())))
    edge = float(np.mean(np.linalg.norm(v[t[:, 1]] - v[t[:, 0]], axis=1)))
    E = rng.uniform(-1.0, 1.0, (T + 1, t.shape[0], 3)) * (edge * T * 0.75)
    return mu, E


def particles(name, count=max(COUNTS)):
    """``(triangle (count,) int32, weights (count, 3))``: the vertex starts repeated (even particles) and random interior points (odd
    ones; at the long horizons a pool of LONG_POOL of them, repeated), so that every prefix holds both kinds."""
    v, t = mesh_of(name)
    rng = np.random.default_rng(2000 + CASES[name][3])
    vt, vw = flow.vertex_starts(t, v.shape[0])
    pool = CASES[name][5] or count
    x = 0.05 + rng.random((pool, 3))
    it, iw = rng.integers(0, t.shape[0], pool).astype(np.int32), x / x.sum(axis=1, keepdims=True)
    tri = np.empty(count, dtype=np.int32)
    w = np.empty((count, 3))
    for i in range(count):
        src = (vt, vw, (i // 2) % v.shape[0]) if i % 2 == 0 else (it, iw, (i // 2) % pool)
        tri[i], w[i] = src[0][src[2]], src[1][src[2]]
    return tri, w


def host_reference(mu, E, triangles, hat, nbr, tri, w, floor, max_crossings):
    """``flow_map_host`` with the trajectory for all the particles: they are independent, so every distinct start is traced once and
    the result is laid out for all of them (the vertex starts repeat; so does the interior pool of the long horizons, where the
    scalar reference of a thousand distinct particles would take ten seconds)."""
    key = np.concatenate([np.asarray(tri, dtype=np.float64)[:, None], w], axis=1)
    uniq, inverse = np.unique(key, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    host = flow.flow_map_host(mu, E, triangles, hat, nbr, uniq[:, 0].astype(np.int32), np.ascontiguousarray(uniq[:, 1:]), floor,
                              max_crossings=max_crossings, trajectory=True)
    return {k: np.ascontiguousarray(a[:, inverse] if k in ("triangles_at", "weights_at") else a[inverse]) for k, a in host.items()}


def density_on_triangles(mu, triangles):
    """rho of every (interval, triangle), with the operations of the specification"""
    t = np.asarray(triangles)
    return ((mu[:, t[:, 0]] + mu[:, t[:, 1]]) + mu[:, t[:, 2]]) * (1.0 / 3.0)


def exercised(name, mu, triangles, host):
    """What a host result (with its trajectory) shows the inputs to exercise: a stop at the boundary (open meshes), a rest at the cap,
    at least two crossings in one interval that did not end in a rest (on more than two triangles: two triangles alone can only
    pass a particle back and forth, which ends at the cap), a particle that sat in a floored triangle."""
    T, max_crossings = mu.shape[0], CASES[name][4]
    rho = density_on_triangles(mu, triangles)
    moving = host["status"] == 0      # (never stopped: it took every interval from the triangle the layer names)
    floored = any(bool(np.any(moving & (rho[l, host["triangles_at"][l]] <= FLOOR))) for l in range(T))
    # (the intervals that ended in a rest hold max_crossings crossings each: more crossings than intervals among the others; or an
    # interval that ends in a triangle which is neither the one it began in nor a neighbour of it)
    free = bool(np.any(host["crossings"] - max_crossings * host["rested"] > T - host["rested"]))
    nbr = flow.triangle_neighbours(triangles)
    for l in range(T):
        f, g = host["triangles_at"][l], host["triangles_at"][l + 1]
        free = free or bool(np.any((g != f) & np.all(nbr[f] != g[:, None], axis=1)))
    out = {"rested": bool(np.any(host["rested"] > 0)),
           "two_crossings": free if np.asarray(triangles).shape[0] > 2 else bool(np.any(host["rested"] > 0)) and max_crossings >= 2,
           "floored": floored}
    if CASES[name][2]:
        out["stopped"] = bool(np.any(host["status"] == 1))
    return out


def caller_hat(plan):
    """the hat gradients the device holds (DevicePlan.hat_grad, device numbering) in the caller's triangle numbering"""
    hat = np.asarray(plan.hat_grad, dtype=np.float64).reshape(-1, 3, 3)
    if plan.perm_tri is None:
        return hat
    out = np.empty_like(hat)
    out[plan.perm_tri] = hat
    return out

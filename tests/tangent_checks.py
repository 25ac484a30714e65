"""The cases of linearised transport (dots_socp_amd.tangent, dots_tangent_*, socp.tangent_embedding), shared by test_tangent_cpu.py
and test_hip_tangent.py (TEST INFRASTRUCTURE): the plane experiment with the bounds of its fp64-oracle run, the meshes and random
inputs of the kernel tests, and the bound two correct Gram sums keep."""
import math

import numpy as np

import flow_checks as fc
from dots_socp_amd import meshes, tangent

U = 2.0 ** -53

# ---- the plane: Gaussians whose transport is a translation ----------------------------------------------------------------------------
PLANE_N, PLANE_T, PLANE_SCALE = 10, 7, 2 * 0.1 ** 2
PLANE_TOL_ORACLE, PLANE_TOL_DEVICE = 1e-5, 1e-4
PLANE_REFERENCE = (0.5, 0.5)
PLANE_CENTRES = ((0.4, 0.4), (0.6, 0.6), (0.6, 0.4), (0.5, 0.65))
PLANE_PAIRS = ((0, 1), (2, 3))
# the bounds of the oracle's run.  Measured (test_tangent_cpu.py prints the figures again): |G_ii / (2 cost_i) - 1| up to 2.6e-3 (the
# prototype: 1.9e-3), an O(h) discretisation gap and not noise: five times the prototype's, 1e-2; the pair distances against twice the
# direct pair cost 3.3e-4 and 1.4e-4 relative (the prototype: 7.1e-5 and 2.8e-4): ten times the worse one, 3e-3; the sigma-weighted mean
# velocity against the displacement 5.2e-4 (the prototype: 4e-4): 5e-3
BOUND_SELF, BOUND_PAIR, BOUND_MEAN = 1e-2, 3e-3, 5e-3
DEVICE_MARGIN = 1.5      # the project's margin of a device run over bounds that rest on the oracle


def plane_case():
    """``(geometry without masses, reference (V,), measures [4 x (V,)], displacements (4, 3))`` of the plane in the unit box"""
    v, t = meshes.plane(PLANE_N)
    geom, _ = meshes.make_geometry(v, t, normalize=False)
    density = lambda c: meshes.gaussian_density(geom["vertices"], geom["area_vertices"], [c[0], c[1], 0.0], PLANE_SCALE)
    moves = np.array([[c[0] - PLANE_REFERENCE[0], c[1] - PLANE_REFERENCE[1], 0.0] for c in PLANE_CENTRES])
    return geom, density(PLANE_REFERENCE), [density(c) for c in PLANE_CENTRES], moves


def oracle_solve(geom, n_time=PLANE_T, tol=PLANE_TOL_ORACLE):
    """``solve(sigma, mu)`` of tangent_embedding_host on the fp64 oracle"""
    from conftest import load_oracle

    oracle = load_oracle()

    def solve(sigma, mu):
        sol, hist = oracle.solver_socp(n_time, {**geom, "mu0": sigma, "mu1": mu}, tol=tol)
        return hist.history["Transportation cost"][-1], sol["phi"][0]
    return solve


def mean_velocity(velocity, w):
    """the sigma-weighted mean of one field (F, 3)"""
    return np.array([math.fsum(w * velocity[:, d]) for d in range(3)]) / math.fsum(w)


def plane_figures(gram, costs, velocities, w, moves, pair_costs):
    """The three figures the plane experiment is judged by: max |G_ii / (2 cost_i) - 1|, per pair |D_ij - 2 cost_ij| / (2 cost_ij), max
    |mean velocity - displacement|"""
    D = tangent.squared_distances(gram)
    own = max(abs(gram[i, i] / (2.0 * costs[i]) - 1.0) for i in range(len(costs)))
    pairs = [abs(D[i, j] - 2.0 * c) / (2.0 * c) for (i, j), c in pair_costs.items()]
    mean = max(float(np.max(np.abs(mean_velocity(velocities[i], w) - moves[i]))) for i in range(len(costs)))
    return own, pairs, mean


# ---- the kernels against the specification ------------------------------------------------------------------------------------------------
# F = 4 (less than a wave); 32; 80; 192; 2 080 = two chunks of the Gram kernel, whose lanes take the triangles lane + 256 c + 512 j: the
# last round (2 048 ..) has 32 lanes of one workgroup at work, half a wave; 5 120 = three chunks
KERNEL_MESHES = {"tetrahedron": 4, "plane4": 32, "icosphere1": 80, "torus": 192, "torus40x26": 2080, "icosphere4": 5120}
KERNEL_N = (1, 2, 3, 5, 16, 17)      # 16 | 17: the potentials of one velocity launch; 4 | 5, 16 | 17: the Gram's 4 x 4 tile and its edge


def kernel_mesh(name):
    if name in fc.CASES:
        return fc.mesh_of(name)
    v, t = meshes.torus(40, 26) if name == "torus40x26" else meshes.icosphere(4)
    return np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(t, dtype=np.int64)


def kernel_geometry(name):
    """the geometry a DeviceProblem is built from: equal masses (nothing is solved)"""
    v, t = kernel_mesh(name)
    assert t.shape[0] == KERNEL_MESHES[name]
    geom, _ = meshes.make_geometry(v, t, np.full(v.shape[0], 1.0 / v.shape[0]), np.full(v.shape[0], 1.0 / v.shape[0]), normalize=False)
    return geom


def kernel_inputs(name, n):
    """``(potentials (n, V), sigma (V,))``: standard normal potentials, each with its own constant of size 3 (no gauge is fixed); a
    reference measure over three decades with a fifth of its entries zero."""
    V = kernel_mesh(name)[0].shape[0]
    rng = np.random.default_rng(5000 + 31 * V + n)
    potentials = rng.standard_normal((n, V)) + rng.uniform(-3.0, 3.0, (n, 1))
    sigma = 10.0 ** rng.uniform(-3.0, 0.0, V)
    sigma[rng.random(V) < 0.2] = 0.0
    if not np.any(sigma > 0.0):
        sigma[0] = 1.0
    return potentials, sigma


def gram_bound(host, A, B, w):
    """What a Gram sum carried as an unevaluated pair keeps against ``gram_host``: ``ulp(host) + 2^-100 F sum_f |term_f|`` per entry --
    the terms are the same bits on both sides and every two_sum is exact; only the low parts are rounded, each a 2^-53 fraction of a
    partial sum's."""
    B = A if B is None else B
    F = A.shape[1]
    size = np.array([[math.fsum(np.abs(tangent.gram_terms(A[i], B[j], w))) for j in range(B.shape[0])] for i in range(A.shape[0])])
    return np.spacing(np.abs(host)) + 2.0 ** -100 * F * size


def renumbering(n_vertices, n_triangles, seed=0):
    """``(pv, pf)``: new vertex i is old vertex pv[i], new triangle i is old triangle pf[i]"""
    rng = np.random.default_rng(7000 + seed)
    return rng.permutation(n_vertices), rng.permutation(n_triangles)


def renumbered(vertices, triangles, pv, pf):
    inv = np.empty_like(pv)
    inv[pv] = np.arange(pv.shape[0])
    return np.ascontiguousarray(vertices[pv]), np.ascontiguousarray(inv[triangles[pf]])

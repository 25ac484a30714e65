"""The cases of the cost gradients (dots_sensitivity), shared by test_sensitivity_cpu.py and test_hip_sensitivity.py (TEST
INFRASTRUCTURE, plain numpy on top of dots_socp_amd.sensitivity): random states on the meshes of flow_checks.py, the kinetic energy
written directly as a sum over t, v and f, and the finite differences of the transport cost on the plane example."""
import numpy as np

import flow_checks as fc
from dots_socp_amd import meshes
from dots_socp_amd.geometry import hat_gradients

MESHES = ("tetrahedron", "strip", "icosphere1", "torus", "plane4")
HORIZONS = (1, 2, 31, 32, 127, 300)      # one interval, both sides of a pitch boundary (32 nodes | 33), a long-horizon pitch (512)
FACTOR_PHI, FACTOR_MU = 0.8125, 1.7      # recovery factors other than 1 (one exact in binary, one not)

# the oracle experiment of DESIGN.md section 9, "Cost gradients"
PLANE_N, PLANE_T, PLANE_TOL, PLANE_NIT = 8, 7, 1e-7, 100000
EPS_DENSITY, EPS_SHAPE = 1e-3, 5e-4
BOUND_COST, BOUND_DENSITY, BOUND_SHAPE = 1e-6, 2e-4, 1.2e-3


def random_state(name, n_time, seed=0):
    """``(mu (T, V), phi (T + 1, V))``: mu in (0, 1], phi standard normal -- every product and sum of the stress is exercised."""
    v, _ = fc.mesh_of(name)
    rng = np.random.default_rng(3000 + 17 * seed + n_time)
    return 1.0 - rng.random((n_time, v.shape[0])), rng.standard_normal((n_time + 1, v.shape[0]))


def vertex_masses(vertices, triangles):
    area = meshes.triangle_areas(vertices, triangles)
    return meshes.vertex_areas(np.asarray(vertices).shape[0], triangles, area) / 3.0


def kinetic_energy_direct(mu, phi, vertices, triangles):
    """K = h sum_t sum_f sum_k mu[t][v_k] (area_f / 3) 0.5 (|grad phi_t|_f^2 / 2 + |grad phi_t+1|_f^2 / 2), written as it reads: the
    density at the corner, a third of the triangle's area, the mean over the interval's two nodes of half the squared gradient --
    no stress tensor, no vertex masses."""
    t = np.asarray(triangles)
    area, hat = hat_gradients(vertices, t)
    grad = np.einsum("fkc,tfk->tfc", hat, phi[:, t])                  # (T + 1, F, 3)
    half_sq = 0.5 * np.einsum("tfc,tfc->tf", grad, grad)
    per_interval = 0.5 * (half_sq[:-1] + half_sq[1:])                 # (T, F)
    return float(np.einsum("tfk,f,tf->", mu[:, t], area / 3.0, per_interval)) / mu.shape[0]


def plane_geometry(bent=False):
    """The plane example (unit box); ``bent``: the sheet with z += 0.05 sin(5 x) cos(4 y), the same masses."""
    geom, _ = meshes.example("plane", n=PLANE_N)
    if not bent:
        return geom
    x = geom["vertices"].copy()
    x[:, 2] += 0.05 * np.sin(5.0 * x[:, 0]) * np.cos(4.0 * x[:, 1])
    return meshes.make_geometry(x, geom["triangles"], geom["mu0"], geom["mu1"], normalize=False)[0]


def density_direction(mu, seed=0):
    """mean-free, supported where mu > 0.2 max, L1 norm 1"""
    support = mu > 0.2 * mu.max()
    d = np.zeros_like(mu)
    d[support] = np.random.default_rng(seed).standard_normal(int(support.sum()))
    d[support] -= d[support].mean()
    return d / np.abs(d).sum()


def shape_direction(n_vertices):
    d = np.random.default_rng(1).standard_normal((n_vertices, 3)) * 0.3
    return d / np.abs(d).max()


def with_change(geom, mu0=None, mu1=None, vertices=None):
    """the geometry with other masses or vertex positions, rebuilt as given (areas follow the vertices; the MASSES stay)"""
    return meshes.make_geometry(geom["vertices"] if vertices is None else vertices, geom["triangles"], geom["mu0"] if mu0 is None else mu0,
                                geom["mu1"] if mu1 is None else mu1, normalize=False)[0]


def central_difference(cost, geom, eps, **direction):
    """(cost(+eps d) - cost(-eps d)) / (2 eps) of ``cost(geometry)`` along one of mu0 / mu1 / vertices"""
    (key, d), = direction.items()
    plus, minus = (cost(with_change(geom, **{key: geom[key] + s * eps * d})) for s in (1.0, -1.0))
    return (plus - minus) / (2.0 * eps)


def densities_held_fixed(mu, phi, vertices, triangles, d, eps=1e-6):
    """The WRONG shape derivative along ``d``: minus the derivative of the kinetic energy with the densities ``mu`` held fixed, so that
    the masses move with the vertex areas (``kinetic_energy_direct`` is explicit in the vertices: a central difference of it)."""
    plus, minus = (kinetic_energy_direct(mu, phi, vertices + s * eps * d, triangles) for s in (1.0, -1.0))
    return -(plus - minus) / (2.0 * eps)


def relative(a, b):
    return abs(a - b) / abs(b)

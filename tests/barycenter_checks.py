"""The cases of the barycentre (dots_socp_amd.barycenter, dots_barycenter_update, socp.barycenter), shared by test_barycenter_cpu.py
and test_hip_barycenter.py (TEST INFRASTRUCTURE): the plane case with its exact answer and the figures of the fp64 oracle the device
test's bounds rest on, the meshes and random inputs of the update test with the bound two correct implementations keep, and the
bump measures of the small surfaces."""
import math

import numpy as np

from dots_socp_amd import barycenter, evaluate, meshes

# ---- the plane: two Gaussians whose barycentres are known exactly ---------------------------------------------------------------------
PLANE_N, PLANE_T, PLANE_TOL, PLANE_ETA, PLANE_STEPS = 10, 7, 1e-4, 100.0, 8
# barycenter_host on oracle/dots_oracle.py (solver_socp(7, ., tol=1e-4)) from the default start with eta = 100, as printed by
#     python -c "import sys; sys.path[:0] = ['tests', '.']; import barycenter_checks as b; b.print_oracle_figures()"
# relative L1 distance (rel_l1 below) to plane_exact_transportation([t]):
ORACLE_HALF_L1 = 0.04414          # weights (0.5, 0.5), 8 steps, t = 0.5   (objective 0.0259017, 0.0103962, ..., 0.0102999; eta halved at step 5)
ORACLE_HALF_OBJECTIVE = 0.010300  # the last objective of that run (0.0102999382); the issue's prototype, from another start: 0.010304
ORACLE_QUARTER_L1 = 0.03344       # weights (0.25, 0.75), 8 steps, t = 0.75  (last objective 0.0077282)
ORACLE_ONE_L1 = 0.01368           # K = 1, the measure mu1 alone, 10 steps: distance to mu1 itself
ORACLE_MARGIN = 1.5               # the project's margin on bounds that rest on the oracle


def rel_l1(a, b):
    """sum |a - b| / sum |b|"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return math.fsum(np.abs(a - b)) / math.fsum(np.abs(b))


def plane_case():
    """``(geometry, [mu0, mu1])`` of the plane example in the unit box"""
    geom, _ = meshes.example("plane", n=PLANE_N, normalize=False)
    return geom, [np.asarray(geom["mu0"], dtype=np.float64), np.asarray(geom["mu1"], dtype=np.float64)]


def plane_exact(geom, t):
    return evaluate.plane_exact_transportation([t], geom["vertices"], geom["area_vertices"])[0]


def oracle_solve(geom, n_time=PLANE_T, tol=PLANE_TOL):
    """``solve(nu, mu)`` of barycenter_host on the fp64 oracle"""
    from conftest import load_oracle

    oracle = load_oracle()

    def solve(nu, mu):
        sol, hist = oracle.solver_socp(n_time, {**geom, "mu0": nu, "mu1": mu}, tol=tol)
        return hist.history["Transportation cost"][-1], sol["phi"][0]
    return solve


def print_oracle_figures():
    geom, (mu0, mu1) = plane_case()
    solve = oracle_solve(geom)
    for name, ms, w, steps, target in (("half", [mu0, mu1], [0.5, 0.5], PLANE_STEPS, plane_exact(geom, 0.5)),
                                       ("quarter", [mu0, mu1], [0.25, 0.75], PLANE_STEPS, plane_exact(geom, 0.75)),
                                       ("one", [mu1], None, 10, mu1)):
        r = barycenter.barycenter_host(solve, ms, w, geom["area_vertices"], steps, PLANE_ETA)
        print(name, "objective", r["objective"], "eta", r["eta"], "rel_l1", rel_l1(r["nu"], target))


# ---- the update against update_host ----------------------------------------------------------------------------------------------------
# name -> (mesh, reorder).  V = 4; 90; 96 in the "nd" numbering, which is not the identity; 642; 1 040 = more than one workgroup of 256
# per stage (5 of them; 1 040 is no multiple of 256, 64 or 2)
UPDATE_MESHES = {"tetrahedron": 4, "plane8": 90, "torus_nd": 96, "icosphere3": 642, "torus40x26": 1040}
UPDATE_N = (1, 2, 3, 16)
UPDATE_ETA = 100.0


def update_mesh(name):
    if name == "tetrahedron":
        v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
        return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)
    if name == "plane8":
        return meshes.plane(8)
    if name == "torus_nd":
        return meshes.torus(12, 8)
    if name == "icosphere3":
        return meshes.icosphere(3)
    return meshes.torus(40, 26)


def update_geometry(name):
    """the geometry a DeviceProblem is built from: equal masses (nothing is solved)"""
    v, t = update_mesh(name)
    v, t = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(t, dtype=np.int64)
    geom, _ = meshes.make_geometry(v, t, np.full(v.shape[0], 1.0 / v.shape[0]), np.full(v.shape[0], 1.0 / v.shape[0]), normalize=False)
    assert v.shape[0] == UPDATE_MESHES[name]
    return geom


def update_inputs(name, n):
    """``(nu (V,), potentials (n, V), weights (n,), eta, mass)``: potentials of the size the solver's are where eta = 100 is the
    working step (eta * |g| of order 1, so that the update moves a good part of the mass), each with its own large constant (no
    gauge is fixed), weights of both signs of size 1 / n, a positive nu over three decades, a mass that is not 1."""
    V = UPDATE_MESHES[name]
    rng = np.random.default_rng(1000 * V + n)
    potentials = 0.02 * rng.standard_normal((n, V)) + rng.uniform(-3.0, 3.0, (n, 1))
    weights = rng.uniform(0.5, 1.5, n) / n
    if n > 2:
        weights[1] = -weights[1]
    nu = 10.0 ** rng.uniform(-3.0, 0.0, V)
    mass = 1.75
    return nu * (mass / math.fsum(nu)), potentials, weights, UPDATE_ETA, mass


U = 2.0 ** -53


def update_bounds(V, nu_host, scalars_host):
    """What two correct implementations of update_host keep (the issue's bounds): per element 8 * 2^-53 * nu + nu * V * 2^-53 -- two
    exp within 1 ulp of the truth differ by at most 2 ulp, the multiplication and the scaling add 2, and a sum of positive terms in any
    order is within V * 2^-53 relative of the exactly rounded one --, the same V * 2^-53 relative for ``sum`` and ``change``, 4 ulp
    for ``gmax`` and ``min``."""
    return {"nu": 8.0 * U * nu_host + np.abs(nu_host) * (V * U), "sum": V * U * abs(scalars_host["sum"]), "change": V * U * abs(scalars_host["change"]),
            "gmax": 4.0 * np.spacing(scalars_host["gmax"]), "min": 4.0 * np.spacing(scalars_host["min"])}


# ---- bumps on the small closed surfaces --------------------------------------------------------------------------------------------------
def bump_measures(geom, count=3):
    """``count`` bumps of mass 1 at farthest vertices (from vertex 0)"""
    v = np.asarray(geom["vertices"], dtype=np.float64)
    return [meshes.bump_density(v, np.asarray(geom["area_vertices"], dtype=np.float64), [c]) for c in meshes.farthest_vertices(v, 0, count)]


def surface_geometry(name):
    v, t = meshes.torus(12, 8) if name == "torus" else meshes.icosphere(1)
    geom, _ = meshes.make_geometry(v, t, normalize=False)
    return {k: val for k, val in geom.items() if k not in ("mu0", "mu1")}

"""The cases and bounds of the windowed modal PCG (dots_pcg_windows), shared by test_pcg_windows_cpu.py -- which measures the bounds on
the host and asserts that the measurements stay under the recorded values -- and test_hip_pcg_windows.py (TEST INFRASTRUCTURE, plain
numpy / scipy on top of pcg_checks.py).

Above 256 time nodes the device solves the T + 1 modal problems in windows of 256 modes, each through the PCG kernels at pitch 256
with a loop of its own.  The host PCG of pcg_checks.py runs ONE loop over all T + 1 columns; a column's arithmetic does not depend on
the other columns (per-column scalars, converged columns frozen one by one), so it is the reference of every window at once."""
import functools

import numpy as np

import pcg_checks as pc

HORIZONS = (300, 511, 600, 1023)      # two windows (the second partly live), two full, three of four (pitch 1024), four full
WINDOWS = {300: 2, 511: 2, 600: 3, 1023: 4}
MESH = pc.SPHERE2                     # V = 162
COLLAPSE_MESH, COLLAPSE_T = pc.TORUS_4176, 300      # the pitch-256 view has 4176 > 1024 workgroups: k_collapse sums the partial rows
ITERATE_CASES = [(MESH, T) for T in HORIZONS] + [(COLLAPSE_MESH, COLLAPSE_T)]
CONVERGED_TOL = 1e-12
MG_COARSEST = 40                      # small enough for a second level on 162 vertices

# Iterates: 100 x the rounding spread of the host PCG alone on these cases (float64 against np.longdouble and against a seeded
# renumbering of the vertices, cg_max_iter = 8 and 16, eps = 0 and 1e-2), never above pcg_checks.PHI_CEILING.
# Measured by test_pcg_windows_cpu.py::test_rounding_spread_and_bound: 2.3e-14 (sphere, T = 1023, eps = 1e-2).
SPREAD = {"windows": 3e-14}
BOUND = {"windows": min(100.0 * SPREAD["windows"], pc.PHI_CEILING)}

# Converged solves (cg_tol = 1e-12): what the stopping rule itself leaves -- the host Jacobi PCG run to convergence against the
# oracle's per-mode SuperLU (gauge removed at eps = 0), largest over HORIZONS and both eps.  The device bound is 10 x that, never
# above 1e-8.  These cases take the sphere's densities AS THEY ARE (equal mass), not pcg_checks.geometry_of's: with unequal masses the
# right-hand side has a mean, for which the singular mode has no solution (eps = 0), or one with a constant of mean / eps (eps > 0);
# SuperLU on the oracle's K + (1e-14 + eps) M then returns a constant that large, and removing it costs the digits -- the host PCG,
# which removes the mean first, is then 4.5e-3 (eps = 0) and 2.4e-8 (eps = 1e-2, T = 1023) from it whatever cg_tol is and in
# np.longdouble too: the reference's error, not the PCG's.  The mean removal is what the iterate cases are for.
# Measured by test_pcg_windows_cpu.py::test_converged_error_and_bound: 3.7e-11 (T = 600, eps = 1e-2), unchanged at cg_tol = 1e-14.
CONVERGED_MEASURED = 5e-11
CONVERGED_BOUND = min(10.0 * CONVERGED_MEASURED, 1e-8)


def mesh_key(mesh):
    name, kw = mesh
    return name, tuple(sorted(kw.items()))


def problem(mesh, T, eps):
    """``(oracle, Problem)`` of the seeded state, as pcg_checks.seeded_problem plants it (computed once, read-only)."""
    return pc.seeded_problem(mesh_key(mesh), T, "modal_pcg", eps)


def remove_gauge(phi, mass):
    w = np.broadcast_to(mass[None, :], phi.shape)
    return phi - np.sum(phi * w) / np.sum(w)


@functools.lru_cache(maxsize=None)
def converged_geometry():
    from dots_socp_amd import meshes

    g = meshes.example(MESH[0], **MESH[1])[0]
    return dict(vertices=g["vertices"], triangles=g["triangles"], mu0=g["mu0"], mu1=g["mu1"])


@functools.lru_cache(maxsize=None)
def converged_case(T, eps):
    """``(oracle with the seeded state, Problem, phi of its step_laplacian)`` on the equal-mass sphere: the per-mode SuperLU solve, gauge
    removed at eps = 0.  Computed once, read-only (the oracle keeps the seeded state: the solve runs on a copy of phi)."""
    s = pc.seeded_oracle(T, converged_geometry(), eps, factorise=True)
    p = pc.problem_of(s, "modal_pcg")
    phi = s.lap_inv(s.laplacian_rhs())
    if eps == 0.0:
        phi = remove_gauge(phi, s.mass_v)
    phi.setflags(write=False)
    return s, p, phi

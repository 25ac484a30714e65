"""The cases of moved vertices on a live context (dots_move_vertices, DeviceProblem.move_vertices, AlmSolver.restart(vertices=),
SolveSession.solve(vertices=), transport_cost(move=True)), shared by test_move_cpu.py and test_hip_move.py (TEST INFRASTRUCTURE): the
three meshes of session_checks with one smooth displacement, the geometry dict of the moved mesh, the twin's plan and the numpy
specification of the per-corner tables the library derives."""
import numpy as np

import session_checks as sc
from dots_socp_amd import meshes

AMPLITUDE = 0.02
CASES, TOL = sc.CASES, sc.TOL


def displaced(vertices, a=AMPLITUDE):
    """v + a (sin(2 pi y + 0.3), sin(2 pi z + 0.7) cos(2 pi x), sin(2 pi x + 1.1)): smooth, bends the plane, changes the triangle areas
    of the three meshes by factors within 0.89 ... 1.13 at a = 0.02 (test_move_cpu.py checks that nothing degenerates)."""
    v = np.asarray(vertices, dtype=np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    two_pi = 2.0 * np.pi
    return v + a * np.stack([np.sin(two_pi * y + 0.3), np.sin(two_pi * z + 0.7) * np.cos(two_pi * x), np.sin(two_pi * x + 1.1)], axis=1)


def moved_mesh(mesh, moved):
    """The mesh dict (no masses) at the positions ``moved``, its areas refreshed as AlmSolver.restart(vertices=) refreshes them."""
    t = np.asarray(mesh["triangles"])
    area_t = meshes.triangle_areas(moved, t)
    return {**mesh, "vertices": np.array(moved, dtype=np.float64), "area_triangles": area_t,
            "area_vertices": meshes.vertex_areas(moved.shape[0], t, area_t)}


def moved_geometry(name, which=2, a=AMPLITUDE):
    mesh, p1, p2 = sc.problems(name)
    mu0, mu1 = p1 if which == 1 else p2
    return {**moved_mesh(mesh, displaced(mesh["vertices"], a)), "mu0": mu0, "mu1": mu1}


def twin_plan(plan, moved, mu0, mu1):
    """The plan of the twin: the session's numbering and tree, assembled from scratch on the moved mesh."""
    from dots_socp_amd import geometry

    return geometry.plan_with_densities(geometry.plan_with_vertices(plan, moved), mu0, mu1)


def derived_tables(plan):
    """The numpy specification of what dots_create derives per corner-list entry and per vertex from a plan (dots_api.hip: build):
    ``corner_scale[j] = sqrt(area[f] / mass[v])``, ``corner_grad_area[j] = hat[f, k] * area[f]`` for the entry j = (f, k) of vertex v,
    ``kdiag[v] = 0.0 + K[v, v]``."""
    cptr, cidx = np.asarray(plan.corner_ptr), np.asarray(plan.corner_idx)
    f = cidx // 3
    vertex = np.repeat(np.arange(plan.n_vertices), np.diff(cptr))
    area = plan.area_tri[f]
    corner_scale = np.sqrt(area / plan.mass_vert[vertex])
    corner_grad_area = plan.hat_grad.reshape(-1, 3)[cidx] * area[:, None]
    kdiag = np.zeros(plan.n_vertices)
    row = np.repeat(np.arange(plan.n_vertices), np.diff(plan.lap_rowptr))
    diag = plan.lap_col == row
    kdiag[row[diag]] = 0.0 + plan.lap_val[diag]
    return {"corner_scale": corner_scale, "corner_grad_area": corner_grad_area, "kdiag": kdiag}

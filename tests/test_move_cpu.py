"""CPU tests of moved vertices on a live context (no device): geometry.plan_with_vertices against the host assembly and the numpy
reference, the numpy specification of the derived tables (move_checks.derived_tables), the driver's calls on the recording stand-in of
DeviceProblem, the option checks of SolveSession.solve and transport_cost, and the two new structures against the header."""
import ctypes
import dataclasses
import importlib
import os
import subprocess

import numpy as np
import pytest

import move_checks as mc
import session_checks as sc
from conftest import ROOT
from dots_socp_amd import _lib, geometry, meshes

ss = importlib.import_module("dots_socp_amd.socp.solver_socp")
NAMES = tuple(sc.CASES)


def session_plan(name, which=1):
    return geometry.build_plan(sc.CASES[name][0], sc.geometry(name, which), reorder="nd")


# ---- the displacement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_displacement_degenerates_nothing(name):
    mesh = sc.problems(name)[0]
    moved = mc.displaced(mesh["vertices"])
    ratio = meshes.triangle_areas(moved, mesh["triangles"]) / meshes.triangle_areas(mesh["vertices"], mesh["triangles"])
    assert 0.89 <= ratio.min() and ratio.max() <= 1.13 and not np.array_equal(moved, mesh["vertices"])
    if name == "plane":      # a bent sheet
        assert np.ptp(mesh["vertices"][:, 2]) == 0.0 and np.ptp(moved[:, 2]) > 0.01


# ---- plan_with_vertices -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_plan_with_vertices_is_the_plan_of_the_moved_mesh_in_the_old_numbering(name):
    plan = session_plan(name)
    mesh = sc.problems(name)[0]
    moved = mc.displaced(mesh["vertices"])
    got = geometry.plan_with_vertices(plan, moved)
    assert got.perm_vert is plan.perm_vert and got.perm_tri is plan.perm_tri and got.dissection is plan.dissection
    assert got.triangles is plan.triangles and got.corner_ptr is plan.corner_ptr and got.corner_idx is plan.corner_idx
    assert got.lap_rowptr is plan.lap_rowptr and got.lap_col is plan.lap_col and got.mu0 is plan.mu0 and got.time_modes is plan.time_modes
    assert np.array_equal(got.vertices, moved[plan.perm_vert]) and got.area_mesh == float(got.area_tri.sum())
    # per-triangle quantities: un-permuted, the host assembly's on the moved mesh in the caller's numbering, bit for bit
    tri = np.asarray(mesh["triangles"])
    area, hat, _, _, _, _ = geometry.assemble_native(moved, tri)
    assert np.array_equal(got.area_tri, area[plan.perm_tri]) and np.array_equal(got.hat_grad, hat[plan.perm_tri])
    # masses and K against the numpy reference in the device numbering (tolerances: test_host_cpu.py,
    # test_native_assembly_matches_the_numpy_reference)
    _, _, mass0, cptr0, cidx0, K0 = geometry.assemble_reference(got.vertices, np.asarray(plan.triangles, dtype=np.int64))
    assert np.array_equal(cptr0, got.corner_ptr) and np.array_equal(cidx0, got.corner_idx)
    assert np.allclose(got.mass_vert, mass0, rtol=1e-15, atol=0)
    import scipy.sparse as sp

    K = sp.csr_matrix((got.lap_val, got.lap_col, got.lap_rowptr), shape=K0.shape)
    assert abs(K - K0).max() <= 1e-13 * abs(K0).max()
    assert abs(np.asarray(K.sum(axis=1))).max() <= 1e-12 * abs(K0).max()
    assert not np.array_equal(got.lap_val, plan.lap_val)
    # the same positions: the plan's own tables again
    back = geometry.plan_with_vertices(got, mesh["vertices"])
    for k in ("area_tri", "hat_grad", "mass_vert", "lap_val", "vertices"):
        assert np.array_equal(getattr(back, k), getattr(plan, k)), k


def test_plan_with_vertices_refuses_what_build_plan_refuses():
    plan = session_plan("plane")
    v = sc.problems("plane")[0]["vertices"]
    with pytest.raises(ValueError, match=r"vertices must have shape \(90, 3\), got \(89, 3\)"):
        geometry.plan_with_vertices(plan, v[:-1])
    bad = v.copy()
    bad[5, 1] = np.nan
    with pytest.raises(ValueError, match="vertices has entries that are not finite"):
        geometry.plan_with_vertices(plan, bad)
    flat = v.copy()
    t0 = plan.perm_vert[plan.triangles[0]]      # (a triangle of the plan, in the caller's numbering)
    flat[t0[1]] = flat[t0[0]]
    with pytest.raises(ValueError, match=r"degenerate triangle \(zero area\)"):
        geometry.plan_with_vertices(plan, flat)
    lonely = dataclasses.replace(plan, triangles=np.ascontiguousarray(plan.triangles[~np.any(plan.triangles == 0, axis=1)]))
    with pytest.raises(ValueError, match=r"isolated vertex \(no incident triangle\)"):
        geometry.plan_with_vertices(lonely, v)


# ---- the numpy specification of the derived tables ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_derived_tables_are_consistent_with_the_plan(name):
    plan = session_plan(name)
    d = mc.derived_tables(plan)
    F, V = plan.n_triangles, plan.n_vertices
    assert d["corner_scale"].shape == (3 * F,) and d["corner_grad_area"].shape == (3 * F, 3) and d["kdiag"].shape == (V,)
    tri = plan.triangles.reshape(-1)
    for v in (0, V // 2, V - 1):
        for j in range(plan.corner_ptr[v], plan.corner_ptr[v + 1]):
            fk = plan.corner_idx[j]
            assert tri[fk] == v
            assert d["corner_scale"][j] == np.sqrt(plan.area_tri[fk // 3] / plan.mass_vert[v])
            assert np.array_equal(d["corner_grad_area"][j], plan.hat_grad.reshape(-1, 3)[fk] * plan.area_tri[fk // 3])
    # sum over a vertex's corners of area = 3 mass; the diagonal of K is the sum of area |grad|^2 over them
    for v in range(V):
        js = slice(plan.corner_ptr[v], plan.corner_ptr[v + 1])
        assert np.isclose(np.sum(d["corner_scale"][js] ** 2), 3.0, rtol=1e-14)
        g = d["corner_grad_area"][js]
        area = plan.area_tri[plan.corner_idx[js] // 3]
        assert np.isclose(np.sum(np.sum(g * g, axis=1) / area), d["kdiag"][v], rtol=1e-13)
    assert np.all(d["kdiag"] > 0)


# ---- the driver on the recording stand-in ---------------------------------------------------------------------------------------------
def test_restart_with_vertices_moves_first_once_and_refreshes_the_geometry(monkeypatch):
    solver = sc.recording_solver(monkeypatch.setattr)
    mesh, _, p2 = sc.problems("plane")
    old = solver.geometry
    moved = mc.displaced(mesh["vertices"])
    before = len(solver.dev.calls)
    solver.restart(*p2, warm=False, vertices=moved)
    calls = solver.dev.calls[before:]
    assert calls[:2] == ["move_vertices", "restart cold"] and calls.count("move_vertices") == 1
    want = mc.moved_mesh(mesh, moved)
    assert set(solver.geometry) == set(old) | {"area_triangles", "area_vertices"}
    for k in ("vertices", "area_triangles", "area_vertices"):
        assert np.array_equal(solver.geometry[k], want[k]), k
    assert solver.geometry["triangles"] is old["triangles"]
    assert np.array_equal(solver.geometry["mu1"], p2[1]) and np.array_equal(old["vertices"], mesh["vertices"])
    assert solver.geometry["vertices"] is not moved      # (a copy: the caller's array is not the solver's)


def test_restart_without_vertices_makes_todays_calls(monkeypatch):
    a = sc.recording_solver(monkeypatch.setattr)
    _, _, p2 = sc.problems("plane")
    before = len(a.dev.calls)
    a.restart(*p2, warm=False)
    assert a.dev.calls[before:] == ["restart cold", "set_params", "scale_z", "set_params"]
    assert a.move_ms is None and "move_vertices" not in a.dev.calls


@pytest.mark.parametrize("refusal", ("closed", "slab", "cascade", "batch"))
def test_the_refusals_of_restart_hold_with_vertices(monkeypatch, refusal):
    solver = sc.recording_solver(monkeypatch.setattr, **({"batched": True} if refusal == "batch" else {}))
    mesh, _, p2 = sc.problems("plane")
    if refusal == "closed":
        solver.close()
    elif refusal == "slab":
        solver.dev.slab = (0, 2, 4)
    elif refusal == "cascade":
        solver._init_from = True
    text = {"closed": "the solver is closed", "slab": "not available on time slabs", "cascade": "started from init_from", "batch": "stepped by a batch"}
    with pytest.raises(ValueError, match="restart: .*" + text[refusal]):
        solver.restart(*p2, vertices=mc.displaced(mesh["vertices"]))
    assert "move_vertices" not in solver.dev.calls


def test_session_solve_checks_vertices_before_the_library_loads():
    loaded = _lib._lib
    mesh, _, (mu0, mu1) = sc.problems("plane")
    s = ss.SolveSession(7, mesh, tol=sc.TOL)
    with pytest.raises(ValueError, match=r"SolveSession.solve: vertices must have shape \(90, 3\), got \(90, 2\)"):
        s.solve(mu0, mu1, vertices=mesh["vertices"][:, :2])
    bad = mesh["vertices"].copy()
    bad[0, 0] = np.inf
    with pytest.raises(ValueError, match="SolveSession.solve: vertices has entries that are not finite"):
        s.solve(mu0, mu1, vertices=bad)
    with pytest.raises(ValueError, match=r"SolveSession.solve: unknown option\(s\) \['move'\]"):
        s.solve(mu0, mu1, move=True)
    assert s.alm is None and s.index == 0 and _lib._lib is loaded


def test_session_solve_hands_the_vertices_to_restart_and_follows_the_move():
    mesh, p1, p2 = sc.problems("plane")
    moved = mc.displaced(mesh["vertices"])
    seen = []

    class Solver:
        nit, congestion0 = 0, 0.0

        def __init__(self, geom):
            self.geometry, self.move_ms = geom, None

        def restart(self, mu0, mu1, warm=True, vertices=None, **kw):
            seen.append((warm, vertices))
            if vertices is not None:
                self.geometry, self.move_ms = {**mc.moved_mesh(mesh, vertices), "mu0": mu0, "mu1": mu1}, (0.1, 0.2, 0.4)
            return 0.5

        def finalize(self, **kw):
            return {}, type("Hist", (), {"solver_stats": {}})()

        def close(self):
            pass

    s = ss.SolveSession(7, mesh, tol=sc.TOL)
    s.alm = Solver({**mesh, "mu0": p1[0], "mu1": p1[1]})
    _, hist = s.solve(*p2, warm=False, vertices=moved)
    assert seen[-1][0] is False and np.array_equal(seen[-1][1], moved)
    assert hist.solver_stats["session"]["moved"] is True and hist.solver_stats["session"]["move_ms"] == (0.1, 0.2, 0.4)
    assert np.array_equal(s.geometry["vertices"], moved) and "mu0" not in s.geometry
    _, hist = s.solve(*p2)
    assert seen[-1] == (True, None) and hist.solver_stats["session"]["moved"] is False and hist.solver_stats["session"]["move_ms"] is None


def test_the_torch_function_checks_move_first():
    torch = pytest.importorskip("torch")
    from dots_socp_amd import torch_cost

    mesh, _, (mu0, mu1) = sc.problems("plane")
    with pytest.raises(ValueError, match="transport_cost: 'move' needs a session"):
        torch_cost.transport_cost(mu0, mu1, mesh["vertices"], mesh["triangles"], 7, move=True)
    s = ss.SolveSession(7, mesh, tol=sc.TOL)
    moved = mesh["vertices"].copy()
    moved[3, 0] += 1e-9
    m0, m1 = torch.tensor(mu0), torch.tensor(mu1)
    with pytest.raises(ValueError, match=r"transport_cost: vertices / triangles are not the session's \(a session solves on one mesh; moved "
                                         r"vertices need a new session\)$"):
        torch_cost.transport_cost(m0, m1, moved, mesh["triangles"], 7, session=s, move=False)
    other = np.asarray(mesh["triangles"])[:, [1, 2, 0]]
    with pytest.raises(ValueError, match="move=True moves the vertices, the triangles must be the session's"):
        torch_cost.transport_cost(m0, m1, moved, other, 7, session=s, move=True)
    with pytest.raises(ValueError, match=r"transport_cost: vertices must have the session's shape \(90, 3\), got \(89, 3\)"):
        torch_cost.transport_cost(m0, m1, moved[:-1], mesh["triangles"], 7, session=s, move=True)
    assert s.alm is None


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_the_built_library_exports_the_two_calls():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("dots_move_vertices", "dots_geometry_copy"):
        assert name in _lib.EXPORTS and name in names
    # exports.map lists the C ABI by its prefix: both names fall under it, and nothing else does
    text = open(os.path.join(ROOT, "dots_socp_amd", "csrc", "exports.map")).read()
    assert "global: dots_*;" in text and "local: *;" in text
    assert "kernels_geometry.hip" in importlib.import_module("dots_socp_amd.build").SOURCES
    assert _lib.ABI_VERSION == 7


def test_the_two_structures_match_the_header(tmp_path):
    move = ("vertices", "device_pointers", "reserved", "ms")
    src = tmp_path / "probe.c"
    prints = ['printf("%zu\\n", sizeof(dots_move_desc));'] + [f'printf("%zu\\n", offsetof(dots_move_desc, {m}));' for m in move]
    prints += ['printf("%zu\\n", sizeof(dots_geometry_tables));'] + [f'printf("%zu\\n", offsetof(dots_geometry_tables, {m}));' for m in _lib.GeometryTables.NAMES]
    prints.append('printf("%d\\n", DOTS_ABI_VERSION);')
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dots_socp_hip.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "probe"
    assert os.system(f"gcc -I{ROOT}/include {src} -o {exe}") == 0
    got = [int(x) for x in os.popen(str(exe)).read().split()]
    want = [ctypes.sizeof(_lib.MoveDesc)] + [getattr(_lib.MoveDesc, m).offset for m in move]
    want += [ctypes.sizeof(_lib.GeometryTables)] + [getattr(_lib.GeometryTables, m).offset for m in _lib.GeometryTables.NAMES]
    assert got == want + [7]

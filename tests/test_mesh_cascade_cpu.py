"""CPU tests of the coarse-to-fine cascade in space: the nested refinement (meshes.subdivide, refine_levels), the transfer of a solution
from a mesh to its refinement as specified in dots_socp_amd/cascade.py (prolong_space), the row maps the device kernel reads against
that specification under independent renumberings of the two meshes, and the argument checks of the driver."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dots_socp_amd import _lib, cascade, meshes

STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")


def on_sphere(p):
    return p / np.linalg.norm(p, axis=1, keepdims=True)


MESHES = {
    "icosphere": lambda: meshes.icosphere(1) + (on_sphere,),
    "torus": lambda: meshes.torus(8, 6) + (meshes.snap_projection(meshes.torus(16, 12)[0]),),
    "plane": lambda: meshes.plane(4) + (None,),
}


def shapes(n, V, F):
    return {"phi": (n + 1, V), "B": (n + 1, F, 3), "E": (n + 1, F, 3), "z_mid": (n, 2, 3, F, 3), "beta_mid": (n, 2, 3, F, 3),
            **{k: (n, V) for k in ("A", "lambda_c", "z_fst", "z_end", "mu", "beta_fst", "beta_end")}}


def euler(v, t):
    return v.shape[0] - meshes._unique_edges(t).shape[0] + t.shape[0]


def test_library_exports_the_space_prolongation():
    lib = _lib.load(host_only=True)
    assert "dots_prolong_space" in _lib.EXPORTS
    assert hasattr(lib, "dots_prolong_space")
    assert _lib.ABI_VERSION == 7      # an addition: the ABI version stays


def test_header_declares_the_space_prolongation(tmp_path):
    import ctypes as C

    text = open(os.path.join(ROOT, "include", "dots_socp_hip.h")).read()
    assert "int dots_prolong_space(dots_ctx *dst, dots_ctx *src, const dots_prolong_space_desc *desc);" in text
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dots_socp_hip.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(dots_prolong_space_desc), offsetof(dots_prolong_space_desc, n_triangles),'
                   " offsetof(dots_prolong_space_desc, factor), offsetof(dots_prolong_space_desc, ms)); return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = _lib.ProlongSpaceDesc
    assert out == [C.sizeof(D), D.n_triangles.offset, D.factor.offset, D.ms.offset]


@pytest.mark.parametrize("name", sorted(MESHES))
def test_subdivide(name):
    v, t, project = MESHES[name]()
    calls = []

    def spy(p):
        calls.append(np.array(p))
        return p if project is None else project(p)

    vf, tf, parents = meshes.subdivide(v, t, project=spy)
    edges = meshes._unique_edges(t)
    Vc, Fc = v.shape[0], t.shape[0]
    assert vf.shape == (Vc + edges.shape[0], 3) and tf.shape == (4 * Fc, 3)
    assert euler(vf, tf) == euler(v, t)
    assert np.array_equal(vf[:Vc], v)
    # the projection sees the new vertices only: the midpoints of the edges, in the order of _unique_edges
    assert len(calls) == 1 and np.array_equal(calls[0], (v[edges[:, 0]] + v[edges[:, 1]]) * 0.5)
    vp, tp = parents["vertex_parents"], parents["triangle_parent"]
    assert vp.dtype == np.int32 and vp.shape == (vf.shape[0], 2) and tp.shape == (4 * Fc,)
    assert np.array_equal(vp[:Vc, 0], np.arange(Vc)) and np.array_equal(vp[:Vc, 1], np.arange(Vc))
    assert np.array_equal(vp[Vc:], edges)
    assert np.array_equal(tp, np.arange(4 * Fc) // 4)
    # the children of (a, b, c): (a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)
    mid = {tuple(e): Vc + i for i, e in enumerate(edges.tolist())}
    for f in (0, Fc // 2, Fc - 1):
        a, b, c = (int(x) for x in t[f])
        ab, bc, ca = mid[tuple(sorted((a, b)))], mid[tuple(sorted((b, c)))], mid[tuple(sorted((c, a)))]
        assert tf[4 * f:4 * f + 4].tolist() == [[a, ab, ca], [ab, b, bc], [ca, bc, c], [ab, bc, ca]]
    # the orientation is kept: on the flat mesh every child has the parent's normal, and the area is preserved
    if name == "plane":
        assert abs(meshes.triangle_areas(vf, tf).sum() - meshes.triangle_areas(v, t).sum()) <= 1e-14
        n = np.cross(vf[tf[:, 1]] - vf[tf[:, 0]], vf[tf[:, 2]] - vf[tf[:, 0]])[:, 2]
        n0 = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])[:, 2]
        assert np.all(np.sign(n) == np.sign(n0)[tp])
    if name == "icosphere":
        assert np.allclose(np.linalg.norm(vf, axis=1), 1.0, atol=1e-15)
        assert vf.shape[0] == 162
    if name == "torus":      # the refinement lies on the generator's own grid
        fine = meshes.torus(16, 12)[0]
        assert {tuple(p) for p in vf.tolist()} == {tuple(p) for p in fine.tolist()}


def test_projection_must_keep_the_count():
    v, t = meshes.plane(4)
    with pytest.raises(ValueError):
        meshes.subdivide(v, t, project=lambda p: p[:-1])


@pytest.mark.parametrize("name", sorted(MESHES))
def test_prolong_space_properties(name):
    v, t, project = MESHES[name]()
    vf, tf, parents = meshes.subdivide(v, t, project)
    Vc, Fc, n = v.shape[0], t.shape[0], 3
    src, dst = shapes(n, Vc, Fc), shapes(n, vf.shape[0], tf.shape[0])
    rng = np.random.default_rng(5)
    for k in STATE:
        for c in (0.3, -1.7e-5, 1.0 / 3.0):      # constants, bit for bit
            out = cascade.prolong_space(np.full(src[k], c), k, parents)
            assert out.shape == dst[k], k
            assert np.array_equal(out, np.full(dst[k], c)), k
        x = rng.standard_normal(src[k])
        out = cascade.prolong_space(x, k, parents)
        assert out.shape == dst[k] and out.dtype == np.float64
        if k in cascade.VERTEX_ARRAYS:
            assert np.array_equal(out[:, :Vc], x)      # kept vertices are copies
            p = parents["vertex_parents"][Vc:]
            assert np.array_equal(out[:, Vc:], (x[:, p[:, 0]] + x[:, p[:, 1]]) * 0.5)
        elif k in cascade.TRIANGLE_ARRAYS:
            for child in range(4):
                assert np.array_equal(out[:, child::4], x)
        else:
            for child in range(4):
                assert np.array_equal(out[:, :, :, child::4], x)
    sol = {k: rng.standard_normal(src[k]) for k in STATE}
    sol["checkpoints"] = None
    up = cascade.prolong_space_solution(sol, parents)
    assert set(up) == set(STATE) and all(up[k].shape == dst[k] for k in STATE)


def test_linear_functions_are_reproduced_on_the_plane():
    v, t = meshes.plane(4)
    vf, _, parents = meshes.subdivide(v, t)
    lin = lambda p: 0.7 * p[:, 0] - 1.3 * p[:, 1] + 0.25      # noqa: E731
    for k in cascade.VERTEX_ARRAYS:
        rows = 4 if k == "phi" else 3
        out = cascade.prolong_space(np.tile(lin(v), (rows, 1)), k, parents)
        assert np.max(np.abs(out - lin(vf)[None, :])) <= 1e-15, k


def test_prolong_space_checks_its_input():
    v, t = meshes.plane(4)
    _, _, parents = meshes.subdivide(v, t)
    V, F = v.shape[0], t.shape[0]
    with pytest.raises(ValueError):
        cascade.prolong_space(np.zeros((3, V)), "rho", parents)
    with pytest.raises(ValueError):
        cascade.prolong_space(np.zeros((3, V + 1)), "mu", parents)          # parents of another mesh
    with pytest.raises(ValueError):
        cascade.prolong_space(np.zeros((3, V - 1)), "mu", parents)
    with pytest.raises(ValueError):
        cascade.prolong_space(np.zeros((4, F + 2, 3)), "B", parents)
    with pytest.raises(ValueError):
        cascade.prolong_space(np.zeros((3, 2, 3, F - 1, 3)), "z_mid", parents)
    with pytest.raises(ValueError):
        cascade.prolong_space(np.zeros((3, V)), "B", parents)               # not the layout of B
    with pytest.raises(ValueError):
        cascade.prolong_space(np.zeros((3, V)), "mu", {"vertex_parents": parents["vertex_parents"]})
    with pytest.raises(ValueError):
        cascade.prolong_space(np.zeros((3, V)), "mu", {"vertex_parents": parents["vertex_parents"][:, :1], "triangle_parent": parents["triangle_parent"]})


def device_rows(x, name, perm_v, perm_f):
    """The rows of the device layout of a reference-layout array in the numbering ``perm`` (device row i = caller entity perm[i]),
    time along the last axis: vertex arrays (V, n), triangle arrays (3F, n), corner arrays (18F, n) with row ((f*3+k)*2+s)*3+c."""
    if name in cascade.VERTEX_ARRAYS:
        return np.ascontiguousarray(x[:, perm_v].T)
    if name in cascade.TRIANGLE_ARRAYS:
        return np.ascontiguousarray(x[:, perm_f, :].transpose(1, 2, 0)).reshape(-1, x.shape[0])
    return np.ascontiguousarray(x[:, :, :, perm_f, :].transpose(3, 2, 1, 4, 0)).reshape(-1, x.shape[0])      # [f][k][s][c][t]


@pytest.mark.parametrize("name", sorted(MESHES))
@pytest.mark.parametrize("permuted", [(True, True), (True, False), (False, True), (False, False)])
def test_row_maps_against_the_specification(name, permuted):
    """What the kernel does with the row maps, done in numpy on rows in device order, equals the specification in device order."""
    v, t, project = MESHES[name]()
    vf, tf, parents = meshes.subdivide(v, t, project)
    Vc, Fc, Vf, Ff, n = v.shape[0], t.shape[0], vf.shape[0], tf.shape[0], 2
    rng = np.random.default_rng(17)
    pvs, pfs = (rng.permutation(Vc), rng.permutation(Fc)) if permuted[0] else (None, None)
    pvd, pfd = (rng.permutation(Vf), rng.permutation(Ff)) if permuted[1] else (None, None)
    vmap, fmap = cascade.space_row_maps(parents, Vc, Fc, pvd, pfd, pvs, pfs)
    assert vmap.dtype == np.int32 and vmap.shape == (Vf, 2) and fmap.dtype == np.int32 and fmap.shape == (Ff,)
    assert vmap.min() >= 0 and vmap.max() < Vc and fmap.min() >= 0 and fmap.max() < Fc
    ident = lambda p, m: np.arange(m) if p is None else p      # noqa: E731
    src, dst = shapes(n, Vc, Fc), shapes(n, Vf, Ff)
    for k in STATE:
        x = rng.standard_normal(src[k])
        want = device_rows(cascade.prolong_space(x, k, parents), k, ident(pvd, Vf), ident(pfd, Ff))
        rows = device_rows(x, k, ident(pvs, Vc), ident(pfs, Fc))
        if k in cascade.VERTEX_ARRAYS:
            a, b = rows[vmap[:, 0]], rows[vmap[:, 1]]
            got = np.where((vmap[:, 0] == vmap[:, 1])[:, None], a, (a + b) * 0.5)
        else:
            rpe = 3 if k in cascade.TRIANGLE_ARRAYS else 18
            got = rows[(fmap[:, None] * rpe + np.arange(rpe)[None, :]).reshape(-1)]
        assert got.shape == want.shape and np.array_equal(got, want), k
        assert dst[k][0] == want.shape[1]
    with pytest.raises(ValueError):
        cascade.space_row_maps(parents, Vc + 1, Fc)
    with pytest.raises(ValueError):
        cascade.space_row_maps(parents, Vc, Fc, perm_vert_dst=np.arange(Vf - 1))


def test_refine_levels():
    geom, _ = meshes.make_geometry(*meshes.icosphere(1))
    c = meshes.farthest_vertices(geom["vertices"], 0, 3)
    geom["mu0"] = meshes.bump_density(geom["vertices"], geom["area_vertices"], [c[0]], 0.6, 0.2)
    geom["mu1"] = meshes.bump_density(geom["vertices"], geom["area_vertices"], [c[1], c[2]], 0.6, 0.2)
    centre = geom["vertices"].mean(axis=0)
    radius = np.linalg.norm(geom["vertices"][0] - centre)
    project = lambda p: centre + radius * on_sphere(p - centre)      # noqa: E731
    given = lambda vv, av: (meshes.bump_density(vv, av, [c[0]], 0.6, 0.2), meshes.bump_density(vv, av, [c[1], c[2]], 0.6, 0.2))      # noqa: E731
    for densities in (None, given):
        levels = meshes.refine_levels(geom, 3, project=project, densities=densities)
        assert len(levels) == 3 and levels[0] is geom and "parents" not in levels[0]
        assert [g["vertices"].shape[0] for g in levels] == [42, 162, 642]
        for coarse, fine in zip(levels, levels[1:]):
            Vc = coarse["vertices"].shape[0]
            assert np.array_equal(fine["vertices"][:Vc], coarse["vertices"])
            assert np.allclose(np.linalg.norm(fine["vertices"] - centre, axis=1), radius, atol=1e-14)
            cascade.check_parents(fine["parents"], n_vertices=Vc, n_triangles=coarse["triangles"].shape[0])
            for k in ("mu0", "mu1"):
                assert fine[k].shape == (fine["vertices"].shape[0],) and np.all(fine[k] >= 0)
                assert abs(fine[k].sum() - 1.0) <= 1e-14
            assert set(fine) >= {"vertices", "triangles", "edges", "area_triangles", "area_vertices", "mu0", "mu1", "parents"}
        if densities is None:      # the density per unit area is what is carried up: a kept vertex keeps its value up to the normalisation
            rho_c, rho_f = levels[0]["mu0"] / levels[0]["area_vertices"], levels[1]["mu0"] / levels[1]["area_vertices"]
            ratio = rho_f[:42][rho_c > 0] / rho_c[rho_c > 0]
            assert np.allclose(ratio, ratio[0], rtol=1e-12)
    assert len(meshes.refine_levels(geom, 1)) == 1
    with pytest.raises(ValueError):
        meshes.refine_levels(geom, 0)
    with pytest.raises(ValueError):
        meshes.refine_levels(geom, 3, project=[project])


class _Finalised:
    """What the argument checks of AlmSolver read of ``init_from``, without a device"""
    finalized = True

    def __init__(self, n_time):
        self.n_time = n_time


def test_argument_errors_before_any_device_call():
    from dots_socp_amd.socp import solver_socp_mesh_cascade, solver_raw_mesh_cascade
    from dots_socp_amd.socp.solver_socp import AlmSolver

    geom, _ = meshes.make_geometry(*meshes.icosphere(1))
    geom["mu0"] = geom["mu1"] = np.full(42, 1.0 / 42)
    levels = meshes.refine_levels(geom, 2, project=on_sphere)
    parents = levels[1]["parents"]
    with pytest.raises(ValueError, match="time grid"):
        AlmSolver(15, levels[1], init_from=_Finalised(7), init_parents=parents)       # mesh and time grid in one call
    with pytest.raises(ValueError, match="init_from"):
        AlmSolver(15, levels[1], init_parents=parents)
    with pytest.raises(ValueError, match="two geometries"):
        solver_socp_mesh_cascade(7, [levels[1]])
    with pytest.raises(ValueError, match="two geometries"):
        solver_socp_mesh_cascade(7, [])
    with pytest.raises(ValueError):
        solver_raw_mesh_cascade(7, [])
    with pytest.raises(ValueError, match="parents"):
        solver_socp_mesh_cascade(7, [levels[0], {k: v for k, v in levels[1].items() if k != "parents"}])
    with pytest.raises(ValueError, match="parents"):
        solver_socp_mesh_cascade(7, [levels[1], levels[1]])                              # not the refinement of the level below
    with pytest.raises(ValueError, match="levels"):
        solver_socp_mesh_cascade(7, levels, levels=[3, 7])                               # no cascade in time in the same call
    with pytest.raises(ValueError):
        solver_socp_mesh_cascade(7, levels, init_from=None)
    with pytest.raises(ValueError):
        solver_socp_mesh_cascade(7, levels, level_tol=-1.0)
    with pytest.raises(ValueError):
        solver_socp_mesh_cascade(7, levels, no_such_option=1)
    with pytest.raises(ValueError):
        solver_socp_mesh_cascade(7, levels, nit=0)

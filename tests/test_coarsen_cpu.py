"""CPU tests of the levels a cascade in space makes of ONE mesh: the native coarsener (dots_coarsen, host code of the library) against
its specification in plain Python (meshes.coarsen(backend="python")) array for array, the properties of the coarse meshes, the
refusals, the exact location (cascade.locate_exact) against closest_on_triangles over all triangles, the restriction of the densities,
the levels meshes.coarsen_levels builds, the option checks of the one-geometry driver, and a run of the coarsener's translation unit
as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dots_socp_amd import _lib, cascade, meshes

MESHES = {
    "icosphere": lambda: meshes.icosphere(3),
    "torus": lambda: meshes.torus(64, 40),
    "knot": lambda: meshes.torus_knot_tube(nu=72, nv=8),
    "plane12": lambda: meshes.plane(12),
    "plane20": lambda: meshes.plane(20),
}
COUNTS = {"icosphere": (642, 160), "torus": (2560, 640), "knot": (576, 144), "plane12": (182, 45), "plane20": (504, 126)}
_cache = {}


def fine(name):
    if ("fine", name) not in _cache:
        _cache["fine", name] = MESHES[name]()
    return _cache["fine", name]


def coarse(name):
    """(vertices_c, triangles_c, kept) of the native coarsener at ratio 4, computed once"""
    if ("coarse", name) not in _cache:
        _cache["coarse", name] = meshes.coarsen(*fine(name))
    return _cache["coarse", name]


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def edge_use(t):
    """directed edges (3F, 2) and, per undirected edge, how many triangles hold it"""
    directed = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=0)
    und, count = np.unique(np.sort(directed, axis=1), axis=0, return_counts=True)
    return directed, und, count


def euler(v, t):
    return v.shape[0] - edge_use(t)[1].shape[0] + t.shape[0]


def boundary_loops(v, t):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    _, und, count = edge_use(t)
    b = und[count == 1]
    if b.shape[0] == 0:
        return 0
    on = np.unique(b)
    idx = np.searchsorted(on, b)
    g = coo_matrix((np.ones(b.shape[0]), (idx[:, 0], idx[:, 1])), shape=(on.size, on.size))
    return connected_components(g, directed=False)[0]


@pytest.mark.parametrize("name", list(MESHES))
def test_native_equals_the_specification(name):
    v, t = fine(name)
    assert same(meshes.coarsen(v, t, backend="python"), coarse(name))


def test_native_equals_the_specification_on_a_second_step_and_an_explicit_count():
    vc, tc, _ = coarse("icosphere")
    second = meshes.coarsen(vc, tc)
    assert second[0].shape[0] == 40 and same(meshes.coarsen(vc, tc, backend="python"), second)
    v, t = fine("torus")
    explicit = meshes.coarsen(v, t, n_vertices=1000)
    assert explicit[0].shape[0] == 1000 and same(meshes.coarsen(v, t, n_vertices=1000, backend="python"), explicit)
    assert same(meshes.coarsen(v, t, ratio=2.5), meshes.coarsen(v, t, n_vertices=1024))


@pytest.mark.parametrize("name", list(MESHES))
def test_properties_of_the_coarse_mesh(name):
    v, t = fine(name)
    vc, tc, kept = coarse(name)
    assert (v.shape[0], vc.shape[0]) == COUNTS[name]
    assert kept.dtype == np.int64 and tc.dtype == np.int64 and np.all(np.diff(kept) > 0)
    assert np.array_equal(vc.view(np.uint64), v[kept].view(np.uint64))
    assert tc.min() == 0 and tc.max() == vc.shape[0] - 1
    directed, _, count = edge_use(tc)
    assert count.min() >= 1 and count.max() <= 2
    assert np.unique(directed, axis=0).shape[0] == directed.shape[0]      # an interior edge is crossed once in either direction
    assert euler(vc, tc) == euler(v, t)
    assert boundary_loops(vc, tc) == boundary_loops(v, t)
    assert np.all(meshes.triangle_areas(vc, tc) > 0.0)
    if name.startswith("plane"):
        a_f, a_c = meshes.triangle_areas(v, t).sum(), meshes.triangle_areas(vc, tc).sum()
        assert abs(a_c - a_f) <= 1e-12 * a_f
    assert same(meshes.coarsen(v, t), coarse(name))      # two calls, one output


def test_second_level_of_the_icosphere_keeps_the_sphere():
    vc, tc, _ = coarse("icosphere")
    v2, t2, kept2 = meshes.coarsen(vc, tc)
    assert v2.shape[0] == 40 and euler(v2, t2) == 2 and boundary_loops(v2, t2) == 0
    assert np.array_equal(v2, vc[kept2])


TETRA = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]))


@pytest.mark.parametrize("backend", ["native", "python"])
def test_refusals(backend):
    v, t = fine("plane12")
    bad = {}
    bad["more than two"] = (np.concatenate([v, [[0.5, 0.5, 1.0]]]), np.concatenate([t, [[t[0, 0], t[0, 1], v.shape[0]], [t[0, 1], t[0, 0], v.shape[0]]]]))
    bad["same direction"] = (np.concatenate([v, [[0.5, 0.5, 1.0]]]), np.concatenate([t, [[t[0, 0], t[0, 1], v.shape[0]]]]))
    flat = v.copy()
    flat[t[5, 2]] = flat[t[5, 0]]      # (two corners of triangle 5 in one point)
    bad["zero area"] = (flat, t)
    out = t.copy()
    out[3, 1] = v.shape[0]
    bad["out of range"] = (v, out)
    negative = t.copy()
    negative[3, 1] = -1
    bad["out of range "] = (v, negative)
    nan = v.copy()
    nan[7, 2] = np.nan
    bad["non-finite"] = (nan, t)
    inf = v.copy()
    inf[0, 0] = np.inf
    bad["non-finite "] = (inf, t)
    for match, (bv, bt) in bad.items():
        with pytest.raises(ValueError, match=match.strip()):
            meshes.coarsen(bv, bt, backend=backend)
    for ratio in (1.0, 0.5, -4.0, float("nan")):
        with pytest.raises(ValueError, match="ratio"):
            meshes.coarsen(v, t, ratio=ratio, backend=backend)
    with pytest.raises(ValueError):
        meshes.coarsen(v, t, backend="no such backend")


def test_entry_point_status_codes():
    lib = _lib.load(host_only=True)
    import ctypes as C

    v, t = TETRA
    v, t = np.ascontiguousarray(v), np.ascontiguousarray(t, dtype=np.int32)
    h = C.c_void_p()
    args = (v.ctypes.data_as(_lib._f64p), t.ctypes.data_as(_lib._i32p))
    assert lib.dots_coarsen(4, 4, *args, 0, C.byref(h)) == _lib.ERR_ARGUMENT
    assert lib.dots_coarsen(0, 4, *args, 1, C.byref(h)) == _lib.ERR_ARGUMENT
    assert lib.dots_coarsen(4, 4, None, args[1], 1, C.byref(h)) == _lib.ERR_ARGUMENT
    assert lib.dots_coarsen(3, 4, *args, 1, C.byref(h)) == _lib.ERR_ARGUMENT and b"out of range" in lib.dots_last_error()
    assert lib.dots_coarsen_vertices(None) == -1 and lib.dots_coarsen_copy(None, None, None) == _lib.ERR_ARGUMENT
    assert lib.dots_abi_version() == 7


def test_a_tetrahedron_comes_back_unchanged():
    v, t = TETRA
    for backend in ("native", "python"):
        vc, tc, kept = meshes.coarsen(v, t, n_vertices=1, backend=backend)
        assert np.array_equal(vc, v) and np.array_equal(tc, t) and np.array_equal(kept, np.arange(4))
    geom, _ = meshes.make_geometry(v, t, normalize=False)
    with pytest.raises(ValueError, match=r"4 vertices.* 4 "):
        meshes.coarsen_levels(geom, 2, locate="exact")


# ---- exact location --------------------------------------------------------------------------------------------------------------
def brute_force(p, v, t):
    """closest_on_triangles on every pair: weights (N, F, 3) and distances (N, F)"""
    n, f = p.shape[0], t.shape[0]
    w, d = cascade.closest_on_triangles(np.repeat(p, f, axis=0), np.tile(v[t[:, 0]], (n, 1)), np.tile(v[t[:, 1]], (n, 1)), np.tile(v[t[:, 2]], (n, 1)))
    return w.reshape(n, f, 3), d.reshape(n, f)


@pytest.mark.parametrize("name", list(MESHES))
def test_locate_exact_against_the_vectorised_region_test(name):
    """Against closest_on_triangles and argmin over all triangles: the same triangle, weights to 1e-12.  A point whose closest point
    lies on an edge or a vertex of the coarse mesh (every fine vertex on the convex side of a crease) is equally far from all the
    triangles around it; the two implementations round those equal distances differently (einsum has no fixed summation order), so
    which of the tied triangles comes first is not comparable between them.  There the located triangle must be one of the tied ones:
    its distance by closest_on_triangles is within 1e-12 of the smallest, and the weights are compared on the located triangle.
    Measured: 0 of 182 / 504 points differ on the planes, 23 of 642 on the icosphere, 67 of 2 560 on the torus, 11 of 576 on the knot."""
    v, t = fine(name)
    vc, tc, kept = coarse(name)
    tri, w, d = cascade.locate_exact(v, vc, tc)
    assert tri.dtype == np.int64 and w.shape == (v.shape[0], 3) and d.shape == (v.shape[0],)
    want_w, want_d = brute_force(v, vc, tc)
    rows = np.arange(v.shape[0])
    first = np.argmin(want_d, axis=1)
    print(f"{name}: {int((tri != first).sum())} of {v.shape[0]} points on another of several equally close triangles")
    assert np.max(want_d[rows, tri] - want_d[rows, first]) <= 1e-12
    apart = np.sort(want_d, axis=1)[:, 1] - want_d[rows, first] > 1e-12      # no second triangle within 1e-12: the same triangle
    assert np.array_equal(tri[apart], first[apart])
    assert np.max(np.abs(w - want_w[rows, tri])) <= 1e-12 and np.max(np.abs(d - want_d[rows, tri])) <= 1e-12
    assert np.all(w >= 0.0) and np.max(np.abs(w.sum(axis=1) - 1.0)) <= 4 * np.finfo(float).eps
    # a kept vertex is a coarse vertex: distance exactly 0, on the incident triangle of the smallest index
    assert np.all(d[kept] == 0.0)
    first_incident = np.full(vc.shape[0], tc.shape[0], dtype=np.int64)
    for k in range(3):
        np.minimum.at(first_incident, tc[:, k], np.arange(tc.shape[0]))
    assert np.array_equal(tri[kept], first_incident)


def test_locate_exact_clamps_beyond_a_boundary_and_refuses_bad_input():
    vc, tc, _ = coarse("plane12")
    p = np.array([[-0.3, 0.4, 0.0], [0.5, 0.5, 0.25], [1.7, -0.2, 0.1]])
    tri, w, d = cascade.locate_exact(p, vc, tc)
    q = np.einsum("ik,ikc->ic", w, vc[tc[tri]])
    assert np.all(w >= 0.0) and np.allclose(w.sum(axis=1), 1.0, atol=1e-15)
    assert np.allclose(np.linalg.norm(p - q, axis=1), d, atol=1e-15)
    assert d[0] >= 0.3 and d[2] >= 0.7 and (w[0] == 0.0).sum() >= 1 and (w[2] == 0.0).sum() >= 1      # beyond the boundary: on an edge or a corner
    assert abs(d[1] - 0.25) < 1e-15 and np.all(w[1] > 0.0)                                                 # above the patch: inside a triangle
    _, all_d = brute_force(p, vc, tc)
    assert np.max(np.abs(d - all_d.min(axis=1))) <= 1e-12
    assert q[:, 0].min() >= -1e-15 and q[:, 0].max() <= vc[:, 0].max() + 1e-15
    with pytest.raises(ValueError, match="non-finite"):
        cascade.locate_exact(np.array([[np.nan, 0.0, 0.0]]), vc, tc)
    with pytest.raises(ValueError, match="zero area"):
        cascade.locate_exact(p, vc, np.concatenate([tc, [[0, 0, 1]]]))
    with pytest.raises(ValueError):
        cascade.locate_exact(p, vc, np.concatenate([tc, [[0, 1, vc.shape[0]]]]))


def test_mesh_locate_validates_on_the_host():
    """The validation of dots_mesh_locate needs no device: every refusal is DOTS_ERR_ARGUMENT (ValueError), and a valid call on a
    machine without a device fails as dots_create does there."""
    vc, tc, _ = coarse("plane12")
    p = fine("plane12")[0]
    bad = [(np.array([[np.inf, 0.0, 0.0]]), vc, tc), (p, np.where(np.arange(vc.shape[0])[:, None] == 3, np.nan, vc), tc),
           (p, vc, np.concatenate([tc, [[0, 1, vc.shape[0]]]])), (p, vc, np.concatenate([tc, [[0, 1, -1]]])),
           (p, vc, np.concatenate([tc, [[0, 0, 1]]]))]
    for args in bad:
        with pytest.raises(ValueError):
            cascade.locate_device(*args)
    with pytest.raises(ValueError):
        cascade.locate_device(p, vc, tc, corner_points=np.full((p.shape[0], 3, 3), np.nan))
    import ctypes as C

    lib = _lib.load(host_only=True)
    assert lib.dots_mesh_locate(None, 0) == _lib.ERR_ARGUMENT
    desc = _lib.MeshLocateDesc(n_points=1, n_vertices=3, n_triangles=1)
    assert lib.dots_mesh_locate(C.byref(desc), 0) == _lib.ERR_ARGUMENT and b"null" in lib.dots_last_error()


@pytest.mark.parametrize("mode", ["kdtree", "exact"])
def test_mesh_transfer_modes(mode):
    v, t = fine("knot")
    vc, tc, _ = coarse("knot")
    g_c, g_f = meshes.make_geometry(vc, tc, normalize=False)[0], meshes.make_geometry(v, t, normalize=False)[0]
    tr = cascade.mesh_transfer(g_c, g_f, locate=mode)
    vs, vw, ts, cs = cascade.check_transfer(tr, n_vertices=vc.shape[0], n_triangles=tc.shape[0])
    assert vs.shape == (v.shape[0], 3) and ts.shape == (t.shape[0],)
    if mode == "kdtree":      # the default is today's behaviour
        default = cascade.mesh_transfer(g_c, g_f)
        assert all(np.array_equal(default[k], tr[k]) for k in tr)
    else:
        tri, w, d = cascade.locate_exact(v, vc, tc)
        assert np.array_equal(vs, tc[tri]) and np.array_equal(vw, w)
        assert tr["max_distance"] <= cascade.mesh_transfer(g_c, g_f)["max_distance"]      # the closest point is no further than a candidate's
    with pytest.raises(ValueError, match="locate"):
        cascade.mesh_transfer(g_c, g_f, locate="nearest")
    with pytest.raises(ValueError, match="locate"):
        meshes.link_levels([g_c, g_f], locate="nearest")


# ---- densities and levels --------------------------------------------------------------------------------------------------------
def sphere_geometry():
    if "geom" not in _cache:
        v, t = fine("icosphere")
        geom, _ = meshes.make_geometry(v, t)
        c = meshes.farthest_vertices(geom["vertices"], 0, 3)
        geom["mu0"] = meshes.bump_density(geom["vertices"], geom["area_vertices"], [c[0]], 0.5, 0.1)
        geom["mu1"] = meshes.bump_density(geom["vertices"], geom["area_vertices"], [c[1], c[2]], 0.5, 0.1)
        _cache["geom"] = geom
    return _cache["geom"]


def test_restrict_density_conserves_mass_and_signs():
    geom = sphere_geometry()
    levels = meshes.coarsen_levels(geom, 2, locate="exact")
    tr = levels[1]["transfer"]
    rng = np.random.default_rng(5)
    for mu in (geom["mu0"], geom["mu1"], rng.random(642)):
        mu_c = meshes.restrict_density(mu, tr)
        assert mu_c.shape == (160,) and np.all(mu_c >= 0.0)
        assert abs(mu_c.sum() - mu.sum()) <= 1e-14 * max(1.0, mu.sum())
    # the transpose of the vertex rule of transfer_space
    x, y = rng.random(160), rng.random(642)
    assert abs(np.dot(cascade.transfer_space(x[None], "mu", tr)[0], y) - np.dot(x, meshes.restrict_density(y, tr))) < 1e-12
    with pytest.raises(ValueError):
        meshes.restrict_density(np.ones(641), tr)


def test_coarsen_levels_are_ready_for_the_drivers():
    from dots_socp_amd.socp.solver_socp import _mesh_cascade_options, _spacetime_cascade_options

    geom = sphere_geometry()
    levels = meshes.coarsen_levels(geom, 3, locate="exact")
    assert [g["vertices"].shape[0] for g in levels] == [40, 160, 642]
    assert levels[2]["vertices"] is geom["vertices"] and "transfer" not in geom and "transfer" not in levels[0]
    for coarse_g, fine_g in zip(levels, levels[1:]):
        assert np.array_equal(coarse_g["vertices"], np.asarray(fine_g["vertices"])[coarse_g["kept"]])
        cascade.check_transfer(fine_g["transfer"], n_vertices=coarse_g["vertices"].shape[0], n_triangles=coarse_g["triangles"].shape[0])
        for k in ("mu0", "mu1"):
            assert np.all(coarse_g[k] >= 0.0) and abs(coarse_g[k].sum() - 1.0) <= 1e-14
        assert set(coarse_g["build"]) == {"coarsen_seconds", "locate_seconds", "locate"} and coarse_g["build"]["locate"] == "exact"
        for key in ("edges", "area_triangles", "area_vertices"):
            assert key in coarse_g
    _mesh_cascade_options(levels, None, {"tol": 1e-3})
    _spacetime_cascade_options(7, levels, [3, 3, 7], None, {"tol": 1e-3})
    one = meshes.coarsen_levels(geom, 1)      # (no coarser level: nothing is located, no device is needed)
    assert len(one) == 1 and one[0] is not geom and one[0]["vertices"] is geom["vertices"]
    with pytest.raises(ValueError):
        meshes.coarsen_levels(geom, 0)
    with pytest.raises(ValueError, match="locate"):
        meshes.coarsen_levels(geom, 2, locate="nearest")


def test_option_errors_before_any_device_call(monkeypatch):
    """Every option of the one-geometry driver is refused before a level is built: coarsen_levels (whose default locates on the
    device) must not be reached."""
    import importlib

    from dots_socp_amd import socp

    module = importlib.import_module("dots_socp_amd.socp.solver_socp")

    def reached(*a, **k):
        raise AssertionError("the levels were built before the options were checked")

    monkeypatch.setattr(meshes, "coarsen_levels", reached)
    monkeypatch.setattr(module, "AlmSolver", reached)
    geom = sphere_geometry()
    bad = [dict(coarse_levels=-1), dict(coarse_levels=1.5), dict(coarse_levels=True), dict(ratio=1.0), dict(ratio="4"), dict(locate="nearest"),
           dict(no_such_option=1), dict(time_slab=(0, 2)), dict(init_from=None), dict(init_transfer=None), dict(levels=[3, 3, 7]),
           dict(spacetime=True, levels=[3, 7]), dict(spacetime=True, levels=[7, 3, 7]), dict(spacetime=True, levels=[3, 3, 15]),
           dict(level_tol=-1.0), dict(nit=0), dict(lap_solver="no such solver"), dict(preconditioner="none"), dict(tol_checkpoints=[1e-9], tol=1e-3)]
    for kw in bad:
        for fn in (module.solver_socp_auto_cascade, socp.solver_raw_auto_cascade, socp.solver_auto_cascade):
            with pytest.raises(ValueError):
                fn(7, geom, **kw)
    with pytest.raises(ValueError):
        socp.solver_raw_auto_cascade(7, geom, readout="nowhere")
    assert socp.solver_raw_auto_cascade.__name__ == "dot_solver_socp_auto_cascade"
    assert socp.solver_auto_cascade.__name__ == "dot_solver_socp_auto_cascade_center"


# ---- the coarsener as a stand-alone program under the sanitizers ---------------------------------------------------------------------
MAIN = r"""
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>
#include "dots_socp_hip.h"
namespace dots { void set_error(const std::string &msg) { std::fprintf(stderr, "%s\n", msg.c_str()); } }
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *fh = std::fopen(argv[1], "r");
    if (!fh) return 2;
    int V, F, target;
    if (std::fscanf(fh, "%d %d %d", &V, &F, &target) != 3) return 2;
    std::vector<double> xyz((size_t)V * 3);
    std::vector<int32_t> tri((size_t)F * 3);
    for (double &x : xyz) if (std::fscanf(fh, "%lf", &x) != 1) return 2;
    for (int32_t &i : tri) if (std::fscanf(fh, "%d", &i) != 1) return 2;
    std::fclose(fh);
    dots_coarse_mesh *m = nullptr;
    if (dots_coarsen(V, F, xyz.data(), tri.data(), target, &m) != 0) return 1;
    std::vector<int32_t> kept((size_t)dots_coarsen_vertices(m)), out((size_t)dots_coarsen_triangles(m) * 3);
    if (dots_coarsen_copy(m, kept.data(), out.data()) != 0) return 1;
    dots_coarsen_free(m);
    std::printf("%zu %zu\n", kept.size(), out.size() / 3);
    for (int32_t k : kept) std::printf("%d\n", k);
    for (int32_t k : out) std::printf("%d\n", k);
    return 0;
}
"""


@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the stand-alone build of the coarsener"
    tmp = tmp_path_factory.mktemp("coarsen_sanitized")
    main = tmp / "main.cpp"
    main.write_text(MAIN)
    exe = tmp / "coarsen_sanitized"
    unit = os.path.join(ROOT, "dots_socp_amd", "csrc", "coarsen.hip")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-Wall",
           f"-I{ROOT}/include", "-x", "c++", unit, str(main), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.mark.parametrize("name", ["torus", "plane20"])
def test_sanitizer_run_of_the_coarsener(sanitized_program, tmp_path, name):
    """The translation unit of dots_coarsen and a small main, built with g++ -fsanitize=address,undefined, run as a process of its own
    on a mesh file: the run is clean (exit 0, nothing on stderr) and prints what the library returns."""
    v, t = fine(name)
    _, _, kept = coarse(name)
    path = tmp_path / "mesh.txt"
    with open(path, "w") as fh:
        fh.write(f"{v.shape[0]} {t.shape[0]} {v.shape[0] // 4}\n")
        fh.write("\n".join("%.17g %.17g %.17g" % tuple(row) for row in v) + "\n")
        fh.write("\n".join("%d %d %d" % tuple(row) for row in t) + "\n")
    r = subprocess.run([sanitized_program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    numbers = np.array(r.stdout.split(), dtype=np.int64)
    n_kept, n_tri = int(numbers[0]), int(numbers[1])
    assert numbers.size == 2 + n_kept + 3 * n_tri
    got_kept, got_tri = numbers[2:2 + n_kept], numbers[2 + n_kept:].reshape(n_tri, 3)
    assert np.array_equal(got_kept, kept)
    renumber = np.full(v.shape[0], -1, dtype=np.int64)
    renumber[kept] = np.arange(kept.size)
    assert np.array_equal(renumber[got_tri], coarse(name)[1])

"""GPU tests of the levels a cascade in space makes of ONE mesh: the exact location on the device (dots_mesh_locate: a grid over the
mesh, one lane per point, rings of cells) against its brute-force specification (cascade.locate_exact / corner_exact) bit for bit,
mesh_transfer(locate="device") against locate="exact", the error codes of the entry point, and the one-geometry driver and plug-ins
against the drivers they hand their levels to."""
import numpy as np
import pytest

from carry_checks import STATE, bits
from conftest import has_gpu
from dots_socp_amd import _lib, cascade, meshes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

_cache = {}


def decimated(name):
    """(fine vertices, fine triangles, coarse vertices, coarse triangles, kept) of the pairs of tests/test_coarsen_cpu.py"""
    if name not in _cache:
        v, t = {"torus": lambda: meshes.torus(64, 40), "knot": lambda: meshes.torus_knot_tube(nu=72, nv=8), "plane12": lambda: meshes.plane(12)}[name]()
        _cache[name] = (v, t) + meshes.coarsen(v, t)
    return _cache[name]


def centroids(v, t):
    return (v[t[:, 0]] + v[t[:, 1]] + v[t[:, 2]]) / 3.0


def case(name):
    """(points, vertices, triangles) of the searched mesh"""
    if name == "icosphere":      # 642 + 1 280 points, not a multiple of 64
        v, t = meshes.icosphere(3)
        return (np.concatenate([v, centroids(v, t)]),) + meshes.icosphere(1)
    if name in ("torus", "knot"):      # kept vertices among the queries: distance 0, ties among the triangles around them
        v, t, vc, tc, _ = decimated(name)
        return np.concatenate([v, centroids(v, t)]), vc, tc
    if name == "plane_outside":      # a patch three times as large, tilted out of the plane: most points lie outside the grid's box
        _, _, vc, tc, _ = decimated("plane12")
        p = meshes.plane(20)[0] * 3.0 - 1.0
        p[:, 2] = 0.3 * np.sin(5.0 * p[:, 0]) + 0.1 * p[:, 1]
        return p, vc, tc
    if name == "few_triangles":      # a few triangles that span every cell
        return (meshes.plane(20)[0],) + meshes.plane(2)
    if name == "one":
        return np.array([[0.3, 0.2, 0.5]]), np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.25]]), np.array([[0, 1, 2]])
    if name in ("workgroup", "workgroup_plus_one"):
        v, t, vc, tc, _ = decimated("torus")
        return v[:256 if name == "workgroup" else 257], vc, tc
    raise KeyError(name)


CASES = ["icosphere", "torus", "knot", "plane_outside", "few_triangles", "one", "workgroup", "workgroup_plus_one"]


@pytest.mark.parametrize("name", CASES)
def test_device_location_equals_the_specification(name):
    p, v, t = case(name)
    rng = np.random.default_rng(11)
    corner_points = p[:, None, :] + 0.2 * rng.standard_normal((p.shape[0], 3, 3))
    want_tri, want_w, want_d = cascade.locate_exact(p, v, t)
    want_corner = cascade.corner_exact(corner_points, v, t, want_tri)
    timing = {}
    tri, w, d, corner = cascade.locate_device(p, v, t, corner_points=corner_points, timing=timing)
    print(f"{name}: {p.shape[0]} points on {t.shape[0]} triangles, kernels {timing['kernel_ms']:.3f} ms")
    assert tri.dtype == np.int64 and corner.dtype == np.int32 and corner.shape == (p.shape[0], 3)
    assert np.array_equal(tri, want_tri)
    assert np.array_equal(bits(w), bits(want_w))
    assert np.array_equal(bits(d), bits(want_d))
    assert np.array_equal(corner, want_corner)
    again = cascade.locate_device(p, v, t)      # without the corner table: three arrays, the same
    assert len(again) == 3 and np.array_equal(again[0], tri) and np.array_equal(bits(again[1]), bits(w)) and np.array_equal(bits(again[2]), bits(d))
    if name in ("torus", "knot"):
        kept = decimated(name)[4]
        assert np.all(d[kept] == 0.0)
    if name == "plane_outside":
        lo, hi = v.min(axis=0), v.max(axis=0)
        assert np.any(np.any((p < lo - 0.5) | (p > hi + 0.5), axis=1))      # further out than several cells


@pytest.mark.parametrize("name", ["torus", "plane12"])
def test_mesh_transfer_on_the_device_equals_exact(name):
    v, t, vc, tc, _ = decimated(name)
    g_c, g_f = meshes.make_geometry(vc, tc, normalize=False)[0], meshes.make_geometry(v, t, normalize=False)[0]
    want = cascade.mesh_transfer(g_c, g_f, locate="exact")
    got = cascade.mesh_transfer(g_c, g_f, locate="device")
    assert set(got) == set(want)
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), k
    uniform = lambda vertices, area: (area / area.sum(), area / area.sum())      # noqa: E731
    linked = meshes.link_levels([g_c, g_f], densities=uniform, locate="device")
    assert np.array_equal(linked[1]["transfer"]["vertex_sources"], want["vertex_sources"])


def test_error_codes_leave_the_device_untouched():
    import ctypes as C

    v, t, vc, tc, _ = decimated("plane12")
    bad = [(np.array([[np.inf, 0.0, 0.0]]), vc, tc), (np.array([[np.nan, 0.0, 0.0]]), vc, tc),
           (v, np.where(np.arange(vc.shape[0])[:, None] == 3, np.nan, vc), tc),
           (v, vc, np.concatenate([tc, [[0, 1, vc.shape[0]]]])), (v, vc, np.concatenate([tc, [[0, 1, -1]]])), (v, vc, np.concatenate([tc, [[0, 0, 1]]]))]
    for args in bad:
        with pytest.raises(ValueError):
            cascade.locate_device(*args)
    with pytest.raises(ValueError):
        cascade.locate_device(v, vc, tc, corner_points=np.full((v.shape[0], 3, 3), np.inf))
    with pytest.raises(ValueError, match="device"):
        cascade.locate_device(v, vc, tc, device=4096)
    lib = _lib.load()
    assert lib.dots_mesh_locate(None, 0) == _lib.ERR_ARGUMENT
    p = np.ascontiguousarray(v)
    t32 = np.ascontiguousarray(tc, dtype=np.int32)
    out_t, out_w, out_d = np.zeros(v.shape[0], dtype=np.int32), np.zeros((v.shape[0], 3)), np.zeros(v.shape[0])
    full = dict(n_points=v.shape[0], n_vertices=vc.shape[0], n_triangles=tc.shape[0], points=p.ctypes.data_as(_lib._f64p),
                vertices=vc.ctypes.data_as(_lib._f64p), triangles=t32.ctypes.data_as(_lib._i32p), triangle=out_t.ctypes.data_as(_lib._i32p),
                weights=out_w.ctypes.data_as(_lib._f64p), distance=out_d.ctypes.data_as(_lib._f64p))
    for drop in ("points", "vertices", "triangles", "triangle", "weights", "distance"):      # NULL pointers
        desc = _lib.MeshLocateDesc(**{k: val for k, val in full.items() if k != drop})
        assert lib.dots_mesh_locate(C.byref(desc), 0) == _lib.ERR_ARGUMENT, drop
    for size in ("n_points", "n_vertices", "n_triangles"):      # sizes < 1
        desc = _lib.MeshLocateDesc(**dict(full, **{size: 0}))
        assert lib.dots_mesh_locate(C.byref(desc), 0) == _lib.ERR_ARGUMENT, size
    corner = np.zeros((v.shape[0], 3), dtype=np.int32)
    desc = _lib.MeshLocateDesc(**dict(full, corner=corner.ctypes.data_as(_lib._i32p)))      # a corner table without corner points
    assert lib.dots_mesh_locate(C.byref(desc), 0) == _lib.ERR_ARGUMENT and lib.dots_last_error()
    assert not out_t.any() and not out_w.any() and not out_d.any()      # nothing was written
    desc = _lib.MeshLocateDesc(**full)
    assert lib.dots_mesh_locate(C.byref(desc), 0) == 0      # and the device is as it was
    assert np.array_equal(out_t, cascade.locate_exact(v, vc, tc)[0])


# ---- the driver that takes one geometry ----------------------------------------------------------------------------------------------
TOL = 1e-3


def sphere_geometry():
    if "geom" not in _cache:
        geom, _ = meshes.make_geometry(*meshes.icosphere(3))
        c = meshes.farthest_vertices(geom["vertices"], 0, 3)
        geom["mu0"] = meshes.bump_density(geom["vertices"], geom["area_vertices"], [c[0]], 0.5, 0.1)
        geom["mu1"] = meshes.bump_density(geom["vertices"], geom["area_vertices"], [c[1], c[2]], 0.5, 0.1)
        _cache["geom"] = geom
        _cache["levels"] = meshes.coarsen_levels(geom, 3, locate="exact")
    return _cache["geom"], _cache["levels"]


def same_run(sol_a, hist_a, sol_b, hist_b):
    assert hist_a.kkt_errors.shape == hist_b.kkt_errors.shape
    assert np.array_equal(hist_a.kkt_errors, hist_b.kkt_errors, equal_nan=True)
    for key in ("Transportation cost", "Objective value"):
        assert np.array_equal(hist_a.history[key], hist_b.history[key], equal_nan=True), key
    for k in STATE:
        assert np.array_equal(bits(sol_a[k]), bits(sol_b[k])), (k, float(np.max(np.abs(sol_a[k] - sol_b[k]))))


def test_auto_cascade_equals_the_mesh_cascade_on_the_same_levels():
    """icosphere(3) at T = 7, tol 1e-3, two coarse levels (642 -> 160 -> 40) located on the device: every level ends below tol, and
    histories and solution are those of solver_socp_mesh_cascade on coarsen_levels(..., locate="exact") bit for bit."""
    from dots_socp_amd.socp import solver_socp_mesh_cascade
    from dots_socp_amd.socp.solver_socp import solver_socp_auto_cascade

    geom, levels = sphere_geometry()
    kw = dict(tol=TOL, nit=4000)
    sol, hist = solver_socp_auto_cascade(7, geom, coarse_levels=2, **kw)
    rec = hist.solver_stats["mesh_cascade"]["levels"]
    print("iterations", [r["iterations"] for r in rec], "kkt_max", [r["kkt_max"] for r in rec], "build", hist.solver_stats["auto_cascade"])
    assert [r["n_vertices"] for r in rec] == [40, 160, 642] and [r["transfer"] for r in rec] == [None, "located", "located"]
    for r in rec:
        assert r["kkt_max"] < TOL, r
    build = hist.solver_stats["auto_cascade"]
    assert [b["n_vertices"] for b in build["levels"]] == [40, 160] and all(b["locate"] == "device" for b in build["levels"])
    assert all(b["coarsen_seconds"] >= 0 and b["locate_seconds"] > 0 and b["max_distance"] > 0 for b in build["levels"])
    assert build["build_seconds"] >= sum(b["coarsen_seconds"] + b["locate_seconds"] for b in build["levels"])
    sol_m, hist_m = solver_socp_mesh_cascade(7, levels, **kw)
    same_run(sol, hist, sol_m, hist_m)
    assert "transfer" not in geom      # the caller's geometry is left as it was


def test_auto_cascade_in_space_and_time_and_without_levels():
    from dots_socp_amd.socp import solver_socp, solver_socp_spacetime_cascade
    from dots_socp_amd.socp.solver_socp import solver_socp_auto_cascade

    geom, levels = sphere_geometry()
    kw = dict(tol=TOL, nit=4000)
    sol, hist = solver_socp_auto_cascade(7, geom, coarse_levels=2, spacetime=True, levels=[3, 3, 7], **kw)
    sol_s, hist_s = solver_socp_spacetime_cascade(7, levels, levels=[3, 3, 7], **kw)
    same_run(sol, hist, sol_s, hist_s)
    assert [r["n_time"] for r in hist.solver_stats["spacetime_cascade"]["levels"]] == [3, 3, 7]
    sol, hist = solver_socp_auto_cascade(7, geom, coarse_levels=0, **kw)
    sol_0, hist_0 = solver_socp(7, geom, **kw)
    same_run(sol, hist, sol_0, hist_0)
    assert "auto_cascade" not in hist.solver_stats


def test_plug_in_returns_what_the_mesh_cascade_plug_in_returns():
    from dots_socp_amd.socp import solver_auto_cascade, solver_mesh_cascade

    geom, levels = sphere_geometry()
    kw = dict(tol=TOL, nit=4000)
    got, hist = solver_auto_cascade(7, geom, coarse_levels=2, **kw)
    want, hist_m = solver_mesh_cascade(7, levels, **kw)
    assert set(got) == set(want)
    for k in ("mu", "E"):
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), k
    assert got["mu"].shape == (8, 642) and np.array_equal(got["mu"][0], geom["mu0"]) and np.array_equal(got["mu"][-1], geom["mu1"])
    assert np.array_equal(hist.kkt_errors, hist_m.kkt_errors, equal_nan=True)

"""CPU tests of the cascade in space between independent triangulations of one surface: the locator (cascade.locate) against a
brute-force search, the transfer tables (mesh_transfer) against the nested case on a flat pair, the specification of the transfer
(transfer_space), the tables the device kernel reads against that specification under independent renumberings of the two meshes
(transfer_row_maps), meshes.link_levels, the header and its ctypes mirror, and the argument checks of the driver and the solver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dots_socp_amd import _lib, cascade, meshes

STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")


def rotation(az, ax):
    """Rz(az) . Rx(ax)"""
    rz = np.array([[np.cos(az), -np.sin(az), 0.0], [np.sin(az), np.cos(az), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(ax), -np.sin(ax)], [0.0, np.sin(ax), np.cos(ax)]])
    return rz @ rx


def rotated_icosphere(level, az, ax):
    v, t = meshes.icosphere(level)
    return v @ rotation(az, ax).T, t


PAIRS = {
    "plane": lambda: (meshes.plane(4), meshes.plane(7)),                                   # 25 -> 72 vertices, the fine patch is larger
    "icosphere": lambda: (meshes.icosphere(1), rotated_icosphere(2, 0.7, 0.4)),            # 42 -> 162 vertices, no shared vertex
    "torus": lambda: (meshes.torus(8, 6), meshes.torus(13, 9)),                            # 48 -> 117 vertices, no common divisor
}


def geometry(v, t):
    return {"vertices": np.asarray(v, dtype=np.float64), "triangles": np.asarray(t)}


def longest_edge(v, t):
    e = np.concatenate([v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 1]], v[t[:, 0]] - v[t[:, 2]]], axis=0)
    return float(np.linalg.norm(e, axis=1).max())


def brute_force_distance(p, v, t):
    """The distance of every point to the mesh by a search over ALL triangles"""
    n, F = p.shape[0], t.shape[0]
    f = np.tile(np.arange(F), n)
    _, d = cascade.closest_on_triangles(np.repeat(p, F, axis=0), v[t[f, 0]], v[t[f, 1]], v[t[f, 2]])
    return d.reshape(n, F).min(axis=1)


def shapes(n, V, F):
    return {"phi": (n + 1, V), "B": (n + 1, F, 3), "E": (n + 1, F, 3), "z_mid": (n, 2, 3, F, 3), "beta_mid": (n, 2, 3, F, 3),
            **{k: (n, V) for k in ("A", "lambda_c", "z_fst", "z_end", "mu", "beta_fst", "beta_end")}}


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_locator_against_a_brute_force_search(name):
    (vc, tc), (vf, tf) = PAIRS[name]()
    tri, w, d = cascade.locate(vf, vc, tc)
    assert tri.shape == (vf.shape[0],) and w.shape == (vf.shape[0], 3) and d.shape == (vf.shape[0],)
    assert tri.min() >= 0 and tri.max() < tc.shape[0]
    assert np.all(w >= 0.0)
    assert np.max(np.abs(w.sum(axis=1) - 1.0)) <= 1e-15 * 4
    # the weights describe the point at that distance
    q = np.einsum("ik,ikj->ij", w, vc[tc[tri]])
    assert np.allclose(np.linalg.norm(vf - q, axis=1), d, rtol=0, atol=1e-15)
    # no triangle of the whole mesh is closer than the one found among the candidates
    assert np.array_equal(d, brute_force_distance(vf, vc, tc))
    again = cascade.locate(vf, vc, tc)
    assert all(np.array_equal(a, b) for a, b in zip((tri, w, d), again))
    assert d.max() <= longest_edge(vc, tc)
    if name == "plane":
        inside = d <= 1e-12
        assert int(inside.sum()) == 58 and int((~inside).sum()) == 14
        # outside the coarse patch a point is clamped to its boundary: an edge or a vertex of the located triangle
        assert np.all((w[~inside] == 0.0).any(axis=1)) and np.all(d[~inside] > 1e-3)
        lin = lambda p: 2.0 * p[:, 0] - 3.0 * p[:, 1] + 0.5      # noqa: E731
        s = tc[tri]
        got = (w[:, 0] * lin(vc)[s[:, 0]] + w[:, 1] * lin(vc)[s[:, 1]]) + w[:, 2] * lin(vc)[s[:, 2]]
        assert np.max(np.abs(got - lin(vf))[inside]) <= 1e-14
    if name == "icosphere":
        assert abs(d.max() - 0.0657) < 5e-5 and abs(longest_edge(vc, tc) - 0.618) < 5e-4
        assert int((w > 1e-12).all(axis=1).sum()) == 150      # (the other twelve lie on an edge of the coarse mesh, up to rounding)
    if name == "torus":
        assert abs(d.max() - 0.132) < 5e-4 and abs(longest_edge(vc, tc) - 1.07) < 5e-3


def test_locator_checks_its_input():
    v, t = meshes.plane(4)
    flat = t.copy()
    flat[3] = [t[3, 0], t[3, 1], t[3, 0]]      # a triangle of zero area
    with pytest.raises(ValueError, match="zero area"):
        cascade.locate(v, v, flat)
    with pytest.raises(ValueError):
        cascade.locate(v[:, :2], v, t)
    with pytest.raises(ValueError):
        cascade.locate(v, v, t + v.shape[0])
    # k larger than the mesh is the whole mesh
    tri, w, d = cascade.locate(v[:5], v[[0, 1, 5]], np.array([[0, 1, 2]]), k=7)
    assert np.array_equal(tri, np.zeros(5, dtype=np.int64)) and np.all(w >= 0)


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_mesh_transfer_tables(name):
    (vc, tc), (vf, tf) = PAIRS[name]()
    tr = cascade.mesh_transfer(geometry(vc, tc), geometry(vf, tf))
    Vf, Ff = vf.shape[0], tf.shape[0]
    assert tr["vertex_sources"].dtype == np.int32 and tr["vertex_sources"].shape == (Vf, 3)
    assert tr["vertex_weights"].dtype == np.float64 and tr["vertex_weights"].shape == (Vf, 3)
    assert tr["triangle_source"].dtype == np.int32 and tr["triangle_source"].shape == (Ff,)
    assert tr["corner_source"].dtype == np.int32 and tr["corner_source"].shape == (Ff, 3)
    assert tr["n_source_vertices"] == vc.shape[0] and tr["n_source_triangles"] == tc.shape[0]
    tri, w, d = cascade.locate(vf, vc, tc)
    assert np.array_equal(tr["vertex_sources"], tc[tri]) and np.array_equal(tr["vertex_weights"], w)
    centroid = (vf[tf[:, 0]] + vf[tf[:, 1]] + vf[tf[:, 2]]) / 3.0
    tri_c, _, d_c = cascade.locate(centroid, vc, tc)
    assert np.array_equal(tr["triangle_source"], tri_c)
    assert tr["max_distance"] == max(d.max(), d_c.max()) <= longest_edge(vc, tc)
    # a corner's source is the corner of the source triangle nearest to it, in barycentric terms
    for k in range(3):
        s = tc[tr["triangle_source"]]
        wk, _ = cascade.closest_on_triangles(vf[tf[:, k]], vc[s[:, 0]], vc[s[:, 1]], vc[s[:, 2]])
        assert np.array_equal(tr["corner_source"][:, k], np.argmax(wk, axis=1))
    cascade.check_transfer(tr, n_vertices=vc.shape[0], n_triangles=tc.shape[0])
    again = cascade.mesh_transfer(geometry(vc, tc), geometry(vf, tf))
    assert all(np.array_equal(tr[k], again[k]) for k in tr)


def test_consistent_with_the_nested_case_on_a_flat_pair():
    v, t = meshes.plane(4)
    vf, tf, parents = meshes.subdivide(v, t)
    tr = cascade.mesh_transfer(geometry(v, t), geometry(vf, tf))
    assert np.array_equal(tr["triangle_source"], parents["triangle_parent"])
    for k in range(3):      # corner k of child k is corner k of the parent
        assert np.all(tr["corner_source"][k::4, k] == k)
    assert tr["max_distance"] <= 1e-15
    rng = np.random.default_rng(2)
    src = shapes(3, v.shape[0], t.shape[0])
    for name in cascade.VERTEX_ARRAYS:
        x = rng.standard_normal(src[name])
        got, want = cascade.transfer_space(x, name, tr), cascade.prolong_space(x, name, parents)
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 1e-14 * np.max(np.abs(want)), name
    for name in cascade.TRIANGLE_ARRAYS:
        x = rng.standard_normal(src[name])
        assert np.array_equal(cascade.transfer_space(x, name, tr), cascade.prolong_space(x, name, parents))


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_transfer_space_shapes_and_rules(name):
    (vc, tc), (vf, tf) = PAIRS[name]()
    tr = cascade.mesh_transfer(geometry(vc, tc), geometry(vf, tf))
    n = 3
    src, dst = shapes(n, vc.shape[0], tc.shape[0]), shapes(n, vf.shape[0], tf.shape[0])
    rng = np.random.default_rng(5)
    vs, vw, ts, cs = tr["vertex_sources"], tr["vertex_weights"], tr["triangle_source"], tr["corner_source"]
    for k in STATE:
        x = rng.standard_normal(src[k])
        out = cascade.transfer_space(x, k, tr)
        assert out.shape == dst[k] and out.dtype == np.float64, k
        if k in cascade.VERTEX_ARRAYS:
            for v in (0, vf.shape[0] // 2, vf.shape[0] - 1):
                assert np.array_equal(out[:, v], (vw[v, 0] * x[:, vs[v, 0]] + vw[v, 1] * x[:, vs[v, 1]]) + vw[v, 2] * x[:, vs[v, 2]])
            const = cascade.transfer_space(np.full(src[k], 0.3), k, tr)      # convex weights: a constant stays one
            assert np.max(np.abs(const - 0.3)) <= 2e-16
        elif k in cascade.TRIANGLE_ARRAYS:
            for f in (0, tf.shape[0] // 2, tf.shape[0] - 1):
                assert np.array_equal(out[:, f], x[:, ts[f]])
        else:
            for f in (0, tf.shape[0] // 2, tf.shape[0] - 1):
                for c in range(3):
                    assert np.array_equal(out[:, :, c, f], x[:, :, cs[f, c], ts[f]])
    sol = {k: rng.standard_normal(src[k]) for k in STATE}
    sol["checkpoints"] = None
    up = cascade.transfer_space_solution(sol, tr)
    assert set(up) == set(STATE) and all(np.array_equal(up[k], cascade.transfer_space(sol[k], k, tr)) for k in STATE)


def test_transfer_space_checks_its_input():
    (vc, tc), (vf, tf) = PAIRS["plane"]()
    tr = cascade.mesh_transfer(geometry(vc, tc), geometry(vf, tf))
    V, F = vc.shape[0], tc.shape[0]
    with pytest.raises(ValueError):
        cascade.transfer_space(np.zeros((3, V)), "rho", tr)
    with pytest.raises(ValueError):
        cascade.transfer_space(np.zeros((3, V + 1)), "mu", tr)              # a transfer of another mesh
    with pytest.raises(ValueError):
        cascade.transfer_space(np.zeros((4, F + 2, 3)), "B", tr)
    with pytest.raises(ValueError):
        cascade.transfer_space(np.zeros((3, 2, 3, F - 1, 3)), "z_mid", tr)
    with pytest.raises(ValueError):
        cascade.transfer_space(np.zeros((3, V)), "B", tr)                   # not the layout of B
    with pytest.raises(ValueError):
        cascade.transfer_space(np.zeros((3, 3, 2, F, 3)), "z_mid", tr)      # not the layout of z_mid
    with pytest.raises(ValueError):
        cascade.transfer_space(np.zeros((3, V)), "mu", {k: v for k, v in tr.items() if k != "vertex_weights"})
    bad = lambda **kw: {**tr, **kw}      # noqa: E731
    w = tr["vertex_weights"].copy()
    w[3, 1] = -1e-3
    nan = tr["vertex_weights"].copy()
    nan[0, 0] = np.nan
    corner = tr["corner_source"].copy()
    corner[2, 2] = 3
    source = tr["vertex_sources"].copy()
    source[1, 1] = V
    for wrong in (bad(vertex_weights=w), bad(vertex_weights=nan), bad(corner_source=corner), bad(vertex_sources=source),
                  bad(vertex_sources=tr["vertex_sources"].astype(np.float64)), bad(vertex_weights=tr["vertex_weights"][:, :2]),
                  bad(triangle_source=tr["triangle_source"][:-1]), bad(triangle_source=tr["triangle_source"] - 1)):
        with pytest.raises(ValueError):
            cascade.check_transfer(wrong)
    with pytest.raises(ValueError):
        cascade.check_transfer(tr, n_vertices=V + 1)
    with pytest.raises(ValueError):
        cascade.check_transfer(tr, n_triangles=F - 1)


def test_identity_transfer():
    """A mesh onto itself: every vertex has one weight 1, every triangle and corner is its own source, and all twelve arrays come back
    bit for bit."""
    v, t = meshes.icosphere(2)
    tr = cascade.mesh_transfer(geometry(v, t), geometry(v, t))
    assert np.array_equal(np.sort(tr["vertex_weights"], axis=1), np.tile([0.0, 0.0, 1.0], (v.shape[0], 1)))
    assert np.array_equal(tr["vertex_sources"][np.arange(v.shape[0]), np.argmax(tr["vertex_weights"], axis=1)], np.arange(v.shape[0]))
    assert np.array_equal(tr["triangle_source"], np.arange(t.shape[0]))
    assert np.array_equal(tr["corner_source"], np.tile(np.arange(3), (t.shape[0], 1)))
    rng = np.random.default_rng(9)
    for k, shape in shapes(3, v.shape[0], t.shape[0]).items():
        x = rng.standard_normal(shape)
        assert np.array_equal(cascade.transfer_space(x, k, tr).view(np.int64), x.view(np.int64)), k


def device_rows(x, name, perm_v, perm_f):
    """The rows of the device layout of a reference-layout array in the numbering ``perm`` (device row i = caller entity perm[i]),
    time along the last axis: vertex arrays (V, n), triangle arrays (3F, n), corner arrays (18F, n) with row ((f*3+k)*2+s)*3+c."""
    if name in cascade.VERTEX_ARRAYS:
        return np.ascontiguousarray(x[:, perm_v].T)
    if name in cascade.TRIANGLE_ARRAYS:
        return np.ascontiguousarray(x[:, perm_f, :].transpose(1, 2, 0)).reshape(-1, x.shape[0])
    return np.ascontiguousarray(x[:, :, :, perm_f, :].transpose(3, 2, 1, 4, 0)).reshape(-1, x.shape[0])      # [f][k][s][c][t]


@pytest.mark.parametrize("name", sorted(PAIRS))
@pytest.mark.parametrize("permuted", [(True, True), (True, False), (False, True), (False, False)])
def test_row_maps_against_the_specification(name, permuted):
    """What the kernel does with its tables, done in numpy on rows in device order, equals the specification in device order."""
    (vc, tc), (vf, tf) = PAIRS[name]()
    tr = cascade.mesh_transfer(geometry(vc, tc), geometry(vf, tf))
    Vc, Fc, Vf, Ff, n = vc.shape[0], tc.shape[0], vf.shape[0], tf.shape[0], 2
    rng = np.random.default_rng(17)
    pvs, pfs = (rng.permutation(Vc), rng.permutation(Fc)) if permuted[0] else (None, None)
    pvd, pfd = (rng.permutation(Vf), rng.permutation(Ff)) if permuted[1] else (None, None)
    vsrc, vw, fsrc, csrc = cascade.transfer_row_maps(tr, pvd, pfd, pvs, pfs)
    assert vsrc.dtype == np.int32 and vsrc.shape == (Vf, 3) and vw.dtype == np.float64 and vw.shape == (Vf, 3)
    assert fsrc.dtype == np.int32 and fsrc.shape == (Ff,) and csrc.dtype == np.int32 and csrc.shape == (Ff, 3)
    assert all(a.flags.c_contiguous for a in (vsrc, vw, fsrc, csrc))
    assert vsrc.min() >= 0 and vsrc.max() < Vc and fsrc.min() >= 0 and fsrc.max() < Fc and csrc.min() >= 0 and csrc.max() <= 2
    ident = lambda p, m: np.arange(m) if p is None else p      # noqa: E731
    src = shapes(n, Vc, Fc)
    for k in STATE:
        x = rng.standard_normal(src[k])
        want = device_rows(cascade.transfer_space(x, k, tr), k, ident(pvd, Vf), ident(pfd, Ff))
        rows = device_rows(x, k, ident(pvs, Vc), ident(pfs, Fc))
        if k in cascade.VERTEX_ARRAYS:
            got = (vw[:, 0:1] * rows[vsrc[:, 0]] + vw[:, 1:2] * rows[vsrc[:, 1]]) + vw[:, 2:3] * rows[vsrc[:, 2]]
        elif k in cascade.TRIANGLE_ARRAYS:
            got = rows[(fsrc[:, None] * 3 + np.arange(3)[None, :]).reshape(-1)]
        else:      # destination row ((f' * 3 + k) * 2 + s) * 3 + c  <-  source row ((fsrc * 3 + csrc[f'][k]) * 2 + s) * 3 + c
            s, c = np.arange(2)[None, None, :, None], np.arange(3)[None, None, None, :]
            got = rows[(((fsrc[:, None, None, None] * 3 + csrc[:, :, None, None]) * 2 + s) * 3 + c).reshape(-1)]
        assert got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64)), k
    with pytest.raises(ValueError):
        cascade.transfer_row_maps(tr, perm_vert_dst=np.arange(Vf - 1))
    with pytest.raises(ValueError):
        cascade.transfer_row_maps(tr, perm_tri_dst=np.arange(Ff + 1))
    with pytest.raises(ValueError):
        cascade.transfer_row_maps(tr, perm_vert_src=np.arange(Vc + 1))
    with pytest.raises(ValueError):
        cascade.transfer_row_maps(tr, perm_tri_src=np.arange(Fc - 1))


def sphere_geometries():
    """icosphere(1), the rotated icosphere(2), icosphere(3) under a second rotation, normalised together"""
    raw = [meshes.icosphere(1), rotated_icosphere(2, 0.7, 0.4), rotated_icosphere(3, -0.3, 1.1)]
    return [meshes.make_geometry((v + 1.0) * 0.5, t, normalize=False)[0] for v, t in raw]


def test_link_levels():
    geoms = sphere_geometries()
    c = meshes.farthest_vertices(geoms[0]["vertices"], 0, 3)
    centres = geoms[0]["vertices"][c]

    def bumps(v, a):
        near = lambda p: int(np.argmin(np.linalg.norm(v - p, axis=1)))      # noqa: E731
        return (meshes.bump_density(v, a, [near(centres[0])], 0.3, 0.05), meshes.bump_density(v, a, [near(centres[1]), near(centres[2])], 0.3, 0.05))

    geoms[0]["mu0"], geoms[0]["mu1"] = bumps(geoms[0]["vertices"], geoms[0]["area_vertices"])
    for densities in (None, bumps):
        levels = meshes.link_levels(geoms, densities=densities)
        assert len(levels) == 3 and "transfer" not in levels[0] and "transfer" not in geoms[1]      # (the input is left alone)
        assert [g["vertices"].shape[0] for g in levels] == [42, 162, 642]
        for coarse, fine in zip(levels, levels[1:]):
            tr = fine["transfer"]
            cascade.check_transfer(tr, n_vertices=coarse["vertices"].shape[0], n_triangles=coarse["triangles"].shape[0])
            assert tr["vertex_sources"].shape[0] == fine["vertices"].shape[0] and tr["triangle_source"].shape[0] == fine["triangles"].shape[0]
            for k in ("mu0", "mu1"):
                assert fine[k].shape == (fine["vertices"].shape[0],) and np.all(fine[k] >= 0)
                assert abs(fine[k].sum() - 1.0) <= 1e-14
        if densities is None:      # the density per unit area of the level below, carried up by the vertex rule
            rho = cascade.transfer_space((levels[0]["mu0"] / levels[0]["area_vertices"])[None, :], "mu", levels[1]["transfer"])[0]
            want = rho * levels[1]["area_vertices"]
            assert np.allclose(levels[1]["mu0"], want / want.sum(), rtol=1e-14, atol=0)
        else:
            assert np.array_equal(levels[1]["mu1"], bumps(levels[1]["vertices"], levels[1]["area_vertices"])[1])
    # a level that has its parents is left alone: a mixed hierarchy
    nested = meshes.refine_levels(geoms[0], 2, project=lambda p: 0.5 + 0.5 * (p - 0.5) / np.linalg.norm(p - 0.5, axis=1, keepdims=True))
    mixed = meshes.link_levels([nested[0], nested[1], geoms[2]])
    assert "transfer" not in mixed[1] and mixed[1]["parents"] is nested[1]["parents"] and np.array_equal(mixed[1]["mu0"], nested[1]["mu0"])
    assert mixed[2]["transfer"]["n_source_vertices"] == 162 and abs(mixed[2]["mu0"].sum() - 1.0) <= 1e-14
    # the distance guard: not the same scaling
    (vc, tc), (vf, tf) = PAIRS["icosphere"]()
    with pytest.raises(ValueError, match="same surface"):
        meshes.link_levels([dict(geoms[0], vertices=3.0 * vc), dict(geoms[1], vertices=vf)])
    assert "transfer" in meshes.link_levels([dict(geoms[0], vertices=vc), dict(geoms[1], vertices=vf)])[1]
    with pytest.raises(ValueError):
        meshes.link_levels([])
    with pytest.raises(ValueError, match="mu0"):
        meshes.link_levels([{k: v for k, v in geoms[0].items() if k not in ("mu0", "mu1")}, geoms[1]])


def test_library_exports_the_space_transfer():
    lib = _lib.load(host_only=True)
    assert "dots_transfer_space" in _lib.EXPORTS
    assert hasattr(lib, "dots_transfer_space")
    assert _lib.ABI_VERSION == 7      # an addition: the ABI version stays


def test_header_declares_the_space_transfer(tmp_path):
    text = open(os.path.join(ROOT, "include", "dots_socp_hip.h")).read()
    assert "int dots_transfer_space(dots_ctx *dst, dots_ctx *src, const dots_transfer_space_desc *desc);" in text
    fields = ("vsrc", "vw", "fsrc", "csrc", "n_vertices", "n_triangles", "factor", "ms")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dots_socp_hip.h"\n'
                   'int main(void){printf("%zu", sizeof(dots_transfer_space_desc));\n'
                   + "".join(f'printf(" %zu", offsetof(dots_transfer_space_desc, {f}));\n' for f in fields) + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = _lib.TransferSpaceDesc
    assert [name for name, _ in D._fields_] == list(fields)
    assert out == [C.sizeof(D)] + [getattr(D, f).offset for f in fields]


class _Finalised:
    """What the argument checks of AlmSolver read of ``init_from``, without a device"""
    finalized = True

    def __init__(self, n_time):
        self.n_time = n_time


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the HIP library fails the test: the refusals must come first."""
    def refuse(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", refuse)


def test_argument_errors_before_any_device_call(no_library):
    from dots_socp_amd.socp import solver_raw_mesh_cascade, solver_socp_mesh_cascade
    from dots_socp_amd.socp.solver_socp import AlmSolver

    geoms = sphere_geometries()
    for g in geoms:
        g["mu0"] = g["mu1"] = np.full(g["vertices"].shape[0], 1.0 / g["vertices"].shape[0])
    levels = meshes.link_levels(geoms)
    nested = meshes.refine_levels(geoms[0], 2)
    transfer = levels[1]["transfer"]
    for solve in (solver_socp_mesh_cascade, solver_raw_mesh_cascade):
        with pytest.raises(ValueError, match="both"):
            solve(7, [levels[0], dict(levels[1], parents=nested[1]["parents"])])
        with pytest.raises(ValueError, match="parents.*transfer"):
            solve(7, [levels[0], {k: v for k, v in levels[1].items() if k != "transfer"}])
        with pytest.raises(ValueError, match="transfer"):
            solve(7, [levels[0], levels[2]])                                      # the transfer of level 2 starts from level 1
        with pytest.raises(ValueError, match="transfer"):
            solve(7, [levels[0], dict(levels[2], transfer=transfer)])             # a transfer to another mesh
        with pytest.raises(ValueError):
            solve(7, levels, init_transfer=transfer)
    with pytest.raises(ValueError, match="init_from"):
        AlmSolver(7, levels[1], init_transfer=transfer)
    with pytest.raises(ValueError, match="time grid"):
        AlmSolver(15, levels[1], init_from=_Finalised(7), init_transfer=transfer)      # mesh and time grid in one call
    with pytest.raises(ValueError, match="exclusive"):
        AlmSolver(7, levels[1], init_from=_Finalised(7), init_transfer=transfer, init_parents=nested[1]["parents"])

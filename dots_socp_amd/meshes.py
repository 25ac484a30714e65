"""Deterministic surface-mesh and boundary-density generators.

The reference's packaged meshes are Git-LFS pointers in the mount
(e.g. ``dot_surface_socp/data/meshes/knots_5.off:1-3``), so every workload in
BASELINE.json is run on a generated stand-in of the same size class:

    icosphere(level=5)            V=10 242  F=20 480   "sphere ~10k"
    torus(400, 250)               V=100 000 F=200 000  "torus ~100k"
    torus_knot_tube(2, 5, ...)    V~4.3k    F~8.6k     knots_5 stand-in
    plane(n)                      flat hexagonal patch, analytic answer 0.04

Densities follow the reference's recipe (``data/settings/knots_5.py:15-20``,
``data/util.py:6-13``): area-weighted Gaussian bumps cut at a radius around fixed
vertices, each normalised to unit mass (``data/load_example.py:138-139``).
"""
from __future__ import annotations

import numpy as np


# --------------------------------------------------------------------------- #
# meshes
# --------------------------------------------------------------------------- #
def _unique_edges(triangles):
    t = np.asarray(triangles)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=0)
    e.sort(axis=1)
    return np.unique(e, axis=0)


def icosphere(level: int = 3, radius: float = 1.0):
    """Subdivided icosahedron projected on the sphere: V = 10*4^level + 2."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array(
        [[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g],
         [0, -1, -g], [0, 1, -g], [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]],
        dtype=np.float64,
    )
    f = np.array(
        [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
         [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5],
         [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]],
        dtype=np.int64,
    )
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(level):
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)
        e.sort(axis=1)
        ue, inv = np.unique(e, axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        mid = v[ue[:, 0]] + v[ue[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        base = v.shape[0]
        v = np.concatenate([v, mid], axis=0)
        nf = f.shape[0]
        m01, m12, m20 = base + inv[:nf], base + inv[nf:2 * nf], base + inv[2 * nf:]
        f = np.concatenate(
            [
                np.stack([f[:, 0], m01, m20], axis=1),
                np.stack([f[:, 1], m12, m01], axis=1),
                np.stack([f[:, 2], m20, m12], axis=1),
                np.stack([m01, m12, m20], axis=1),
            ],
            axis=0,
        )
    return radius * v, f


def _periodic_grid_triangles(nu: int, nv: int):
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    i1, j1 = (i + 1) % nu, (j + 1) % nv
    a, b, c, d = i * nv + j, i1 * nv + j, i1 * nv + j1, i * nv + j1
    return np.concatenate(
        [np.stack([a, b, c], axis=-1).reshape(-1, 3), np.stack([a, c, d], axis=-1).reshape(-1, 3)], axis=0
    ).astype(np.int64)


def torus(nu: int = 64, nv: int = 40, R: float = 1.0, r: float = 0.4):
    """Torus of major radius R, minor radius r on an nu x nv periodic grid: V = nu*nv, F = 2V."""
    u = 2 * np.pi * np.arange(nu) / nu
    w = 2 * np.pi * np.arange(nv) / nv
    uu, ww = np.meshgrid(u, w, indexing="ij")
    x = (R + r * np.cos(ww)) * np.cos(uu)
    y = (R + r * np.cos(ww)) * np.sin(uu)
    z = r * np.sin(ww)
    return np.stack([x, y, z], axis=-1).reshape(-1, 3), _periodic_grid_triangles(nu, nv)


def torus_knot_tube(p: int = 2, q: int = 5, nu: int = 216, nv: int = 20, R: float = 1.0, r: float = 0.45,
                    tube: float = 0.12):
    """Tube of radius ``tube`` around the (p, q) torus knot: stand-in for the reference's knots_5."""
    s = 2 * np.pi * np.arange(nu) / nu

    def curve(s):
        rad = R + r * np.cos(q * s)
        return np.stack([rad * np.cos(p * s), rad * np.sin(p * s), r * np.sin(q * s)], axis=-1)

    c = curve(s)
    ds = 1e-4
    tan = curve(s + ds) - curve(s - ds)
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    # a smooth periodic frame: normal = component of the radial direction orthogonal to the tangent
    radial = c.copy()
    radial[:, 2] = 0.0
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    n1 = radial - np.sum(radial * tan, axis=1, keepdims=True) * tan
    n1 /= np.linalg.norm(n1, axis=1, keepdims=True)
    n2 = np.cross(tan, n1)
    w = 2 * np.pi * np.arange(nv) / nv
    v = c[:, None, :] + tube * (np.cos(w)[None, :, None] * n1[:, None, :] + np.sin(w)[None, :, None] * n2[:, None, :])
    return v.reshape(-1, 3), _periodic_grid_triangles(nu, nv)


def plane(n: int = 20):
    """Flat patch of [0,1]^2 tiled by equilateral triangles of side 1/n (rows offset by half a side).

    Same family as the reference's procedural mesh (``data/meshes/plane.py:3-69``): n+1 vertices
    per row, rows spaced sqrt(3)/(2n) apart.  Written independently; vertex numbering is row-major.
    """
    dx = 1.0 / n
    dy = dx * np.sqrt(3.0) / 2.0
    rows = int(1.0 / dy) + 1
    cols = n + 1
    jj, ii = np.meshgrid(np.arange(cols), np.arange(rows))
    x = jj * dx + np.where(ii % 2 == 1, dx / 2.0, 0.0)
    y = ii * dy
    verts = np.stack([x, y, np.zeros_like(x)], axis=-1).reshape(-1, 3)
    idx = lambda i, j: i * cols + j  # noqa: E731
    tris = []
    for i in range(rows - 1):
        for j in range(cols - 1):
            if i % 2 == 0:
                tris.append([idx(i, j), idx(i, j + 1), idx(i + 1, j)])
                tris.append([idx(i, j + 1), idx(i + 1, j + 1), idx(i + 1, j)])
            else:
                tris.append([idx(i, j), idx(i + 1, j + 1), idx(i + 1, j)])
                tris.append([idx(i, j), idx(i, j + 1), idx(i + 1, j + 1)])
    return verts, np.asarray(tris, dtype=np.int64)


# --------------------------------------------------------------------------- #
# nested refinement (the levels of a cascade in space, cascade.prolong_space)
# --------------------------------------------------------------------------- #
def subdivide(vertices, triangles, project=None):
    """One 1 -> 4 midpoint subdivision: ``(vertices_f, triangles_f, parents)``.

    The coarse vertices keep their indices ``0 .. Vc - 1``; the edge midpoints follow in the order of ``_unique_edges``.  ``project``
    (optional) is applied to the new vertices only, e.g. to put them back on a sphere or torus.  A parent ``(a, b, c)`` with the
    midpoints ``ab, bc, ca`` has the children ``4f + 0 = (a, ab, ca)``, ``4f + 1 = (ab, b, bc)``, ``4f + 2 = (ca, bc, c)``,
    ``4f + 3 = (ab, bc, ca)``: corner k of child k is corner k of the parent.  ``parents`` = {"vertex_parents": (Vf, 2) int32 -- both
    entries of a kept vertex are the vertex itself, those of a midpoint the ends of its edge --, "triangle_parent": (Ff,) int32, here
    ``f' // 4`` (stored, so that a hierarchy need not be 1 -> 4)}."""
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles).astype(np.int64)
    Vc, Fc = v.shape[0], t.shape[0]
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=0)
    e.sort(axis=1)
    ue, inv = np.unique(e, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    mid = (v[ue[:, 0]] + v[ue[:, 1]]) * 0.5
    if project is not None:
        mid = np.asarray(project(mid), dtype=np.float64)
        if mid.shape != (ue.shape[0], 3):
            raise ValueError("subdivide: project must return one point per new vertex")
    ab, bc, ca = Vc + inv[:Fc], Vc + inv[Fc:2 * Fc], Vc + inv[2 * Fc:]
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    children = np.stack([np.stack([a, ab, ca], axis=1), np.stack([ab, b, bc], axis=1), np.stack([ca, bc, c], axis=1),
                         np.stack([ab, bc, ca], axis=1)], axis=1)      # [f][child][corner]
    kept = np.arange(Vc, dtype=np.int64)
    parents = {"vertex_parents": np.ascontiguousarray(np.concatenate([np.stack([kept, kept], axis=1), ue], axis=0), dtype=np.int32),
               "triangle_parent": np.ascontiguousarray(np.arange(4 * Fc) // 4, dtype=np.int32)}
    return np.concatenate([v, mid], axis=0), children.reshape(-1, 3), parents


def snap_projection(points):
    """A ``project`` for ``subdivide`` that moves every new vertex to the nearest of ``points`` (the vertices of the surface at the
    finer resolution, e.g. ``torus(2 * nu, 2 * nv)[0]`` above ``torus(nu, nv)``): the refined mesh then lies on the generator's own
    grid.  Two new vertices that take the same point raise ``ValueError``."""
    from scipy.spatial import cKDTree

    pts = np.asarray(points, dtype=np.float64)
    tree = cKDTree(pts)

    def project(mid):
        idx = tree.query(mid)[1]
        if np.unique(idx).size != idx.size:
            raise ValueError("snap_projection: two new vertices snap to the same point")
        return pts[idx]

    return project


def refine_levels(geometry, n_levels, project=None, densities=None):
    """``n_levels`` geometries from coarse to fine: ``geometry`` itself, then ``n_levels - 1`` subdivisions (``subdivide``), every
    refined level with its ``parents`` (the map to the level below) under the key "parents".

    ``project``: None, one callable for every step, or a list of one callable (or None) per step.  ``densities(vertices,
    area_vertices) -> (mu0, mu1)`` gives a refined level its end points; without it the densities per unit area (``mu / area_vertices``)
    of the level below are carried up by the vertex rule of ``cascade.prolong_space`` (copy at a kept vertex, half-sum of the two
    parents at a midpoint) and weighted with the level's own ``area_vertices``.  Either way ``mu0`` / ``mu1`` are scaled to unit mass.
    The coordinates are taken as they are (``make_geometry(..., normalize=False)``): a kept vertex is the same point on every level,
    so normalise the coarsest geometry, not the levels."""
    n_levels = int(n_levels)
    if n_levels < 1:
        raise ValueError("refine_levels: at least one level")
    steps = list(project) if isinstance(project, (list, tuple)) else [project] * (n_levels - 1)
    if len(steps) != n_levels - 1:
        raise ValueError("refine_levels: one projection per refinement step")
    levels = [geometry]
    for proj in steps:
        g = levels[-1]
        v, t, parents = subdivide(g["vertices"], g["triangles"], proj)
        fine, _ = make_geometry(v, t, normalize=False)
        if densities is not None:
            mu0, mu1 = densities(fine["vertices"], fine["area_vertices"])
        else:
            area_c = g["area_vertices"] if "area_vertices" in g else vertex_areas(
                np.asarray(g["vertices"]).shape[0], g["triangles"], triangle_areas(g["vertices"], g["triangles"]))
            p0, p1 = parents["vertex_parents"][:, 0], parents["vertex_parents"][:, 1]
            rho0, rho1 = np.asarray(g["mu0"], dtype=np.float64) / area_c, np.asarray(g["mu1"], dtype=np.float64) / area_c
            mu0 = np.where(p0 == p1, rho0[p0], (rho0[p0] + rho0[p1]) * 0.5) * fine["area_vertices"]
            mu1 = np.where(p0 == p1, rho1[p0], (rho1[p0] + rho1[p1]) * 0.5) * fine["area_vertices"]
        mu0, mu1 = np.asarray(mu0, dtype=np.float64), np.asarray(mu1, dtype=np.float64)
        fine["mu0"], fine["mu1"] = mu0 / mu0.sum(), mu1 / mu1.sum()
        fine["parents"] = parents
        levels.append(fine)
    return levels


def link_levels(geometries, densities=None, locate="kdtree"):
    """The counterpart of ``refine_levels`` for meshes that already exist: ``geometries`` (coarse to fine) are independent
    triangulations of one surface in the same coordinates (normalised together); every level after the first gets the map to the level
    below under the key "transfer" (``cascade.mesh_transfer``).  A level that already has "parents" is left as it is, so nested and
    located levels may be mixed.  The levels are returned as new dicts; the arrays are shared with the input.

    ``mu0`` / ``mu1`` of a level that lacks them: ``densities(vertices, area_vertices) -> (mu0, mu1)``, or without it the densities per
    unit area of the level below carried up by the vertex rule of ``cascade.transfer_space`` (of ``cascade.prolong_space`` on a level
    with "parents") and weighted with the level's own ``area_vertices``; either way scaled to unit mass.  ``locate``: how
    ``cascade.mesh_transfer`` locates ("kdtree" | "exact" | "device")."""
    from . import cascade

    levels = [dict(g) for g in geometries]
    if not levels:
        raise ValueError("link_levels: at least one geometry")

    def areas(g):
        if "area_vertices" not in g:
            g["area_triangles"] = triangle_areas(g["vertices"], g["triangles"])
            g["area_vertices"] = vertex_areas(np.asarray(g["vertices"]).shape[0], g["triangles"], g["area_triangles"])
        return np.asarray(g["area_vertices"], dtype=np.float64)

    for coarse, fine in zip(levels, levels[1:]):
        if fine.get("parents") is None:
            fine["transfer"] = cascade.mesh_transfer(coarse, fine, locate=locate)
        if fine.get("mu0") is not None and fine.get("mu1") is not None:
            continue
        area_f = areas(fine)
        if densities is not None:
            mu0, mu1 = densities(np.asarray(fine["vertices"], dtype=np.float64), area_f)
        else:
            if coarse.get("mu0") is None or coarse.get("mu1") is None:
                raise ValueError("link_levels: the level below has no mu0 / mu1 to carry up")
            area_c = areas(coarse)
            if fine.get("parents") is not None:
                up = lambda rho: cascade.prolong_space(rho[None, :], "mu", fine["parents"])[0]      # noqa: E731
            else:
                up = lambda rho: cascade.transfer_space(rho[None, :], "mu", fine["transfer"])[0]      # noqa: E731
            mu0 = up(np.asarray(coarse["mu0"], dtype=np.float64) / area_c) * area_f
            mu1 = up(np.asarray(coarse["mu1"], dtype=np.float64) / area_c) * area_f
        mu0, mu1 = np.asarray(mu0, dtype=np.float64), np.asarray(mu1, dtype=np.float64)
        fine["mu0"], fine["mu1"] = mu0 / mu0.sum(), mu1 / mu1.sum()
    return levels


# --------------------------------------------------------------------------- #
# coarsening (the levels of a cascade in space from ONE mesh)
# --------------------------------------------------------------------------- #
COS_BOUNDARY_TURN = 0.7071067811865476      # cos(pi / 4): the most a boundary may turn at a vertex that is removed
MIN_NORMAL_COSINE = 0.2                     # a triangle that survives a collapse keeps its normal to this cosine


def _coarsen_arguments(vertices, triangles, n_vertices, ratio):
    v = np.ascontiguousarray(vertices, dtype=np.float64)
    t = np.asarray(triangles)
    if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1 or t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise ValueError("coarsen: vertices (V, 3) and triangles (F, 3) expected")
    if not np.issubdtype(t.dtype, np.integer):
        raise ValueError("coarsen: integer triangles expected")
    if n_vertices is None:
        if not ratio > 1:
            raise ValueError(f"coarsen: ratio must be > 1 (got {ratio})")
        target = int(np.floor(v.shape[0] / float(ratio)))
    else:
        target = int(n_vertices)
        if target != n_vertices or target < 1:
            raise ValueError("coarsen: n_vertices must be a positive integer")
    return v, np.ascontiguousarray(t, dtype=np.int64), target


def _check_coarsen_mesh(v, t):
    """The refusals of ``coarsen`` (the native version makes the same ones in the same order)."""
    if t.min() < 0 or t.max() >= v.shape[0]:
        raise ValueError("coarsen: triangle index out of range")
    if not np.all(np.isfinite(v)):
        raise ValueError("coarsen: non-finite coordinates")
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    if not np.all(np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) > 0.0):
        raise ValueError("coarsen: a triangle of zero area")
    directed = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=0)
    if np.unique(np.sort(directed, axis=1), axis=0, return_counts=True)[1].max() > 2:
        raise ValueError("coarsen: an edge with more than two triangles")
    if np.unique(directed, axis=0).shape[0] != directed.shape[0]:
        raise ValueError("coarsen: two triangles cross an edge in the same direction")


def _coarsen_python(v, t, target):
    """The specification of ``coarsen`` in plain Python (the rules are in its docstring): ``(kept, triangles_c)``."""
    import heapq
    from math import sqrt

    P, T = v.tolist(), t.tolist()
    V = len(P)
    inc = [[] for _ in range(V)]      # the live triangles around every vertex
    for f, tri in enumerate(T):
        for w in tri:
            inc[w].append(f)
    alive_v, alive_t = [True] * V, [True] * len(T)

    def sub(a, b):
        return (a[0] - b[0], a[1] - b[1], a[2] - b[2])

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def norm(a):
        return sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])

    def normal(p0, p1, p2):
        e1, e2 = sub(P[p1], P[p0]), sub(P[p2], P[p0])
        return (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])

    def key(a, b):
        a, b = (a, b) if a < b else (b, a)
        return (norm(sub(P[a], P[b])), a, b)

    def neighbours(x):
        return {w for f in inc[x] for w in T[f] if w != x}

    def allowed(u, v_):
        edge_t = [f for f in inc[v_] if u in T[f]]
        if not 1 <= len(edge_t) <= 2:
            return False
        nu, nv = neighbours(u), neighbours(v_)
        if (nu & nv) != {w for f in edge_t for w in T[f] if w != u and w != v_}:
            return False
        count = {}
        for f in inc[v_]:
            for w in T[f]:
                if w != v_:
                    count[w] = count.get(w, 0) + 1
        boundary = sorted(w for w, k in count.items() if k == 1)
        if boundary:
            if len(edge_t) != 1 or len(boundary) != 2:
                return False
            a, b = sub(P[v_], P[boundary[0]]), sub(P[boundary[1]], P[v_])
            if not dot(a, b) >= (COS_BOUNDARY_TURN * norm(a)) * norm(b):
                return False
        elif len((nu | nv) - {u, v_}) < 3:
            return False
        for f in inc[v_]:
            if f in edge_t:
                continue
            p = T[f]
            q = [u if w == v_ else w for w in p]
            n_old, n_new = normal(*p), normal(*q)
            length = norm(n_new)
            if not length > 0.0 or not dot(n_old, n_new) >= (MIN_NORMAL_COSINE * norm(n_old)) * length:
                return False
        return True

    def collapse(u, v_):
        for f in list(inc[v_]):
            if u in T[f]:
                alive_t[f] = False
                for w in T[f]:
                    inc[w].remove(f)
        for f in inc[v_]:
            T[f] = [u if w == v_ else w for w in T[f]]
            inc[u].append(f)
        inc[v_] = []
        alive_v[v_] = False

    def all_edges():
        return [key(a, b) for a in range(V) if alive_v[a] for b in neighbours(a) if a < b]

    heap = all_edges()
    heapq.heapify(heap)
    live, collapsed = V, False
    while live > target:
        if not heap:
            if not collapsed:
                break      # a whole refill without a collapse: what was reached is the result
            heap = all_edges()
            heapq.heapify(heap)
            collapsed = False
            continue
        _, a, b = heapq.heappop(heap)
        if not (alive_v[a] and alive_v[b]) or not any(b in T[f] for f in inc[a]):
            continue
        for u, v_ in ((a, b), (b, a)):
            if allowed(u, v_):
                collapse(u, v_)
                live -= 1
                collapsed = True
                for w in neighbours(u):
                    heapq.heappush(heap, key(u, w))
                break
    kept = np.flatnonzero(np.asarray(alive_v))
    return kept, np.asarray([T[f] for f in range(len(T)) if alive_t[f]], dtype=np.int64).reshape(-1, 3)


def _coarsen_native(v, t, target):
    import ctypes as C

    from . import _lib

    lib = _lib.load(host_only=True)
    if t.max() >= 2 ** 31 or t.min() < -2 ** 31:
        raise ValueError("coarsen: triangle index out of range")
    t32 = np.ascontiguousarray(t, dtype=np.int32)
    handle = C.c_void_p()
    rc = lib.dots_coarsen(v.shape[0], t32.shape[0], v.ctypes.data_as(_lib._f64p), t32.ctypes.data_as(_lib._i32p), target, C.byref(handle))
    if rc == _lib.ERR_ARGUMENT:
        raise ValueError("coarsen: " + lib.dots_last_error().decode("utf-8", "replace").split(": ", 1)[-1])
    _lib.check(rc, "dots_coarsen")
    try:
        kept = np.empty(lib.dots_coarsen_vertices(handle), dtype=np.int32)
        tri = np.empty((lib.dots_coarsen_triangles(handle), 3), dtype=np.int32)
        _lib.check(lib.dots_coarsen_copy(handle, kept.ctypes.data_as(_lib._i32p), tri.ctypes.data_as(_lib._i32p)), "dots_coarsen_copy")
    finally:
        lib.dots_coarsen_free(handle)
    return kept.astype(np.int64), tri.astype(np.int64)


def coarsen(vertices, triangles, n_vertices=None, ratio=4.0, backend="native"):
    """Half-edge-collapse decimation: ``(vertices_c, triangles_c, kept)``.  The coarse vertices are a subset of the fine ones and no
    position moves: ``kept`` (ascending fine indices) with ``vertices_c == vertices[kept]`` bit for bit; ``triangles_c`` are the
    surviving fine triangles in fine order and corner order, with the substituted, renumbered vertices.

    ``backend="python"`` is the specification, ``"native"`` (``dots_coarsen``, host C++ of the library) returns identical arrays.
    The rules are chosen so that nothing depends on an implementation's data structures:

    * candidates: a multiset of undirected edges keyed ``(length, a, b)``, ``a < b``, ``length = sqrt((dx*dx + dy*dy) + dz*dz)``;
      every edge once at the start; always the smallest key is popped, and skipped when an end point is dead or the two are no
      longer adjacent;
    * removing ``b`` (keeping ``a``) is tried first, then removing ``a``; if neither is allowed the entry is dropped;
    * removing ``v``, keeping ``u``, is allowed if (1) the edge has one or two triangles, (2) the common neighbours of ``u`` and ``v``
      are exactly the vertices opposite the edge in those triangles (the link condition), (3) for a boundary ``v``: the edge is a
      boundary edge, ``v`` has exactly two boundary neighbours ``prev < next`` and ``dot(v - prev, next - v) >= (cos(pi/4) |v - prev|)
      |next - v|``, (4) for an interior ``v``: ``u`` keeps at least three neighbours, (5) every other triangle around ``v``, with ``v``
      replaced by ``u``, has a non-zero normal ``n'`` with ``n . n' >= (0.2 |n|) |n'|`` against its old normal ``n`` (normals are
      ``cross(p1 - p0, p2 - p0)``, every dot product ``(x0*y0 + x1*y1) + x2*y2``);
    * after a collapse every edge now around ``u`` is inserted again (duplicates are harmless);
    * it stops when the live vertex count is <= the target: ``n_vertices``, else ``floor(V / ratio)``; when the candidates run out
      first they are refilled with every current edge; a whole refill without a collapse returns what was reached (the caller sees
      the count).

    ``ValueError`` before any work: an edge with more than two triangles, two triangles crossing an edge in the same direction, a
    zero-area triangle, an index out of range, non-finite coordinates, ``ratio <= 1``."""
    if backend not in ("native", "python"):
        raise ValueError("coarsen: backend must be 'native' or 'python'")
    v, t, target = _coarsen_arguments(vertices, triangles, n_vertices, ratio)
    if backend == "python":
        _check_coarsen_mesh(v, t)
        kept, tri = _coarsen_python(v, t, target)
    else:
        kept, tri = _coarsen_native(v, t, target)
    renumber = np.full(v.shape[0], -1, dtype=np.int64)
    renumber[kept] = np.arange(kept.size)
    return v[kept], renumber[tri], kept


def restrict_density(mu_fine, transfer):
    """A density (mass per vertex) of the destination mesh of ``transfer`` (``cascade.mesh_transfer``) on its source mesh:
    ``mu_c[s] += w * mu_f[v]`` over ``vertex_sources`` / ``vertex_weights`` (``np.add.at`` in row order), the transpose of the vertex
    rule of ``cascade.transfer_space``.  The clamped weights of a vertex sum to 1 and are >= 0: mass and signs are kept."""
    from . import cascade

    vs, vw, _, _ = cascade.check_transfer(transfer)
    mu = np.asarray(mu_fine, dtype=np.float64)
    if mu.shape != (vs.shape[0],):
        raise ValueError(f"restrict_density: expected {vs.shape[0]} values (one per vertex of the transfer's destination), got shape {mu.shape}")
    out = np.zeros(int(transfer["n_source_vertices"]))
    np.add.at(out, vs, vw * mu[:, None])
    return out


def coarsen_levels(geometry, n_levels=3, ratio=4.0, locate="device", device=0):
    """``n_levels`` geometries from coarse to fine out of ONE: the finest is ``dict(geometry)``, every coarser level is
    ``make_geometry(..., normalize=False)`` of ``coarsen(level above, ratio=ratio)`` with "kept" (its vertices as indices of the level
    above), ``mu0`` / ``mu1`` restricted from the level above (``restrict_density``) and scaled to unit mass, and "build" =
    {"coarsen_seconds", "locate_seconds", "locate"}.  Every level but the coarsest carries "transfer" (``cascade.mesh_transfer`` with
    ``locate``, "device" | "exact" | "kdtree"; ``device``: the GPU of "device"), so the list is ready for
    ``solver_socp_mesh_cascade`` / ``solver_socp_spacetime_cascade``.

    ``ValueError`` when a level does not reach half the vertices of the one above (the mesh does not coarsen: too small, or all
    boundary and creases), and where ``cascade.mesh_transfer`` raises."""
    import time

    from . import cascade

    n_levels = int(n_levels)
    if n_levels < 1:
        raise ValueError("coarsen_levels: at least one level")
    cascade.check_locate(locate, "coarsen_levels")
    levels = [dict(geometry)]
    for _ in range(n_levels - 1):
        fine = levels[0]
        t0 = time.perf_counter()
        v, t, kept = coarsen(fine["vertices"], fine["triangles"], ratio=ratio)
        t1 = time.perf_counter()
        n_fine = np.asarray(fine["vertices"]).shape[0]
        if 2 * v.shape[0] > n_fine:
            raise ValueError(f"coarsen_levels: the mesh of {n_fine} vertices coarsens to {v.shape[0]} only, not to half: too few levels "
                             "can be made of it")
        coarse, _ = make_geometry(v, t, normalize=False)
        coarse["kept"] = kept
        t2 = time.perf_counter()
        fine["transfer"] = cascade.mesh_transfer(coarse, fine, locate=locate, device=device)
        t3 = time.perf_counter()
        for k in ("mu0", "mu1"):
            if fine.get(k) is not None:
                mu = restrict_density(fine[k], fine["transfer"])
                coarse[k] = mu / mu.sum()
        coarse["build"] = {"coarsen_seconds": t1 - t0, "locate_seconds": t3 - t2, "locate": locate}
        levels.insert(0, coarse)
    return levels


# --------------------------------------------------------------------------- #
# geometry dict (GeometryData of the reference, utils/type.py:6-13)
# --------------------------------------------------------------------------- #
def triangle_areas(vertices, triangles):
    v, t = np.asarray(vertices, dtype=np.float64), np.asarray(triangles)
    return 0.5 * np.linalg.norm(np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 1]]), axis=1)


def vertex_areas(n_vertices, triangles, area_triangles):
    """Sum of incident triangle areas (the reference's un-divided ``area_vertices``,
    ``surface_pre_computations_socp.py:123``)."""
    t = np.asarray(triangles)
    out = np.zeros(n_vertices)
    for k in range(3):
        np.add.at(out, t[:, k], area_triangles)
    return out


def bump_density(vertices, area_vertices, centers, radius=0.5, sigma=0.5):
    """Sum of area-weighted truncated Gaussians around ``vertices[c]`` for c in centers, mass 1."""
    v = np.asarray(vertices, dtype=np.float64)
    mu = np.zeros(v.shape[0])
    for c in centers:
        d = np.linalg.norm(v - v[c], axis=1)
        mu += area_vertices * np.where(d < radius, np.exp(-d ** 2 / sigma), 0.0)
    return mu / mu.sum()


def gaussian_density(vertices, area_vertices, center, scale):
    """Un-truncated area-weighted Gaussian exp(-|x-c|^2/scale), mass 1 (``data/settings/plane.py:14-25``)."""
    d2 = np.sum((np.asarray(vertices, dtype=np.float64) - np.asarray(center)[None, :]) ** 2, axis=1)
    mu = area_vertices * np.exp(-d2 / scale)
    return mu / mu.sum()


def make_geometry(vertices, triangles, mu0=None, mu1=None, normalize=True):
    """Build the geometry dict the solver receives; optionally normalised into the unit box.

    Normalisation restates ``socp/data_preprocessing.py:5-37``: translate and scale so the
    bounding box is [0, s]^3 with longest side 1 (the trimesh centroid shift cancels in the
    final min-subtraction).  Returns ``(geometry, scale_factor)``.
    """
    v = np.asarray(vertices, dtype=np.float64).copy()
    t = np.asarray(triangles, dtype=np.int64)
    scale = 1.0
    if normalize:
        scale = 1.0 / (v.max(axis=0) - v.min(axis=0)).max()
        v = (v - v.min(axis=0)) * scale
    area_t = triangle_areas(v, t)
    area_v = vertex_areas(v.shape[0], t, area_t)
    geom = {
        "vertices": v,
        "triangles": t,
        "edges": _unique_edges(t),
        "area_triangles": area_t,
        "area_vertices": area_v,
    }
    if mu0 is not None:
        geom["mu0"] = np.asarray(mu0, dtype=np.float64)
        geom["mu1"] = np.asarray(mu1, dtype=np.float64)
    return geom, scale


def farthest_vertices(vertices, start: int, count: int):
    """Greedy farthest-point vertex indices (deterministic centres for the bumps)."""
    v = np.asarray(vertices, dtype=np.float64)
    picked = [int(start)]
    dist = np.linalg.norm(v - v[start], axis=1)
    for _ in range(count - 1):
        nxt = int(np.argmax(dist))
        picked.append(nxt)
        dist = np.minimum(dist, np.linalg.norm(v - v[nxt], axis=1))
    return picked


def example(name: str, **kw):
    """Named synthetic workloads (stand-ins for BASELINE.json's configs).

    Returns ``(geometry, scale_factor)`` with mu0 (one bump) and mu1 (two bumps) set, normalised.
    """
    if name == "plane":
        n = kw.get("n", 20)
        v, t = plane(n)
        at = triangle_areas(v, t)
        av = vertex_areas(v.shape[0], t, at)
        mu0 = gaussian_density(v, av, [0.4, 0.4, 0.0], 2 * 0.1 ** 2)   # data/settings/plane.py:5-11
        mu1 = gaussian_density(v, av, [0.6, 0.6, 0.0], 2 * 0.1 ** 2)
        return make_geometry(v, t, mu0, mu1, normalize=kw.get("normalize", True))
    if name == "sphere":
        v, t = icosphere(kw.get("level", 5))
    elif name == "torus":
        v, t = torus(kw.get("nu", 400), kw.get("nv", 250))
    elif name == "knot":
        v, t = torus_knot_tube(2, 5, kw.get("nu", 216), kw.get("nv", 20))
    else:
        raise ValueError(f"unknown example {name!r}")
    geom, scale = make_geometry(v, t)
    c = farthest_vertices(geom["vertices"], 0, 3)
    radius, sigma = kw.get("radius", 0.35), kw.get("sigma", 0.05)
    # recipe of data/settings/knots_5.py:15-20 on the normalised mesh (radius/sigma sized for the unit box)
    geom["mu0"] = bump_density(geom["vertices"], geom["area_vertices"], [c[0]], radius, sigma)
    geom["mu1"] = bump_density(geom["vertices"], geom["area_vertices"], [c[1], c[2]], radius, sigma)
    return geom, scale


def read_off(path):
    """Triangle mesh from an OFF file: ``(vertices (V,3) float64, triangles (F,3) int64, edges (3F,2) int64)``.

    Same contract as the reference's reader (``data/util.py:73-144``): first line ``OFF``, then the vertex and face
    counts, then V coordinate lines and F lines ``3 i j k``; empty lines are skipped; edges are the three directed
    sides of every triangle in file order; a malformed file raises ``ValueError``.  Written independently: the
    payload is parsed with numpy in two blocks instead of line by line (a 100k-vertex mesh reads in ~0.1 s)."""
    try:
        with open(path, "r") as fh:
            lines = [ln.split() for ln in fh]
    except OSError as exc:
        raise ValueError(f"Error reading .off file: {exc}") from exc
    lines = [ln for ln in lines if ln]
    if not lines or lines[0] != ["OFF"]:
        raise ValueError("Error reading .off file: Not a valid .off file")
    if len(lines) < 2 or len(lines[1]) < 2:
        raise ValueError("Error reading .off file: Invalid file format: missing vertex/triangle counts")
    try:
        nv, nf = int(lines[1][0]), int(lines[1][1])
        body = lines[2:]
        faces = [ln for ln in body if ln[0] == "3"]
        verts = [ln for ln in body if ln[0] != "3"]
        if len(verts) != nv:
            raise ValueError(f"Expected {nv} vertices but found {len(verts)}")
        if len(faces) != nf:
            raise ValueError(f"Expected {nf} triangles but found {len(faces)}")
        if any(len(ln) < 3 for ln in verts) or any(len(ln) < 4 for ln in faces):
            raise ValueError("Invalid vertex / triangle data")
        vertices = np.array([ln[:3] for ln in verts], dtype=np.float64).reshape(nv, 3)
        triangles = np.array([ln[1:4] for ln in faces], dtype=np.int64).reshape(nf, 3)
    except ValueError as exc:
        raise ValueError(f"Error reading .off file: {exc}") from exc
    edges = np.stack([triangles[:, [0, 1]], triangles[:, [1, 2]], triangles[:, [2, 0]]], axis=1).reshape(-1, 2)
    return vertices, triangles, edges


def write_off(path, vertices, triangles):
    """Write a triangle mesh as OFF (the inverse of ``read_off``; 17 significant digits)."""
    v, t = np.asarray(vertices, dtype=np.float64), np.asarray(triangles)
    with open(path, "w") as fh:
        fh.write("OFF\n%d %d 0\n" % (v.shape[0], t.shape[0]))
        for row in v:
            fh.write("%.17g %.17g %.17g\n" % tuple(row))
        for row in t:
            fh.write("3 %d %d %d\n" % tuple(int(i) for i in row))

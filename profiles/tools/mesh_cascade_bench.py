"""Coarse-to-fine cascade in space against the cold solve: for a workload and n_time, ``solver_socp`` on the finest mesh and
``solver_socp_mesh_cascade`` with one, two and three coarse levels below it in one process, alternating, the host clock around each
WHOLE call (plans, factorisations of every level, transfers, iterations, download of the solution) ending in a device synchronise;
per level the stopping iteration and seconds, and the transfer's device milliseconds and bytes.

    python profiles/tools/mesh_cascade_bench.py --mesh torus100k --T 31 [--depths 1,2,3] [--tol 1e-4] [--reps 2] [--level-tol 1e-3]

The meshes are nested by construction: the generator's grid at (nu, nv) / 2^d is the coarsest level, and every refinement step snaps
the edge midpoints to the generator's grid at twice the resolution (meshes.snap_projection), so the finest level is the generator's
own mesh at (nu, nv), triangulated as ``_periodic_grid_triangles`` does, numbered by the subdivision.  ``torus100k`` is the torus at
400 x 256 (102 400 vertices): the 400 x 250 of bench.py has a single nested level below it (250 / 4 is not an integer).  The knot is
bench.py's 216 x 20 tube: two nested levels exist below it (108 x 10, 54 x 5), so a depth of three is refused.  All levels are
normalised with the finest mesh's bounding box; the densities are the recipe of ``meshes.example`` around three vertices of the
coarsest level (present on every level).  Building the levels on the host is not part of the timed calls: they are the input.

``--grids 100x63,200x125,400x250`` (coarse to fine) gives the hierarchy as generator grids of the workload's surface instead: the levels
are then independent triangulations, none nested in another, linked by ``meshes.link_levels`` (every level located on the one below,
the state carried over barycentrically by ``dots_transfer_space``), the finest grid is the workload (400x250 is bench.py's own
torus100k), and ``--depths`` counts coarse levels from the finest grid down (default: every depth the list allows).  The densities are
the same bumps around the points of three vertices of the coarsest grid.  The seconds the hierarchy took to build (``hierarchy_s``:
meshes, location, densities) are printed in every line; they are not part of the timed calls either.

``--coarsen K`` adds ``solver_socp_auto_cascade`` with K coarse levels to the alternation (kind = "auto"): the caller has the finest
mesh only, the coarse levels are decimated from it (``meshes.coarsen_levels``) and located on the device INSIDE the timed call.  Before
the alternation one line (kind = "levels") gives, per pair of decimated levels, the seconds of the coarsening and of
``cascade.mesh_transfer`` with ``locate="kdtree"`` and ``locate="device"`` (entry to return, and the kernels' own milliseconds).
``torus400x250`` is bench.py's own torus: one nested level exists below it (``--depths 1``).

Prints one JSON line per call (kind = "cold" / "cascade" / "auto") and a summary line.  The transfer's device milliseconds are set against the
bytes it moves (every source and destination array once) at 6.3 TB/s, the copy rate DESIGN.md quotes.  bench.py is unchanged."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

COPY_BPS = 6.3e12
GRIDS = {"torus100k": ("torus", 400, 256), "torus400x250": ("torus", 400, 250), "knot": ("knot", 216, 20), "torus6k": ("torus", 96, 64)}


def generator(kind, nu, nv):
    from dots_socp_amd import meshes

    return meshes.torus(nu, nv) if kind == "torus" else meshes.torus_knot_tube(2, 5, nu, nv)


def build_levels(mesh, depth):
    """``depth + 1`` nested geometries, coarse to fine, the last one the generator's mesh at its full resolution."""
    import numpy as np

    from dots_socp_amd import meshes

    kind, nu, nv = GRIDS[mesh]
    if nu % (1 << depth) or nv % (1 << depth) or (nv >> depth) < 3:
        raise SystemExit(f"{mesh}: {nu} x {nv} has no nested level {depth} steps down")
    fine_v = generator(kind, nu, nv)[0]
    lo, scale = fine_v.min(axis=0), 1.0 / (fine_v.max(axis=0) - fine_v.min(axis=0)).max()
    norm = lambda v: (v - lo) * scale      # noqa: E731
    v0, t0 = generator(kind, nu >> depth, nv >> depth)
    coarse, _ = meshes.make_geometry(norm(v0), t0, normalize=False)
    c = meshes.farthest_vertices(coarse["vertices"], 0, 3)
    dens = lambda v, a: (meshes.bump_density(v, a, [c[0]], 0.35, 0.05), meshes.bump_density(v, a, [c[1], c[2]], 0.35, 0.05))      # noqa: E731
    coarse["mu0"], coarse["mu1"] = dens(coarse["vertices"], coarse["area_vertices"])
    steps = [meshes.snap_projection(norm(generator(kind, nu >> d, nv >> d)[0])) for d in range(depth - 1, -1, -1)]
    levels = meshes.refine_levels(coarse, depth + 1, project=steps, densities=dens)
    assert np.asarray(levels[-1]["vertices"]).shape[0] == nu * nv
    return levels


def build_grid_levels(mesh, grids):
    """The generator's meshes at ``grids`` = [(nu, nv), ...] (coarse to fine), normalised with the finest mesh's bounding box and linked
    by ``meshes.link_levels``: independent triangulations of one surface."""
    import numpy as np

    from dots_socp_amd import meshes

    kind = GRIDS[mesh][0]
    raw = [generator(kind, nu, nv) for nu, nv in grids]
    fine_v = raw[-1][0]
    lo, scale = fine_v.min(axis=0), 1.0 / (fine_v.max(axis=0) - fine_v.min(axis=0)).max()
    geoms = [meshes.make_geometry((v - lo) * scale, t, normalize=False)[0] for v, t in raw]
    centres = geoms[0]["vertices"][meshes.farthest_vertices(geoms[0]["vertices"], 0, 3)]

    def dens(v, a):      # the recipe of meshes.example around the vertex of this level nearest to each centre
        c = [int(np.argmin(np.linalg.norm(v - p, axis=1))) for p in centres]
        return meshes.bump_density(v, a, [c[0]], 0.35, 0.05), meshes.bump_density(v, a, [c[1], c[2]], 0.35, 0.05)

    geoms[0]["mu0"], geoms[0]["mu1"] = dens(geoms[0]["vertices"], geoms[0]["area_vertices"])
    return meshes.link_levels(geoms, densities=dens)


def level_pair_times(fine, n_coarse):
    """Per pair of decimated levels below ``fine`` (fine to coarse): the seconds of the coarsening, of mesh_transfer with the kd-tree
    candidates on the host and with the exact location on the device, and the device milliseconds of the location kernels."""
    import numpy as np

    from dots_socp_amd import cascade, meshes

    pairs, above = [], fine
    for _ in range(n_coarse):
        t0 = time.perf_counter()
        v, t, _ = meshes.coarsen(above["vertices"], above["triangles"])
        t1 = time.perf_counter()
        below, _ = meshes.make_geometry(v, t, normalize=False)
        t2 = time.perf_counter()
        cascade.mesh_transfer(below, above, locate="kdtree")
        t3 = time.perf_counter()
        cascade.mesh_transfer(below, above, locate="device")
        t4 = time.perf_counter()
        tf = np.asarray(above["triangles"])
        vf = np.asarray(above["vertices"], dtype=np.float64)
        timing = {}
        cascade.locate_device(np.concatenate([vf, (vf[tf[:, 0]] + vf[tf[:, 1]] + vf[tf[:, 2]]) / 3.0]), v, t, timing=timing)
        pairs.append({"fine_vertices": int(vf.shape[0]), "coarse_vertices": int(v.shape[0]), "coarsen_s": round(t1 - t0, 4),
                      "locate_kdtree_s": round(t3 - t2, 4), "locate_device_s": round(t4 - t3, 4), "locate_kernel_ms": round(timing["kernel_ms"], 3)})
        above = below
    return pairs


def sync():
    import torch

    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="knot", choices=sorted(GRIDS))
    ap.add_argument("--T", type=int, default=31)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--nit", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--depths", default=None, help="comma-separated numbers of coarse levels (default 1,2,3; with --grids every depth the list allows)")
    ap.add_argument("--grids", default=None, help="the hierarchy as generator grids, coarse to fine, e.g. 100x63,200x125,400x250 (located levels)")
    ap.add_argument("--level-tol", type=float, default=None)
    ap.add_argument("--coarsen", type=int, default=0, help="add the auto cascade with this many decimated coarse levels (built inside the timed call)")
    ap.add_argument("--congestion", type=float, default=0.0)
    a = ap.parse_args()

    import numpy as np

    from dots_socp_amd.socp import solver_socp, solver_socp_auto_cascade, solver_socp_mesh_cascade

    t_build = time.perf_counter()
    if a.grids:
        grids = [tuple(int(n) for n in g.split("x")) for g in a.grids.split(",")]
        if len(grids) < 2 or any(len(g) != 2 for g in grids):
            raise SystemExit("--grids: at least two grids NUxNV, coarse to fine")
        depths = [int(x) for x in a.depths.split(",")] if a.depths else list(range(1, len(grids)))
        if max(depths) > len(grids) - 1 or min(depths) < 1:
            raise SystemExit(f"--depths: {len(grids)} grids give 1 .. {len(grids) - 1} coarse levels")
        deepest = build_grid_levels(a.mesh, grids)
    else:
        depths = [int(x) for x in (a.depths or "1,2,3").split(",")]
        deepest = build_levels(a.mesh, max(depths))
    hierarchy_s = round(time.perf_counter() - t_build, 3)
    fine = deepest[-1]
    V = int(np.asarray(fine["vertices"]).shape[0])
    common = dict(tol=a.tol, nit=a.nit, congestion=a.congestion, time_limit=1e9)
    base = dict(mesh=a.mesh, n_time=a.T, vertices=V, tol=a.tol, congestion=a.congestion, hierarchy_s=hierarchy_s)
    if a.grids:
        base["grids"] = a.grids
    best = {}
    plain = {k: v for k, v in fine.items() if k not in ("parents", "transfer")}      # what a caller with one mesh has
    if a.coarsen:
        print(json.dumps(dict(base, kind="levels", pairs=level_pair_times(plain, a.coarsen))), flush=True)
    for rep in range(a.reps):
        for depth in [0] + depths + (["auto"] if a.coarsen else []):
            kind = "cold" if depth == 0 else "auto" if depth == "auto" else "cascade"
            sync()
            t0 = time.perf_counter()
            if depth == 0:
                sol, hist = solver_socp(a.T, fine, **common)
            elif depth == "auto":
                sol, hist = solver_socp_auto_cascade(a.T, plain, coarse_levels=a.coarsen, level_tol=a.level_tol, **common)
            else:
                sol, hist = solver_socp_mesh_cascade(a.T, deepest[-depth - 1:], level_tol=a.level_tol, **common)
            sync()
            wall = time.perf_counter() - t0
            out = dict(base, kind=kind, depth=depth, rep=rep, wall_s=round(wall, 4), iterations=int(hist.kkt_iteration[-1]) + 1,
                       running_time=round(float(hist.running_time), 4), cost=float(hist.history["Transportation cost"][-1]),
                       kkt_max=float(np.nanmax(np.asarray(hist.kkt_errors[-1], dtype=np.float64))))
            if depth == "auto":
                out["coarse_levels"] = a.coarsen
                out["build"] = hist.solver_stats["auto_cascade"]
            if depth:
                rec = hist.solver_stats["mesh_cascade"]["levels"]
                for r in rec:
                    if r["prolong_ms"]:
                        r["prolong_floor_ms"] = round(1e3 * r["prolong_bytes"] / COPY_BPS, 4)
                        r["prolong_tb_per_s"] = round(r["prolong_bytes"] / (1e-3 * r["prolong_ms"]) / 1e12, 3)
                out["levels"] = rec
                out["level_tol"] = a.level_tol
            best[depth] = min(best.get(depth, wall), wall)
            del sol, hist
            print(json.dumps(out), flush=True)
    print(json.dumps(dict(base, kind="summary", level_tol=a.level_tol, cold_wall_s=round(best[0], 4),
                          cascade_wall_s={str(d): round(best[d], 4) for d in depths}, auto_wall_s=round(best["auto"], 4) if a.coarsen else None,
                          cold_over_cascade={str(d): round(best[0] / best[d], 3) for d in depths})), flush=True)


if __name__ == "__main__":
    main()

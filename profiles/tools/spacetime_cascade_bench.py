"""Cascade in space and time at once against the cascade in space and the cold solve: for a workload and n_time, ``solver_socp`` on the
finest mesh, ``solver_socp_mesh_cascade`` with two coarse levels below it (the best the mesh cascade measured) and
``solver_socp_spacetime_cascade`` on the same three meshes with its default levels, in one process, alternating, the host clock around
each WHOLE call (plans, factorisations of every level, transfers, iterations, download of the solution) ending in a device synchronise;
per level n_time, the stopping iteration and seconds, and the carrier's device milliseconds and bytes.

    python profiles/tools/spacetime_cascade_bench.py --mesh torus100k --T 127 [--levels 31,63,127] [--tol 1e-4] [--reps 2] [--level-tol 1e-3]

The hierarchy is ``mesh_cascade_bench.build_levels``'s: nested by construction, the finest level the generator's own mesh (``torus100k``:
the torus at 400 x 256), all levels normalised together, the same three bumps on every level; building it is not part of the timed
calls.  Prints one JSON line per call (kind = "cold" / "mesh_cascade" / "spacetime_cascade") and a summary line.  A carrier's device
milliseconds are set against ``prolong_bytes`` at 6.3 TB/s, the copy rate DESIGN.md quotes: a sanity figure.  bench.py is unchanged."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mesh_cascade_bench import COPY_BPS, GRIDS, build_levels, sync      # noqa: E402

DEPTH = 2      # coarse levels below the finest mesh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="torus100k", choices=sorted(GRIDS))
    ap.add_argument("--T", type=int, default=127)
    ap.add_argument("--levels", default=None, help="n_time per mesh level, coarse to fine (default: the driver's)")
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--nit", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--level-tol", type=float, default=None)
    ap.add_argument("--congestion", type=float, default=0.0)
    a = ap.parse_args()

    import numpy as np

    from dots_socp_amd import cascade
    from dots_socp_amd.socp import solver_socp, solver_socp_mesh_cascade, solver_socp_spacetime_cascade

    t_build = time.perf_counter()
    geoms = build_levels(a.mesh, DEPTH)
    hierarchy_s = round(time.perf_counter() - t_build, 3)
    levels = cascade.check_spacetime_levels([int(x) for x in a.levels.split(",")] if a.levels else None, a.T, len(geoms))
    fine = geoms[-1]
    common = dict(tol=a.tol, nit=a.nit, congestion=a.congestion, time_limit=1e9)
    base = dict(mesh=a.mesh, n_time=a.T, vertices=int(np.asarray(fine["vertices"]).shape[0]), tol=a.tol, congestion=a.congestion,
                hierarchy_s=hierarchy_s, levels_n_time=levels, level_tol=a.level_tol)
    kinds = ("cold", "mesh_cascade", "spacetime_cascade")
    best, carriers = {}, None
    for rep in range(a.reps):
        for kind in kinds:
            sync()
            t0 = time.perf_counter()
            if kind == "cold":
                sol, hist = solver_socp(a.T, fine, **common)
            elif kind == "mesh_cascade":
                sol, hist = solver_socp_mesh_cascade(a.T, geoms, level_tol=a.level_tol, **common)
            else:
                sol, hist = solver_socp_spacetime_cascade(a.T, geoms, levels=levels, level_tol=a.level_tol, **common)
            sync()
            wall = time.perf_counter() - t0
            out = dict(base, kind=kind, rep=rep, wall_s=round(wall, 4), iterations=int(hist.kkt_iteration[-1]) + 1,
                       running_time=round(float(hist.running_time), 4), cost=float(hist.history["Transportation cost"][-1]),
                       kkt_max=float(np.nanmax(np.asarray(hist.kkt_errors[-1], dtype=np.float64))))
            if kind != "cold":
                rec = hist.solver_stats[kind]["levels"]
                for r in rec:
                    if r["prolong_ms"]:
                        r["prolong_floor_ms"] = round(1e3 * r["prolong_bytes"] / COPY_BPS, 4)
                        r["prolong_tb_per_s"] = round(r["prolong_bytes"] / (1e-3 * r["prolong_ms"]) / 1e12, 3)
                out["levels"] = rec
                if kind == "spacetime_cascade":
                    carriers = [dict(n_time=r["n_time"], prolong_ms=r["prolong_ms"], prolong_bytes=r["prolong_bytes"],
                                     prolong_floor_ms=r.get("prolong_floor_ms")) for r in rec[1:]]
            best[kind] = min(best.get(kind, wall), wall)
            del sol, hist
            print(json.dumps(out), flush=True)
    print(json.dumps(dict(base, kind="summary", wall_s={k: round(best[k], 4) for k in kinds},
                          cold_over={k: round(best["cold"] / best[k], 3) for k in kinds[1:]},
                          mesh_over_spacetime=round(best["mesh_cascade"] / best["spacetime_cascade"], 3), carriers=carriers)), flush=True)


if __name__ == "__main__":
    main()

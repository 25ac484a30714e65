"""Coarse-to-fine time cascade against the cold solve: for a workload and n_time, ``solver_socp`` and ``solver_socp_cascade`` in one
process, alternating, the host clock around each WHOLE call (plans, factorisations of every level, prolongations, iterations,
download of the solution) ending in a device synchronise; per level the iterations and seconds.

    python profiles/tools/cascade_bench.py --mesh knot --T 127 [--tol 1e-4] [--reps 2] [--levels 31,127] [--level-tol 1e-3]

Prints one JSON line per call (kind = "cold" / "cascade") and a summary line.  The prolongation's device milliseconds are set against
the bytes it moves (every source and destination array once) at 6.3 TB/s, the copy rate DESIGN.md quotes.  bench.py is unchanged; this
script only reuses its mesh recipes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MESHES = {"knot": ("knot", {}), "torus100k": ("torus", dict(nu=400, nv=250)), "sphere10k": ("sphere", dict(level=5))}
COPY_BPS = 6.3e12


def pitch(n_time):
    p = 8
    while p < n_time + 1:
        p <<= 1
    return p


def state_bytes(V, F, n_time):
    """the twelve state arrays in the device layout: 7 vertex arrays + phi, B and E (3 F rows each), z_mid and beta_mid (18 F rows each)"""
    return 8 * pitch(n_time) * (8 * V + 2 * 3 * F + 2 * 18 * F)


def sync():
    import torch

    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="knot", choices=sorted(MESHES))
    ap.add_argument("--T", type=int, default=127)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--nit", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--levels", default=None, help="comma-separated n_time values (default: the solver's rule)")
    ap.add_argument("--level-tol", type=float, default=None)
    ap.add_argument("--congestion", type=float, default=0.0)
    a = ap.parse_args()

    import numpy as np

    from dots_socp_amd import meshes
    from dots_socp_amd.socp import solver_socp, solver_socp_cascade

    name, kw = MESHES[a.mesh]
    geom, _ = meshes.example(name, **kw)
    V, F = np.asarray(geom["vertices"]).shape[0], np.asarray(geom["triangles"]).shape[0]
    levels = None if a.levels is None else [int(x) for x in a.levels.split(",")]
    common = dict(tol=a.tol, nit=a.nit, congestion=a.congestion, time_limit=1e9)
    base = dict(mesh=a.mesh, n_time=a.T, vertices=int(V), tol=a.tol, congestion=a.congestion)
    best = {}
    for rep in range(a.reps):
        for kind in ("cold", "cascade"):
            sync()
            t0 = time.perf_counter()
            if kind == "cold":
                sol, hist = solver_socp(a.T, geom, **common)
            else:
                sol, hist = solver_socp_cascade(a.T, geom, levels=levels, level_tol=a.level_tol, **common)
            sync()
            wall = time.perf_counter() - t0
            out = dict(base, kind=kind, rep=rep, wall_s=round(wall, 4), iterations=int(hist.kkt_iteration[-1]) + 1,
                       running_time=round(float(hist.running_time), 4), cost=float(hist.history["Transportation cost"][-1]),
                       kkt_max=float(np.nanmax(np.asarray(hist.kkt_errors[-1], dtype=np.float64))))
            if kind == "cascade":
                rec = hist.solver_stats["cascade"]["levels"]
                for prev, r in zip([None] + rec[:-1], rec):
                    if prev is not None:
                        nbytes = state_bytes(V, F, prev["n_time"]) + state_bytes(V, F, r["n_time"])
                        r["prolong_bytes"] = nbytes
                        r["prolong_floor_ms"] = round(1e3 * nbytes / COPY_BPS, 4)
                out["levels"] = rec
                out["level_tol"] = a.level_tol
            best[kind] = min(best.get(kind, wall), wall)
            del sol, hist
            print(json.dumps(out), flush=True)
    print(json.dumps(dict(base, kind="summary", cold_wall_s=round(best["cold"], 4), cascade_wall_s=round(best["cascade"], 4),
                          cold_over_cascade=round(best["cold"] / best["cascade"], 3))), flush=True)


if __name__ == "__main__":
    main()

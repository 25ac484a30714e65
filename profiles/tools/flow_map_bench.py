"""The flow map at the end of a solve (dots_flow_map): device milliseconds of the one launch and the bytes that cross to the host,
against the bytes of downloading ``mu`` and ``E`` -- what a caller had to move before to trace particles in Python.

    python profiles/tools/flow_map_bench.py --mesh torus100k --T 31 [--particles N] [--nit 100] [--tol 1e-4] [--reps 5] [--trajectory]

The state is what ``--nit`` ALM iterations leave (a transport on its way: the map needs velocities, not a converged solve).
``--particles``: that many starts, the vertex starts repeated (default: one per vertex).  Prints one JSON line per repetition and a
summary line.  bench.py is unchanged; this script only reuses its mesh recipes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MESHES = {"plane": ("plane", dict(n=20)), "knot": ("knot", {}), "torus100k": ("torus", dict(nu=400, nv=250)), "sphere10k": ("sphere", dict(level=5))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="knot", choices=sorted(MESHES))
    ap.add_argument("--T", type=int, default=31)
    ap.add_argument("--particles", type=int, default=0)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--nit", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trajectory", action="store_true")
    a = ap.parse_args()

    import numpy as np

    from dots_socp_amd import flow, meshes
    from dots_socp_amd.socp.solver_socp import AlmSolver

    name, kw = MESHES[a.mesh]
    geom, _ = meshes.example(name, **kw)
    V, F = np.asarray(geom["vertices"]).shape[0], np.asarray(geom["triangles"]).shape[0]
    tri, w = flow.vertex_starts(geom["triangles"], V)
    P = a.particles or V
    pick = np.arange(P) % V
    starts = (np.ascontiguousarray(tri[pick]), np.ascontiguousarray(w[pick]))
    download_bytes = 8 * (a.T * V + (a.T + 1) * 3 * F)      # mu and E, the arrays a host tracer needs
    base = dict(mesh=a.mesh, n_time=a.T, vertices=int(V), triangles=int(F), particles=int(P), trajectory=bool(a.trajectory), nit=a.nit)
    alm = AlmSolver(a.T, geom, tol=a.tol, nit=a.nit, time_limit=1e9)
    try:
        for _ in range(a.nit):
            if alm.iterate():
                break
        alm.dev.sync()
        best = None
        for rep in range(a.reps):
            t0 = time.perf_counter()
            out = alm.flow_map(starts=starts, trajectory=a.trajectory)
            wall = time.perf_counter() - t0
            rec = dict(base, kind="flow_map", rep=rep, device_ms=round(out["ms"], 4), wall_s=round(wall, 5), crossed_bytes=int(out["bytes"]),
                       download_bytes=int(download_bytes), download_over_crossed=round(download_bytes / out["bytes"], 1),
                       stopped=int(np.sum(out["status"] == 1)), rested=int(np.sum(out["rested"])), crossings=int(np.sum(out["crossings"])),
                       crossings_max=int(np.max(out["crossings"])))
            best = rec if best is None or rec["device_ms"] < best["device_ms"] else best
            print(json.dumps(rec), flush=True)
        t0 = time.perf_counter()
        mu, E = alm.dev.download("mu"), alm.dev.download("E")
        rec = dict(base, kind="download", wall_s=round(time.perf_counter() - t0, 5), bytes=int(mu.nbytes + E.nbytes))
        print(json.dumps(rec), flush=True)
        print(json.dumps(dict(best, kind="summary", download_wall_s=rec["wall_s"])), flush=True)
    finally:
        alm.close()


if __name__ == "__main__":
    main()

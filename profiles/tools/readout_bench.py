"""The end of a solve, read out on the device against the download + numpy path: whole ``solver()`` calls in one process,
alternating ``readout="host"`` (the reference of every time here), ``"device"`` (copies straight into the caller's pageable arrays)
and ``"device"`` with ``DOTS_READOUT_PINNED=8192`` (copies through two pinned 8 MB slots of the context), the host clock around each call ending
in a device synchronise.  Inside each call the read-out alone is bracketed: ``finalize_s`` (AlmSolver.finalize, entry to return),
``tail_s`` (finalize entry to the plug-in's return: the host path converts units and centres after finalize), and for the device
paths the milliseconds of the read-out launches with the bytes they move (every value of mu and E read once and written once) over
that time, beside the 6.3 TB/s copy rate DESIGN.md quotes.

    python profiles/tools/readout_bench.py --mesh torus100k --T 31 [--tol 1e-4] [--nit 300] [--reps 3]

Prints one JSON line per call and a summary line.  bench.py is unchanged; this script only reuses its mesh recipes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MESHES = {"knot": ("knot", {}), "torus100k": ("torus", dict(nu=400, nv=250)), "sphere10k": ("sphere", dict(level=5))}
COPY_BPS = 6.3e12
KINDS = (("host", "host", "0"), ("device", "device", "0"), ("device_pinned", "device", "8192"))


def sync():
    import torch

    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="knot", choices=sorted(MESHES))
    ap.add_argument("--T", type=int, default=31)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--nit", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()

    import numpy as np

    from dots_socp_amd import meshes
    from dots_socp_amd.socp import solver
    from dots_socp_amd.socp.solver_socp import AlmSolver

    clock = {}
    finalize = AlmSolver.finalize

    def timed_finalize(self, *args, **kw):
        clock["enter"] = time.perf_counter()
        out = finalize(self, *args, **kw)
        clock["leave"] = time.perf_counter()
        return out

    AlmSolver.finalize = timed_finalize
    name, kw = MESHES[a.mesh]
    geom, _ = meshes.example(name, **kw)
    V, F = np.asarray(geom["vertices"]).shape[0], np.asarray(geom["triangles"]).shape[0]
    base = dict(mesh=a.mesh, n_time=a.T, vertices=int(V), triangles=int(F), tol=a.tol, nit=a.nit)
    best = {}
    for rep in range(a.reps):
        for kind, readout, pinned in KINDS:
            os.environ["DOTS_READOUT_PINNED"] = pinned
            sync()
            t0 = time.perf_counter()
            sol, hist = solver(a.T, geom, readout=readout, tol=a.tol, nit=a.nit, time_limit=1e9)
            t1 = time.perf_counter()
            sync()
            out = dict(base, kind=kind, rep=rep, wall_s=round(time.perf_counter() - t0, 4), finalize_s=round(clock["leave"] - clock["enter"], 5),
                       tail_s=round(t1 - clock["enter"], 5), iterations=int(hist.kkt_iteration[-1]) + 1,
                       returned_bytes=int(sol["mu"].nbytes + sol["E"].nbytes), cost=float(hist.history["Transportation cost"][-1]))
            ro = hist.solver_stats.get("readout")
            if ro:
                moved = 2 * 8 * (a.T * V + (a.T + 1) * 3 * F)      # mu and E read once; the output written once
                out.update(readout_ms=round(ro["ms"], 4), copied_bytes=int(ro["bytes"]), launch_bytes=moved,
                           launch_TBps=round(moved / (1e-3 * ro["ms"]) / 1e12, 3), copy_rate_TBps=COPY_BPS / 1e12)
            for key in ("wall_s", "finalize_s", "tail_s"):
                best[kind, key] = min(best.get((kind, key), out[key]), out[key])
            del sol, hist
            print(json.dumps(out), flush=True)
    os.environ.pop("DOTS_READOUT_PINNED", None)
    summary = dict(base, kind="summary")
    for (kind, key), v in sorted(best.items()):
        summary[f"{kind}_{key}"] = v
    for kind in ("device", "device_pinned"):
        summary[f"host_over_{kind}_finalize"] = round(best["host", "finalize_s"] / best[kind, "finalize_s"], 3)
        summary[f"host_over_{kind}_tail"] = round(best["host", "tail_s"] / best[kind, "tail_s"], 3)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()

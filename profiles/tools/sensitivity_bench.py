"""The cost gradients read out on the device (dots_sensitivity) against the path that exists without it: download of ``phi`` and
``mu`` plus a vectorised numpy evaluation of the same tensor (sensitivity.stress_numpy: the same bits).  No solve: the call's time
does not depend on the values, so a random state is uploaded to a context in the solver's "nd" numbering.

    python profiles/tools/sensitivity_bench.py --mesh torus100k --T 31 [--reps 5]

Per repetition one JSON line per path: ``device`` (outputs copied to the host), ``device_tensors`` (outputs left on the device as torch
tensors) and ``download_numpy``; host clock around each call ending in a device synchronise, and for the device paths the
milliseconds of the two launches.  The kernel's yardstick is bytes over time beside the 6.3 TB/s copy rate DESIGN.md quotes:
``unique_bytes`` counts phi, mu and the outputs once, ``requested_bytes`` every lane's loads (a corner lane reads four rows; the
three corners of a triangle and the triangles round a vertex share theirs through the caches).  A summary line has the best of
each.  bench.py is unchanged; this script only reuses its mesh recipes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MESHES = {"knot": ("knot", {}), "torus100k": ("torus", dict(nu=400, nv=250))}
COPY_BPS = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="knot", choices=sorted(MESHES))
    ap.add_argument("--T", type=int, default=31, choices=(31, 127))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()

    import numpy as np
    import torch

    from dots_socp_amd import meshes, sensitivity
    from dots_socp_amd.device import DeviceProblem

    name, kw = MESHES[a.mesh]
    geom, _ = meshes.example(name, **kw)
    tri = np.asarray(geom["triangles"])
    mass = np.asarray(geom["area_vertices"], dtype=np.float64) / 3.0
    dev = DeviceProblem(a.T, geom, lap_solver="spacetime_pcg", reorder="nd")
    V, F, T = dev.V, dev.F, a.T
    rng = np.random.default_rng(0)
    dev.upload("mu", 1.0 - rng.random((T, V)))
    dev.upload("phi", rng.standard_normal((T + 1, V)))
    f_phi, f_mu = 0.8125, 1.7
    base = dict(mesh=a.mesh, n_time=T, vertices=int(V), triangles=int(F), pitch=dev._state_pitch())
    unique = 8 * ((2 * T + 1) * V + 2 * V + 18 * F)
    requested = 8 * (3 * F * 4 * (T + 1) + 2 * V + 18 * F)
    best, last = {}, {}

    def record(kind, wall, **more):
        out = dict(base, kind=kind, wall_s=round(wall, 6), **more)
        for key in ("wall_s", "device_ms"):
            if key in out:
                best[kind, key] = min(best.get((kind, key), out[key]), out[key])
        print(json.dumps(out), flush=True)

    def device_fields():
        ms = dev.sensitivity_ms
        return dict(device_ms=round(ms, 4), bytes_to_host=int(dev.sensitivity_bytes), unique_bytes=unique, requested_bytes=requested,
                    unique_TBps=round(unique / (1e-3 * ms) / 1e12, 3), requested_TBps=round(requested / (1e-3 * ms) / 1e12, 3),
                    copy_rate_TBps=COPY_BPS / 1e12)

    try:
        for rep in range(a.reps + 1):      # (repetition 0 warms up: first launch of the kernels, the inverse numbering, torch's allocator)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last["device"] = dev.sensitivity(f_phi, f_mu, mass)
            wall = time.perf_counter() - t0
            if rep:
                record("device", wall, rep=rep, **device_fields())
            t0 = time.perf_counter()
            on_dev = dev.sensitivity(f_phi, f_mu, mass, to_device=True)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if rep:
                record("device_tensors", wall, rep=rep, **device_fields())
            del on_dev
            before = dev.debug_counter(9)
            t0 = time.perf_counter()
            phi, mu = dev.download("phi"), dev.download("mu")
            t1 = time.perf_counter()
            p0, pT = sensitivity.potentials_host(phi, f_phi)
            last["numpy"] = {"phi0": p0, "phiT": pT, "stress": sensitivity.stress_numpy(mu, phi, tri, mass, f_mu, f_phi)}
            wall = time.perf_counter() - t0
            if rep:
                record("download_numpy", wall, rep=rep, download_s=round(t1 - t0, 6), numpy_s=round(wall - (t1 - t0), 6),
                       bytes_to_host=int(dev.debug_counter(9) - before))
        equal = all(np.array_equal(last["device"][k].view(np.int64), last["numpy"][k].view(np.int64)) for k in ("phi0", "phiT", "stress"))
    finally:
        dev.close()
    summary = dict(base, kind="summary", same_bits=bool(equal), unique_bytes=unique, requested_bytes=requested)
    for (kind, key), v in sorted(best.items()):
        summary[f"{kind}_{key}"] = v
    summary["unique_TBps_at_best_ms"] = round(unique / (1e-3 * best["device", "device_ms"]) / 1e12, 3)
    summary["download_numpy_over_device_wall"] = round(best["download_numpy", "wall_s"] / best["device", "wall_s"], 2)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()

"""Long time horizons (T + 1 in (256, 1024]) with the direct solver: steady ALM it/s, solve ms and the sweeps' achieved fraction of 8 TB/s
on algorithmic bytes (dots_front_info / bench_kernel 3), optionally against spacetime_pcg on the same problem.

    python profiles/tools/long_horizon_bench.py --mesh knot --T 511 [--steps 40 --warmup 10] [--spacetime-steps 5]

Prints one JSON line per configuration.  bench.py is unchanged; this script only reuses its mesh recipes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MESHES = {"knot": ("knot", {}), "torus100k": ("torus", dict(nu=400, nv=250))}
PEAK_BPS = 8.0e12


def steady(alm, steps, warmup):
    for _ in range(warmup):
        alm.iterate()
    alm.dev.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        alm.iterate()
    alm.dev.sync()
    return steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="knot", choices=sorted(MESHES))
    ap.add_argument("--T", type=int, default=511)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--spacetime-steps", type=int, default=0, help="also time this many iterations of spacetime_pcg (0: skip)")
    a = ap.parse_args()

    from dots_socp_amd import meshes
    from dots_socp_amd.socp.solver_socp import AlmSolver

    name, kw = MESHES[a.mesh]
    geom, _ = meshes.example(name, **kw)
    nit = a.steps + a.warmup + 10
    t0 = time.perf_counter()
    alm = AlmSolver(a.T, geom, nit=nit, tol=1e-12)
    setup_s = time.perf_counter() - t0
    its = steady(alm, a.steps, a.warmup)
    ms, alg_bytes = alm.dev.bench_kernel(3, reps=10)
    out = dict(mesh=a.mesh, n_time=a.T, vertices=int(alm.dev.V), setup_s=round(setup_s, 3), it_per_s=round(its, 3), solve_ms=round(ms, 4),
               sweep_bytes=alg_bytes, sweep_peak_fraction=round(alg_bytes / (ms * 1e-3) / PEAK_BPS, 4),
               factor_bytes_per_solve=alm.front_summary.get("bytes_per_solve_as_installed"), bands=alm.front_summary.get("bands"))
    alm.close()
    if a.spacetime_steps > 0:
        pcg = AlmSolver(a.T, geom, nit=a.spacetime_steps + 12, tol=1e-12, lap_solver="spacetime_pcg", preconditioner="jacobi")
        out["spacetime_pcg_it_per_s"] = round(steady(pcg, a.spacetime_steps, 2), 4)
        out["direct_over_spacetime"] = round(its / out["spacetime_pcg_it_per_s"], 2)
        pcg.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""Batched ALM iterations on one factor: B contexts share the factor of the first (dots_front_share) and advance in lockstep, one
iteration each with ONE batched pair of sweeps (dots_step_many).  One JSON line per batch size.

    python profiles/tools/batch_bench.py --workload torus100k --batch 1,2,4,8 --steps 50 --warmup 10

Densities: bumps at farthest-point centres from a seed (meshes.bump_density); iterations are quiet (z_mid not stored, gathers carried),
as the quiet iterations of a solve.  Per line: aggregate ALM iterations/s (sum over the B problems; host clock around the timed window,
the streams synchronised at both ends), ms per batched iteration, the batched sweeps alone timed by device events (dots_bench_many) with
the factor bytes per problem they imply, and the setup seconds (factor built once).  DOTS_FRONT_NR=2/4/8 selects the rhs per launch."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from dots_socp_amd import meshes  # noqa: E402
from dots_socp_amd.device import DeviceProblem, bench_many, step_many  # noqa: E402
from dots_socp_amd.geometry import build_plan, plan_with_densities  # noqa: E402

WORKLOADS = {"knot": ("knot", {}, 31), "sphere10k": ("sphere", dict(level=5), 31), "torus100k": ("torus", dict(nu=400, nv=250), 31)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="knot", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", default="1,2,4,8")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    name, kw, T = WORKLOADS[a.workload]
    geom, _ = meshes.example(name, **kw)
    sizes = [int(s) for s in a.batch.split(",")]
    v = np.asarray(geom["vertices"])
    av = meshes.vertex_areas(v.shape[0], geom["triangles"], meshes.triangle_areas(v, geom["triangles"]))
    rng = np.random.default_rng(a.seed)
    t0 = time.perf_counter()
    base = build_plan(T, geom, reorder="nd")
    devs = []
    for k in range(max(sizes)):
        c = meshes.farthest_vertices(v, int(rng.integers(v.shape[0])), 4)
        d = DeviceProblem(T, geom, lap_solver="modal_pcg", plan=plan_with_densities(base, meshes.bump_density(v, av, c[:2]), meshes.bump_density(v, av, c[2:])))
        d.set_params(eps=0.0)
        if k == 0:
            summary = d.setup_frontal(eps=0.0)
            setup_s = time.perf_counter() - t0
        else:
            d.share_frontal(devs[0])
        d.step_flags(skip_z_mid=True, carry=True)
        devs.append(d)
    factor_bytes = float(summary["bytes_per_solve_as_installed"])

    for B in sizes:
        grp = devs[:B]
        for _ in range(a.warmup):
            for d in grp:
                d.step_flags(skip_z_mid=True, carry=True)
            step_many(grp)
        for d in grp:
            d.sync()
        t = time.perf_counter()
        for _ in range(a.steps):
            for d in grp:
                d.step_flags(skip_z_mid=True, carry=True)
            step_many(grp)
        for d in grp:
            d.sync()
        wall = time.perf_counter() - t
        sweep_ms = bench_many(grp, reps=max(10, a.steps // 2))
        print(json.dumps({"workload": a.workload, "batch": B, "nr_max": os.environ.get("DOTS_FRONT_NR", "4"), "setup_s": round(setup_s, 3),
                          "alm_iterations_per_s": round(B * a.steps / wall, 1), "ms_per_batched_iteration": round(1e3 * wall / a.steps, 4),
                          "ms_batched_sweeps": round(sweep_ms, 4), "ms_sweeps_per_problem": round(sweep_ms / B, 4),
                          "factor_bytes_per_problem": factor_bytes / B,
                          "factor_GBps": round(factor_bytes / (sweep_ms * 1e-3) / 1e9, 1)}), flush=True)
    for d in reversed(devs):
        d.close()


if __name__ == "__main__":
    main()

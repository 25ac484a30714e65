"""Long horizons without a factor: the direct solve against the windowed multigrid PCG (pcg_windows=True) on one problem where both
fit, in steady ALM iterations/s (timed windows of the two solvers alternating in one process) and PCG iterations per solve.

    python profiles/tools/long_pcg_bench.py [--mesh torus25k --T 511 --steps 100 --warmup 10 --repeats 3 --cg-tol 1e-8]

Prints one JSON line.  bench.py is unchanged."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MESHES = {"torus25k": ("torus", dict(nu=200, nv=128)), "knot": ("knot", {})}


def window(alm, steps):
    """``steps`` ALM iterations between two device synchronisations: (iterations/s, PCG iterations per solve)."""
    alm.dev.sync()
    cg0 = alm.cg_total
    t0 = time.perf_counter()
    for _ in range(steps):
        alm.iterate()
    alm.dev.sync()
    return steps / (time.perf_counter() - t0), (alm.cg_total - cg0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="torus25k", choices=sorted(MESHES))
    ap.add_argument("--T", type=int, default=511)
    ap.add_argument("--steps", type=int, default=100, help="ALM iterations per timed window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="timed windows per solver, the two solvers alternating")
    ap.add_argument("--cg-tol", type=float, default=1e-8)
    a = ap.parse_args()

    from dots_socp_amd import meshes
    from dots_socp_amd.device import pcg_window_plan
    from dots_socp_amd.socp.solver_socp import AlmSolver

    name, kw = MESHES[a.mesh]
    geom, _ = meshes.example(name, **kw)
    nit = a.warmup + a.repeats * a.steps + 10
    out = dict(mesh=a.mesh, n_time=a.T, windows=len(pcg_window_plan(a.T)), cg_tol=a.cg_tol, steps=a.steps, repeats=a.repeats)
    t0 = time.perf_counter()
    direct = AlmSolver(a.T, geom, nit=nit, tol=1e-12)
    out.update(vertices=int(direct.dev.V), direct_setup_s=round(time.perf_counter() - t0, 3))
    t0 = time.perf_counter()
    pcg = AlmSolver(a.T, geom, nit=nit, tol=1e-12, lap_solver="modal_pcg", pcg_windows=True, cg_tol=a.cg_tol)
    out.update(pcg_setup_s=round(time.perf_counter() - t0, 3), mg_levels=(pcg.mg_summary or {}).get("levels"))
    for alm in (direct, pcg):
        window(alm, a.warmup)
    rates = {"direct": [], "pcg": []}
    per_solve = []
    for _ in range(a.repeats):
        rates["direct"].append(window(direct, a.steps)[0])
        its, n = window(pcg, a.steps)
        rates["pcg"].append(its)
        per_solve.append(n)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    out.update(direct_it_per_s=[round(x, 2) for x in rates["direct"]], pcg_it_per_s=[round(x, 2) for x in rates["pcg"]],
               pcg_iterations_per_solve=[round(x, 2) for x in per_solve], pcg_not_converged=int(pcg.cg_fail),
               pcg_windows_ran=pcg.dev.pcg_windows_ran()[0], direct_over_pcg=round(med(rates["direct"]) / med(rates["pcg"]), 2))
    direct.close()
    pcg.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

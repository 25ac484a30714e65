"""A loop of neighbouring transport problems on one surface, solved four ways: what a solve session (socp.SolveSession: one live
context, dots_restart between the problems) saves against the paths that exist without it.

    python profiles/tools/session_bench.py --mesh torus100k --T 31 --steps 10 [--tol 1e-4] [--nit 3000] > profiles/session/<name>.jsonl

The problems: ``mu0`` is the example's; ``mu1``'s two bumps (``meshes.bump_density``) start at the example's centres and move by one
mesh edge per step, each towards the other one's start.  Every problem is solved by

    fresh_cold        a new solver from zero (what ``solver_socp`` does), nothing downloaded
    fresh_host_warm   a new solver with ``init_solution=`` the twelve arrays of the previous problem's solution (its own chain): the
                      host warm start, twelve arrays down and twelve up
    session_cold      ``SolveSession.solve(warm=False)``
    session_warm      ``SolveSession.solve(warm=True)``: the previous iterate rescaled on the device

One JSON line per solve: wall time of the whole call (set-up, iterations, finalize, and for fresh_host_warm the download that
feeds the next step), iterations, set-up seconds (everything before the first iteration), bytes to and from the host, the restart's
device milliseconds, cost and the largest KKT residual.  A summary line has the means over the steps after the first (the first
builds every context) and the three comparisons: session_cold against fresh_cold, session_warm against fresh_host_warm (same
iterations each; the wall time differs by the set-up, and by the round trip), and warm against cold iterations.  bench.py is
unchanged; this script only reuses its mesh recipes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MESHES = {"knot": ("knot", {}), "torus100k": ("torus", dict(nu=400, nv=250))}
KINDS = ("fresh_cold", "fresh_host_warm", "session_cold", "session_warm")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="knot", choices=sorted(MESHES))
    ap.add_argument("--T", type=int, default=31, choices=(31, 127))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--nit", type=int, default=3000)
    a = ap.parse_args()

    import numpy as np
    import scipy.sparse as sp

    from dots_socp_amd import meshes
    from dots_socp_amd.device import STATE_NAMES
    from dots_socp_amd.socp import SolveSession
    from dots_socp_amd.socp.solver_socp import AlmSolver

    name, kw = MESHES[a.mesh]
    geom, _ = meshes.example(name, **kw)
    v, tri = np.asarray(geom["vertices"]), np.asarray(geom["triangles"])
    V = v.shape[0]
    mesh = {k: val for k, val in geom.items() if k not in ("mu0", "mu1")}
    mu0 = np.asarray(geom["mu0"], dtype=np.float64)
    centres = [int(c) for c in meshes.farthest_vertices(v, 0, 3)[1:3]]      # (as meshes.example places the two bumps of mu1)
    radius, sigma = kw.get("radius", 0.35), kw.get("sigma", 0.05)
    edges = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    adj = sp.csr_matrix((np.ones(2 * edges.shape[0]), (np.r_[edges[:, 0], edges[:, 1]], np.r_[edges[:, 1], edges[:, 0]])), shape=(V, V))
    targets = [v[centres[1]].copy(), v[centres[0]].copy()]

    def step_centres(cs):
        out = []
        for c, target in zip(cs, targets):
            nb = adj.indices[adj.indptr[c]:adj.indptr[c + 1]]
            out.append(int(nb[np.argmin(np.sum((v[nb] - target) ** 2, axis=1))]))
        return out

    base = dict(mesh=a.mesh, n_time=a.T, vertices=int(V), triangles=int(tri.shape[0]), tol=a.tol, nit=a.nit)
    opts = dict(tol=a.tol, nit=a.nit)
    rows = {k: [] for k in KINDS}

    def emit(kind, step, wall, hist, setup, to_host, from_host, restart_ms, iterations):
        out = dict(base, kind=kind, step=step, centres=list(cs), wall_s=round(wall, 6), iterations=int(iterations), setup_s=round(setup, 6),
                   bytes_to_host=int(to_host), bytes_from_host=int(from_host), restart_ms=None if restart_ms is None else round(restart_ms, 4),
                   cost=float(hist.history["Transportation cost"][-1]), kkt_max=float(np.nanmax(np.asarray(hist.kkt_errors[-1], dtype=np.float64))))
        rows[kind].append(out)
        print(json.dumps(out), flush=True)

    def fresh(kind, step, mu1, init):
        t0 = time.perf_counter()
        alm = AlmSolver(a.T, {**mesh, "mu0": mu0, "mu1": mu1}, init_solution=init, **opts)
        try:
            setup = time.perf_counter() - t0
            for _ in range(alm.nit):
                if alm.iterate():
                    break
            solution, hist = alm.finalize(outputs=() if kind == "fresh_cold" else None)
            to_host = alm.dev.debug_counter(9)
        finally:
            alm.close()
        wall = time.perf_counter() - t0
        from_host = 0 if not init else sum(np.asarray(init[k]).nbytes for k in STATE_NAMES)
        emit(kind, step, wall, hist, setup, to_host, from_host, None, alm.counter_main + 1)
        return None if kind == "fresh_cold" else {k: solution[k] for k in STATE_NAMES}

    def in_session(kind, step, s, mu1):
        before = 0 if s.alm is None else s.alm.dev.debug_counter(9)
        t0 = time.perf_counter()
        _, hist = s.solve(mu0, mu1, warm=kind == "session_warm", outputs=())
        wall = time.perf_counter() - t0
        st = hist.solver_stats["session"]
        emit(kind, step, wall, hist, st["setup_seconds"], s.alm.dev.debug_counter(9) - before, 0, st["restart_ms"], s.alm.counter_main + 1)

    cs, previous = list(centres), None
    with SolveSession(a.T, mesh, **opts) as cold, SolveSession(a.T, mesh, **opts) as warm:
        for step in range(a.steps + 1):      # (step 0 builds the sessions' contexts and starts the host chain: not in the means)
            mu1 = meshes.bump_density(v, np.asarray(geom["area_vertices"]), cs, radius, sigma)
            fresh("fresh_cold", step, mu1, None)
            previous = fresh("fresh_host_warm", step, mu1, previous)
            in_session("session_cold", step, cold, mu1)
            in_session("session_warm", step, warm, mu1)
            cs = step_centres(cs)
        restart_kernel_ms, restart_kernel_bytes = warm.alm.dev.bench_kernel(5, reps=10)

    def mean(kind, key):
        vals = [r[key] for r in rows[kind][1:] if r[key] is not None]
        return None if not vals else round(float(np.mean(vals)), 6)

    summary = dict(base, kind="summary", steps=a.steps)
    for kind in KINDS:
        for key in ("wall_s", "iterations", "setup_s", "restart_ms"):
            summary[f"{kind}_{key}"] = mean(kind, key)
        summary[f"{kind}_bytes_to_host"] = rows[kind][-1]["bytes_to_host"]
        summary[f"{kind}_bytes_from_host"] = rows[kind][-1]["bytes_from_host"]
    same = lambda x, y: [r["iterations"] for r in rows[x]] == [r["iterations"] for r in rows[y]]      # noqa: E731
    summary["cold_same_iterations"] = same("session_cold", "fresh_cold")
    summary["warm_same_iterations"] = same("session_warm", "fresh_host_warm")
    summary["cold_same_cost"] = [r["cost"] for r in rows["session_cold"]] == [r["cost"] for r in rows["fresh_cold"]]
    summary["warm_same_cost"] = [r["cost"] for r in rows["session_warm"]] == [r["cost"] for r in rows["fresh_host_warm"]]
    summary["session_cold_wall_saved_s"] = round(summary["fresh_cold_wall_s"] - summary["session_cold_wall_s"], 6)
    summary["session_warm_wall_saved_s"] = round(summary["fresh_host_warm_wall_s"] - summary["session_warm_wall_s"], 6)
    summary["warm_over_cold_iterations"] = round(summary["session_warm_iterations"] / summary["session_cold_iterations"], 4)
    summary["session_warm_over_session_cold_wall"] = round(summary["session_warm_wall_s"] / summary["session_cold_wall_s"], 4)
    summary["restart_kernel_ms"] = round(restart_kernel_ms, 4)
    summary["restart_kernel_TBps"] = round(restart_kernel_bytes / (1e-3 * restart_kernel_ms) / 1e12, 3)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()

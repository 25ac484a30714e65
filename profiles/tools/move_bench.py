"""A loop in which the surface moves a little every step while the end masses stay, solved four ways: what moving the vertices of a
live context (SolveSession.solve(vertices=): dots_move_vertices + dots_restart) saves against the paths that exist without it.

    python profiles/tools/move_bench.py --mesh torus100k --T 31 --steps 10 [--tol 1e-4] [--nit 3000] > profiles/move/<name>.jsonl

Step k displaces the example's vertices by the smooth field ``(sin(2 pi y + 0.3), sin(2 pi z + 0.7) cos(2 pi x), sin(2 pi x + 1.1))`` of
the coordinates scaled to the unit box, at amplitude 0.002 k of the box's longest side.  Every step is solved by

    fresh_cold        a new ``AlmSolver`` on the moved mesh from zero: new plan, tree, symbolic analysis, context and factor
    fresh_host_warm   the same with ``init_solution=`` the twelve arrays of the previous step's solution (its own chain): twelve
                      arrays down and twelve up
    session_cold      ``SolveSession.solve(warm=False, vertices=)``: tables and factor refreshed on the live context
    session_warm      ``SolveSession.solve(warm=True, vertices=)``: and the previous iterate rescaled on the device

The four alternate in one process, after one warm-up step each (step 0, at amplitude 0: it builds the sessions' contexts and starts
the host chain; it is not in the means).  One JSON line per solve: wall time of the whole call, iterations, set-up seconds (everything
before the first iteration), bytes to and from the host, the move's device milliseconds (assembly launches, factor refresh, whole
call), the restart's, cost and the largest KKT residual.  The summary line has the means over the steps after the first and the two
comparisons: session_cold against fresh_cold, session_warm against fresh_host_warm.  A new solver numbers the moved mesh itself, so
the fresh and the session runs are the same problem in two numberings, not the same bits.  bench.py is unchanged; this script only
reuses its mesh recipes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MESHES = {"knot": ("knot", {}), "torus100k": ("torus", dict(nu=400, nv=250))}
KINDS = ("fresh_cold", "fresh_host_warm", "session_cold", "session_warm")
AMPLITUDE_PER_STEP = 0.002


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="knot", choices=sorted(MESHES))
    ap.add_argument("--T", type=int, default=31)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--nit", type=int, default=3000)
    a = ap.parse_args()

    import numpy as np

    from dots_socp_amd import meshes
    from dots_socp_amd.device import STATE_NAMES
    from dots_socp_amd.socp import SolveSession
    from dots_socp_amd.socp.solver_socp import AlmSolver

    name, kw = MESHES[a.mesh]
    geom, _ = meshes.example(name, **kw)
    v0, tri = np.asarray(geom["vertices"], dtype=np.float64), np.asarray(geom["triangles"])
    V = v0.shape[0]
    mesh = {k: val for k, val in geom.items() if k not in ("mu0", "mu1")}
    mu0, mu1 = np.asarray(geom["mu0"], dtype=np.float64), np.asarray(geom["mu1"], dtype=np.float64)
    lo, side = v0.min(axis=0), float(np.max(v0.max(axis=0) - v0.min(axis=0)))

    def displaced(k):
        u = (v0 - lo) / side
        x, y, z = u[:, 0], u[:, 1], u[:, 2]
        w = 2.0 * np.pi
        field = np.stack([np.sin(w * y + 0.3), np.sin(w * z + 0.7) * np.cos(w * x), np.sin(w * x + 1.1)], axis=1)
        return v0 + (AMPLITUDE_PER_STEP * k * side) * field

    def mesh_at(x):
        area_t = meshes.triangle_areas(x, tri)
        return {**mesh, "vertices": x, "area_triangles": area_t, "area_vertices": meshes.vertex_areas(V, tri, area_t)}

    base = dict(mesh=a.mesh, n_time=a.T, vertices=int(V), triangles=int(tri.shape[0]), tol=a.tol, nit=a.nit)
    opts = dict(tol=a.tol, nit=a.nit)
    rows = {k: [] for k in KINDS}

    def emit(kind, step, wall, hist, setup, to_host, from_host, restart_ms, move_ms, iterations):
        out = dict(base, kind=kind, step=step, amplitude=AMPLITUDE_PER_STEP * step, wall_s=round(wall, 6), iterations=int(iterations), setup_s=round(setup, 6),
                   bytes_to_host=int(to_host), bytes_from_host=int(from_host), restart_ms=None if restart_ms is None else round(restart_ms, 4),
                   move_assembly_ms=None if move_ms is None else round(move_ms[0], 4), move_factor_ms=None if move_ms is None else round(move_ms[1], 4),
                   move_ms=None if move_ms is None else round(move_ms[2], 4),
                   cost=float(hist.history["Transportation cost"][-1]), kkt_max=float(np.nanmax(np.asarray(hist.kkt_errors[-1], dtype=np.float64))))
        rows[kind].append(out)
        print(json.dumps(out), flush=True)

    def fresh(kind, step, x, init):
        t0 = time.perf_counter()
        alm = AlmSolver(a.T, {**mesh_at(x), "mu0": mu0, "mu1": mu1}, init_solution=init, **opts)
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
        emit(kind, step, wall, hist, setup, to_host, from_host + x.nbytes, None, None, alm.counter_main + 1)
        return None if kind == "fresh_cold" else {k: solution[k] for k in STATE_NAMES}

    def in_session(kind, step, s, x):
        before = 0 if s.alm is None else s.alm.dev.debug_counter(9)
        t0 = time.perf_counter()
        _, hist = s.solve(mu0, mu1, warm=kind == "session_warm", outputs=(), vertices=x)
        wall = time.perf_counter() - t0
        st = hist.solver_stats["session"]
        emit(kind, step, wall, hist, st["setup_seconds"], s.alm.dev.debug_counter(9) - before, x.nbytes, st["restart_ms"], st["move_ms"], s.alm.counter_main + 1)

    previous = None
    with SolveSession(a.T, mesh, **opts) as cold, SolveSession(a.T, mesh, **opts) as warm:
        for step in range(a.steps + 1):
            x = displaced(step)
            fresh("fresh_cold", step, x, None)
            previous = fresh("fresh_host_warm", step, x, previous)
            in_session("session_cold", step, cold, x)
            in_session("session_warm", step, warm, x)

    def mean(kind, key):
        vals = [r[key] for r in rows[kind][1:] if r[key] is not None]
        return None if not vals else round(float(np.mean(vals)), 6)

    summary = dict(base, kind="summary", steps=a.steps)
    for kind in KINDS:
        for key in ("wall_s", "iterations", "setup_s", "restart_ms", "move_assembly_ms", "move_factor_ms", "move_ms"):
            summary[f"{kind}_{key}"] = mean(kind, key)
        summary[f"{kind}_bytes_to_host"] = rows[kind][-1]["bytes_to_host"]
        summary[f"{kind}_bytes_from_host"] = rows[kind][-1]["bytes_from_host"]
    summary["session_cold_wall_saved_s"] = round(summary["fresh_cold_wall_s"] - summary["session_cold_wall_s"], 6)
    summary["session_warm_wall_saved_s"] = round(summary["fresh_host_warm_wall_s"] - summary["session_warm_wall_s"], 6)
    summary["session_cold_over_fresh_cold_wall"] = round(summary["session_cold_wall_s"] / summary["fresh_cold_wall_s"], 4)
    summary["session_warm_over_fresh_host_warm_wall"] = round(summary["session_warm_wall_s"] / summary["fresh_host_warm_wall_s"], 4)
    summary["warm_over_cold_iterations"] = round(summary["session_warm_iterations"] / summary["session_cold_iterations"], 4)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()

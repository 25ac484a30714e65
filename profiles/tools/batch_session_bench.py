"""A loop over a minibatch of four neighbouring transport problems on one surface, solved four ways: what a batch session
(socp.BatchSession: live contexts on one shared factor, dots_restart and dots_move_vertices_many) saves against the paths that exist
without it.

    python profiles/tools/batch_session_bench.py --mesh torus100k --series masses --steps 10 > profiles/batch_session/<name>.jsonl
    python profiles/tools/batch_session_bench.py --mesh torus100k --series move --steps 10 > profiles/batch_session/<name>.jsonl

The problems: ``mu0`` is the example's; problem j's ``mu1`` is one bump (``meshes.bump_density``) at the j-th of four vertices far from
each other.  ``--series masses``: every step moves every centre by one mesh edge towards the next problem's first centre, on a fixed
surface.  ``--series move``: the masses stay and step k displaces the vertices by the smooth field of move_bench.py at amplitude
0.002 k of the box's longest side.  Every step is solved by

    many           ``solver_socp_many`` anew: plan, tree, factor and four contexts (three repetitions a step: their spread is the
                   run-to-run noise the other differences are read against)
    sessions_warm  four ``SolveSession`` s, one per problem, solved one after the other, warm
    batch_cold     ``BatchSession.solve_many(warm=False)``: cold restarts on the live contexts, batched sweeps
    batch_warm     ``BatchSession.solve_many(warm=True)``: each slot from its last iterate

alternating in one process, whole calls, after one warm-up step (step 0: it builds the contexts; not in the means).  One JSON line per
call: wall time, the iterations of each problem, bytes to the host (dots_debug_counter 9 of every context the call used) and, in the move
series, the device milliseconds of the move (assembly launches, factor refresh, whole call; summed over the four sessions for
sessions_warm).  The summary line has the means, the spread of ``many`` and two identities that must hold exactly on a fixed surface:
the iterations of batch_cold are those of many, the iterations of batch_warm those of sessions_warm (in the move series ``many``
numbers the moved mesh itself: the same problem in another numbering, not the same bits).  bench.py is unchanged; this script only
reuses its mesh recipes."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MESHES = {"knot": ("knot", {}), "torus100k": ("torus", dict(nu=400, nv=250))}
KINDS = ("many", "sessions_warm", "batch_cold", "batch_warm")
AMPLITUDE_PER_STEP = 0.002
N_PROBLEMS = 4
MANY_REPEATS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="knot", choices=sorted(MESHES))
    ap.add_argument("--series", default="masses", choices=("masses", "move"))
    ap.add_argument("--T", type=int, default=31)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--nit", type=int, default=3000)
    a = ap.parse_args()

    import numpy as np
    import scipy.sparse as sp

    from dots_socp_amd import meshes
    from dots_socp_amd.socp import BatchSession, SolveSession, solver_socp_many

    ss = importlib.import_module("dots_socp_amd.socp.solver_socp")
    name, kw = MESHES[a.mesh]
    geom, _ = meshes.example(name, **kw)
    v0, tri = np.asarray(geom["vertices"], dtype=np.float64), np.asarray(geom["triangles"])
    V = v0.shape[0]
    mesh = {k: val for k, val in geom.items() if k not in ("mu0", "mu1")}
    mu0 = np.asarray(geom["mu0"], dtype=np.float64)
    radius, sigma = kw.get("radius", 0.35), kw.get("sigma", 0.05)
    centres = [int(c) for c in meshes.farthest_vertices(v0, 0, N_PROBLEMS + 1)[1:]]
    targets = [v0[centres[(j + 1) % N_PROBLEMS]].copy() for j in range(N_PROBLEMS)]
    edges = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    adj = sp.csr_matrix((np.ones(2 * edges.shape[0]), (np.r_[edges[:, 0], edges[:, 1]], np.r_[edges[:, 1], edges[:, 0]])), shape=(V, V))
    lo, side = v0.min(axis=0), float(np.max(v0.max(axis=0) - v0.min(axis=0)))

    def step_centres(cs):
        out = []
        for c, target in zip(cs, targets):
            nb = adj.indices[adj.indptr[c]:adj.indptr[c + 1]]
            out.append(int(nb[np.argmin(np.sum((v0[nb] - target) ** 2, axis=1))]))
        return out

    def displaced(k):
        u = (v0 - lo) / side
        x, y, z = u[:, 0], u[:, 1], u[:, 2]
        w = 2.0 * np.pi
        field = np.stack([np.sin(w * y + 0.3), np.sin(w * z + 0.7) * np.cos(w * x), np.sin(w * x + 1.1)], axis=1)
        return v0 + (AMPLITUDE_PER_STEP * k * side) * field

    def mesh_at(x):
        area_t = meshes.triangle_areas(x, tri)
        return {**mesh, "vertices": x, "area_triangles": area_t, "area_vertices": meshes.vertex_areas(V, tri, area_t)}

    # bytes to the host of contexts that a call closes itself (solver_socp_many): read as they close
    closed_bytes = [0]
    close = ss.AlmSolver.close

    def counting_close(self):
        if not getattr(self, "closed", False):
            closed_bytes[0] += self.dev.debug_counter(9)
        close(self)

    ss.AlmSolver.close = counting_close

    base = dict(mesh=a.mesh, series=a.series, n_time=a.T, vertices=int(V), triangles=int(tri.shape[0]), tol=a.tol, nit=a.nit, problems=N_PROBLEMS)
    opts = dict(tol=a.tol, nit=a.nit)
    rows = {k: [] for k in KINDS}

    def emit(kind, step, wall, hists, to_host, move_ms, repeat=0):
        out = dict(base, kind=kind, step=step, repeat=repeat, wall_s=round(wall, 6), iterations=[int(h.kkt_iteration[-1]) + 1 for h in hists],
                   bytes_to_host=int(to_host), move_assembly_ms=None if move_ms is None else round(move_ms[0], 4),
                   move_factor_ms=None if move_ms is None else round(move_ms[1], 4), move_ms=None if move_ms is None else round(move_ms[2], 4),
                   cost=[float(h.history["Transportation cost"][-1]) for h in hists])
        rows[kind].append(out)
        print(json.dumps(out), flush=True)

    def live_bytes(solvers):
        return sum(s.dev.debug_counter(9) for s in solvers if s is not None)

    def many(step, x, problems, repeat):
        closed_bytes[0] = 0
        t0 = time.perf_counter()
        results = solver_socp_many(a.T, mesh_at(x) if moving else mesh, problems, max_batch=N_PROBLEMS, outputs=())
        emit("many", step, time.perf_counter() - t0, [h for _, h in results], closed_bytes[0], None, repeat)

    def sessions_warm(step, sessions, x, problems):
        before = live_bytes([s.alm for s in sessions])
        t0 = time.perf_counter()
        hists = [s.solve(p["mu0"], p["mu1"], warm=True, outputs=(), vertices=x if moving and step > 0 else None)[1] for s, p in zip(sessions, problems)]
        wall = time.perf_counter() - t0
        moves = [h.solver_stats["session"]["move_ms"] for h in hists]
        move_ms = None if moves[0] is None else tuple(float(sum(m[i] for m in moves)) for i in range(3))
        emit("sessions_warm", step, wall, hists, live_bytes([s.alm for s in sessions]) - before, move_ms)

    def batch(kind, step, bs, x, problems):
        before = live_bytes(bs.solvers)
        t0 = time.perf_counter()
        results = bs.solve_many(problems, warm=kind == "batch_warm" and step > 0, outputs=(), vertices=x if moving and step > 0 else None)
        wall = time.perf_counter() - t0
        emit(kind, step, wall, [h for _, h in results], live_bytes(bs.solvers) - before, results[0][1].solver_stats["session"]["move_ms"])

    moving = a.series == "move"
    cs = list(centres)
    sessions = [SolveSession(a.T, mesh, **opts) for _ in range(N_PROBLEMS)]
    try:
        with BatchSession(a.T, mesh, max_batch=N_PROBLEMS) as cold, BatchSession(a.T, mesh, max_batch=N_PROBLEMS) as warm:
            for step in range(a.steps + 1):
                x = displaced(step) if moving else v0
                problems = [dict(mu0=mu0, mu1=meshes.bump_density(v0, np.asarray(geom["area_vertices"]), [c], radius, sigma), **opts) for c in cs]
                for repeat in range(MANY_REPEATS if step > 0 else 1):
                    many(step, x, problems, repeat)
                sessions_warm(step, sessions, x, problems)
                batch("batch_cold", step, cold, x, problems)
                batch("batch_warm", step, warm, x, problems)
                if not moving:
                    cs = step_centres(cs)
    finally:
        for s in sessions:
            s.close()

    def mean(kind, key, repeat=None):
        vals = [r[key] for r in rows[kind] if r["step"] > 0 and r[key] is not None and (repeat is None or r["repeat"] == repeat)]
        return None if not vals else round(float(np.mean(vals)), 6)

    summary = dict(base, kind="summary", steps=a.steps)
    for kind in KINDS:
        for key in ("wall_s", "move_assembly_ms", "move_factor_ms", "move_ms"):
            summary[f"{kind}_{key}"] = mean(kind, key)
        its = [sum(r["iterations"]) for r in rows[kind] if r["step"] > 0 and r["repeat"] == 0]
        summary[f"{kind}_iterations_per_step"] = round(float(np.mean(its)), 3) if its else None
        summary[f"{kind}_bytes_to_host_per_step"] = mean(kind, "bytes_to_host")
    per_repeat = [mean("many", "wall_s", r) for r in range(MANY_REPEATS)]
    summary["many_wall_s_by_repeat"] = per_repeat
    summary["many_wall_s_spread"] = None if None in per_repeat else round(max(per_repeat) - min(per_repeat), 6)

    def iterations(kind):
        return [r["iterations"] for r in rows[kind] if r["repeat"] == 0]

    summary["batch_cold_iterations_equal_many"] = iterations("batch_cold") == iterations("many")
    summary["batch_warm_iterations_equal_sessions_warm"] = iterations("batch_warm") == iterations("sessions_warm")
    for kind in ("batch_cold", "batch_warm"):
        other = "many" if kind == "batch_cold" else "sessions_warm"
        if summary[f"{kind}_wall_s"] and summary[f"{other}_wall_s"]:
            summary[f"{kind}_wall_saved_s"] = round(summary[f"{other}_wall_s"] - summary[f"{kind}_wall_s"], 6)
            summary[f"{kind}_over_{other}_wall"] = round(summary[f"{kind}_wall_s"] / summary[f"{other}_wall_s"], 4)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()

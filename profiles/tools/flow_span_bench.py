"""The trace between two time nodes at the end of a solve (dots_flow_trace): what backward costs beside forward on the same
particles, and what the action and the push add.

    python profiles/tools/flow_span_bench.py --mesh torus100k --T 31 [--nit 100] [--tol 1e-4] [--reps 3] [--starts vertices,1]

The state is what ``--nit`` ALM iterations leave.  Starts: one particle per vertex, and ``level^2`` per triangle (flow.triangle_starts)
for the levels given; the mass is that of mu0 forward and of mu1 backward (flow.start_masses).  For every choice of starts one JSON
line per (direction, action, push), device milliseconds, best of ``--reps``:

- ``direction``: "map" (dots_flow_map / dots_flow_push over the whole horizon, the kernels without a span), "forward" (0, T),
  "backward" (T, 0), "first_half" (0, T // 2) and "back_half" (T, T // 2) through dots_flow_trace;
- ``action``: whether the action is returned (the span kernels always form it: this is the copy of one double per particle);
- ``push``: None, "end" or "all" (mass alone);
- ``ms``, ``bytes``, and ``rested`` / ``stopped`` particles; with the action ``action_sum`` = sum(mass * action).

Nothing is gated on it.  bench.py is unchanged; this script only reuses its mesh recipes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MESHES = {"plane": ("plane", dict(n=20)), "knot": ("knot", {}), "torus100k": ("torus", dict(nu=400, nv=250)), "sphere10k": ("sphere", dict(level=5))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="knot", choices=sorted(MESHES))
    ap.add_argument("--T", type=int, default=31)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--nit", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--starts", default="vertices,1")
    a = ap.parse_args()

    import numpy as np

    from dots_socp_amd import flow, meshes
    from dots_socp_amd.socp import _geometry_with_areas
    from dots_socp_amd.socp.solver_socp import AlmSolver

    name, kw = MESHES[a.mesh]
    geom, _ = meshes.example(name, **kw)
    g = _geometry_with_areas(geom)
    vertices, triangles = np.asarray(geom["vertices"], dtype=np.float64), np.asarray(geom["triangles"]).astype(np.int64)
    V, F, T = vertices.shape[0], triangles.shape[0], a.T
    base = dict(mesh=a.mesh, n_time=T, vertices=int(V), triangles=int(F), nit=a.nit)
    spans = {"map": None, "forward": (0, T), "backward": (T, 0), "first_half": (0, T // 2), "back_half": (T, T // 2)}
    alm = AlmSolver(T, geom, tol=a.tol, nit=a.nit, time_limit=1e9)
    try:
        for _ in range(a.nit):
            if alm.iterate():
                break
        alm.dev.sync()
        for choice in a.starts.split(","):
            level = None if choice == "vertices" else int(choice)
            tri, w = flow.vertex_starts(triangles, V) if level is None else flow.triangle_starts(triangles, level)
            masses = {m: flow.start_masses(g[m], g["area_vertices"], g["area_triangles"], triangles, tri, w, level) for m in ("mu0", "mu1")}
            for direction, span in spans.items():
                mass = masses["mu1" if span is not None and span[0] == T else "mu0"]
                for action in ((False,) if span is None else (False, True)):
                    for push in (None, "end", "all"):
                        request = dict(starts=(tri, w), span=span, action=action, push=None if push is None else {"mass": mass, "layers": push})
                        out = min((alm.flow_map(**request) for _ in range(a.reps)), key=lambda r: r["ms"])
                        rec = dict(base, kind="flow_span", starts=choice, particles=int(tri.shape[0]), direction=direction, span=span, action=action,
                                   push=push, ms=round(out["ms"], 4), bytes=int(out["bytes"]), rested=int(np.sum(out["rested"] > 0)),
                                   stopped=int(np.sum(out["status"] == 1)))
                        if action:
                            rec["action_sum"] = float(np.sum(mass * out["action"]))
                        print(json.dumps(rec), flush=True)
    finally:
        alm.close()


if __name__ == "__main__":
    main()

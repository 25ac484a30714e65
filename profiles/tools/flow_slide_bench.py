"""The sliding mode of the flow map (dots_flow_slide) beside dots_flow_trace on the same particles in the same process: what the slides
cost, how much mass still rests, and how far the pushed measure is from the target with and without them.

    python profiles/tools/flow_slide_bench.py --mesh torus100k --T 31 [--nit 100,1500] [--tol 1e-4] [--reps 3] [--starts vertices,1,2]

The state is what ``--nit`` ALM iterations leave (several counts: the same solver goes on to the next).  Starts: one particle per
vertex, and ``level^2`` per triangle (flow.triangle_starts) for the levels given; the mass is that of mu0 forward and of mu1
backward (flow.start_masses).  For every state, choice of starts and direction -- "forward" (0, T) and "backward" (T, 0) -- one JSON
line per ``slide`` (false: dots_flow_trace, true: dots_flow_slide), each with the action and the push of the last layer:

- ``ms``: device milliseconds, best of ``--reps``, and ``ms_all``: every repetition (the spread a difference has to stand out of);
- ``rested`` / ``stopped`` / ``slid``: particles; ``rested_mass`` / ``stopped_mass`` / ``slid_mass``: what they carry;
- ``to_mu1`` (forward) or ``to_mu0`` (backward): relative L1 distance of the pushed measure from the target;
- ``steps_sum`` / ``steps_max``: the turns of the inner loop over all the particles and of the slowest one.  dots_flow_trace does
  not count them: for ``slide`` false they come from ``crossings + intervals traversed`` (a particle that never stops takes one turn
  more than it crosses in every interval, a rest included), which is exact for the particles that did not stop and is given for
  those alone (``steps_of`` names how many).

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
    ap.add_argument("--nit", default="100")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--starts", default="vertices,1,2")
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
    counts = sorted(int(x) for x in a.nit.split(","))
    alm = AlmSolver(T, geom, tol=a.tol, nit=counts[-1], time_limit=1e9)
    try:
        done, stopped_early = 0, False
        for nit in counts:
            while done < nit and not stopped_early:
                stopped_early = bool(alm.iterate())
                done += 1
            alm.dev.sync()
            base = dict(mesh=a.mesh, n_time=T, vertices=int(V), triangles=int(F), nit=nit, iterations=done, kind="flow_slide")
            for choice in a.starts.split(","):
                level = None if choice == "vertices" else int(choice)
                tri, w = flow.vertex_starts(triangles, V) if level is None else flow.triangle_starts(triangles, level)
                masses = {m: flow.start_masses(g[m], g["area_vertices"], g["area_triangles"], triangles, tri, w, level) for m in ("mu0", "mu1")}
                for direction, span in (("forward", (0, T)), ("backward", (T, 0))):
                    mass = masses["mu0" if span[0] == 0 else "mu1"]
                    for slide in (False, True):
                        request = dict(starts=(tri, w), span=span, action=True, push={"mass": mass, "layers": "end"}, slide=slide)
                        runs = [alm.flow_map(**request) for _ in range(a.reps)]
                        out = min(runs, key=lambda r: r["ms"])
                        pushed = out["pushed"]
                        target = "to_mu1" if span[1] == T else "to_mu0"
                        rec = dict(base, starts=choice, particles=int(tri.shape[0]), direction=direction, slide=slide, ms=round(out["ms"], 4),
                                   ms_all=[round(r["ms"], 4) for r in runs], bytes=int(out["bytes"]), rested=int(np.sum(out["rested"] > 0)),
                                   rested_intervals=int(np.sum(out["rested"])), stopped=int(np.sum(out["status"] == 1)),
                                   rested_mass=pushed["rested_mass"], stopped_mass=pushed["stopped_mass"], total_mass=float(np.sum(mass)),
                                   action_sum=float(np.sum(mass * out["action"])))
                        rec[target] = float(pushed[target]["l1"])
                        if slide:
                            rec.update(slid=int(np.sum(out["slides"] > 0)), slides=int(np.sum(out["slides"])), slid_mass=pushed["slid_mass"],
                                       steps_sum=int(np.sum(out["steps"], dtype=np.int64)), steps_max=int(np.max(out["steps"])), steps_of=int(tri.shape[0]))
                        else:
                            on = out["status"] == 0
                            steps = out["crossings"][on].astype(np.int64) + T
                            rec.update(steps_sum=int(steps.sum()), steps_max=int(steps.max()) if steps.size else 0, steps_of=int(on.sum()))
                        print(json.dumps(rec), flush=True)
            if stopped_early:
                break
    finally:
        alm.close()


if __name__ == "__main__":
    main()

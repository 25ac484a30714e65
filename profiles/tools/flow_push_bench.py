"""The push-forward at the end of a solve (dots_flow_push): what the deposit costs beside the trace, and the whole call against the
path it replaces -- ``trajectory=True`` (or the end points alone for the last layer) plus ``np.add.at`` on the host.

    python profiles/tools/flow_push_bench.py --mesh torus100k --T 31 [--nit 100] [--tol 1e-4] [--reps 3] [--starts vertices,1,2]

The state is what ``--nit`` ALM iterations leave.  Starts: one particle per vertex, and ``level^2`` per triangle (flow.triangle_starts)
for the levels given; the mass is that of mu0 (flow.start_masses), the three attributes are the start coordinates.  For every
(starts, layers, attributes) one JSON line:

- ``push_ms`` / ``map_ms``: device milliseconds of dots_flow_push (zeroing, trace with deposits, conversion) and of dots_flow_map on
  the same particles, best of ``--reps``; ``deposit_ms`` their difference;
- ``issued``: the non-zero contributions (one 64-bit atomic each, counted on the host from the trajectory with the operations of the
  specification), ``deposit_gb_s``: 8 bytes each over ``deposit_ms``;
- ``push_wall_s`` / ``push_bytes``: the whole call and the bytes it copies to the host; ``host_wall_s`` / ``host_bytes``: the same
  sums through the trace's outputs and ``np.add.at`` (the call with the layers it needs, plus the scatter), ``host_scatter_s`` the
  scatter alone; ``max_difference``: the largest difference between the two results;
- ``rested_mass``, ``stopped_mass``, ``to_mu1``: of the pushed measure (``to_mu1``: its last layer against mu1).

bench.py is unchanged; this script only reuses its mesh recipes."""
import argparse
import json
import math
import os
import sys
import time

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
    base = dict(mesh=a.mesh, n_time=T, vertices=int(V), triangles=int(F), nit=a.nit)
    alm = AlmSolver(T, geom, tol=a.tol, nit=a.nit, time_limit=1e9)
    try:
        for _ in range(a.nit):
            if alm.iterate():
                break
        alm.dev.sync()
        for choice in a.starts.split(","):
            level = None if choice == "vertices" else int(choice)
            starts = "vertices" if level is None else ("triangles", level)
            tri, w = flow.vertex_starts(triangles, V) if level is None else flow.triangle_starts(triangles, level)
            P = tri.shape[0]
            mass = flow.start_masses(g["mu0"], g["area_vertices"], g["area_triangles"], triangles, tri, w, level)
            where = flow.positions(vertices, triangles, tri, w)
            map_ms = min(alm.flow_map(starts=(tri, w))["ms"] for _ in range(a.reps))
            # the path this replaces, once per choice of starts: the trajectory to the host ...
            t0 = time.perf_counter()
            traj = alm.flow_map(starts=(tri, w), trajectory=True)
            traj_wall, traj_bytes = time.perf_counter() - t0, int(traj["bytes"])
            t0 = time.perf_counter()
            ends = alm.flow_map(starts=(tri, w))
            ends_wall, ends_bytes = time.perf_counter() - t0, int(ends["bytes"])
            vert_at = triangles[traj["triangles_at"]]      # (T + 1, P, 3)
            for n_attr in (0, 3):
                attributes = np.ascontiguousarray(where.T) if n_attr else None
                carried = np.concatenate([mass[None, :]] + ([mass[None, :] * attributes] if n_attr else []), axis=0)
                for layers in ("end", "all"):
                    best = None
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        out = alm.flow_map(starts=(tri, w), push={"mass": mass, "attributes": attributes, "layers": layers})
                        wall = time.perf_counter() - t0
                        if best is None or out["ms"] < best[0]["ms"]:
                            best = (out, wall)
                    out, wall = best
                    pushed = out["pushed"]
                    first = 0 if layers == "all" else T
                    L = T + 1 - first
                    # ... and np.add.at over the layers asked for
                    t0 = time.perf_counter()
                    host = np.zeros((1 + n_attr, L, V))
                    for c in range(1 + n_attr):
                        for l in range(L):
                            np.add.at(host[c, l], vert_at[first + l].reshape(-1), (carried[c][:, None] * traj["weights_at"][first + l]).reshape(-1))
                    scatter = time.perf_counter() - t0
                    issued = 0
                    for c in range(1 + n_attr):
                        scale = math.ldexp(1.0, int(pushed["exponents"][c]))
                        for l in range(L):
                            issued += int(np.count_nonzero(np.rint((carried[c][:, None] * traj["weights_at"][first + l]) * scale)))
                    both = np.concatenate([pushed["mass"][None]] + ([pushed["attributes"]] if n_attr else []), axis=0)
                    deposit_ms = out["ms"] - map_ms
                    rec = dict(base, kind="flow_push", starts=choice, particles=int(P), layers=layers, attributes=n_attr,
                               push_ms=round(out["ms"], 4), map_ms=round(map_ms, 4), deposit_ms=round(deposit_ms, 4), issued=issued,
                               deposit_gb_s=round(8e-9 * issued / (1e-3 * deposit_ms), 1) if deposit_ms > 0 else None,
                               push_wall_s=round(wall, 5), push_bytes=int(out["bytes"]),
                               host_wall_s=round((traj_wall if layers == "all" else ends_wall) + scatter, 5), host_scatter_s=round(scatter, 5),
                               host_bytes=traj_bytes if layers == "all" else ends_bytes, max_difference=float(np.max(np.abs(both - host))),
                               dropped=int(pushed["dropped"]), exponents=[int(k) for k in pushed["exponents"]],
                               rested_mass=pushed["rested_mass"], stopped_mass=pushed["stopped_mass"], total_mass=float(mass.sum()),
                               rested_particles=int(np.sum(out["rested"] > 0)), to_mu1={k: round(v, 6) for k, v in pushed["to_mu1"].items()},
                               layer_sum_error=float(np.max(np.abs(pushed["mass"].sum(axis=1) - mass.sum()))))
                    print(json.dumps(rec), flush=True)
    finally:
        alm.close()


if __name__ == "__main__":
    main()

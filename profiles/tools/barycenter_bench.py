"""The barycentre of K bumps on one surface, iterated two ways: what the device loop (socp.barycenter: dots_barycenter_update, restarts
from device masses in the contexts' numbering) saves against the same mirror descent written over ``torch_cost.transport_costs(session=bs)``
with the update in torch.

    python profiles/tools/barycenter_bench.py --mesh knot --T 31 --K 3 > profiles/barycenter/<name>.jsonl
    python profiles/tools/barycenter_bench.py --mesh torus100k --T 31 --K 3 > profiles/barycenter/<name>.jsonl

The measures: one bump (``meshes.bump_density``) at each of K vertices far from each other, equal weights, the default start.  Both
loops take ``--steps`` outer steps with the same ``--eta`` and the same rule (eta halved after a step whose objective rose), each as a
whole call that builds its own batch session; they alternate in one process, ``--reps`` times, after one discarded call of each.  One
JSON line per call: wall time, seconds per outer step with and without step 0 (which builds plan, factor and contexts), the objective,
eta and inner iterations per step, and bytes to the host per step (dots_debug_counter 9 of the session's contexts; the torch loop also
moves the masses and gradients through torch, which that counter does not see: 2 V doubles per problem and restart are copied to the
host by ``DeviceProblem.restart``, and V per problem come back as the gradient).  The summary line has the means.  bench.py is
unchanged; this script only reuses its mesh recipes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MESHES = {"knot": ("knot", {}), "torus100k": ("torus", dict(nu=400, nv=250))}
KINDS = ("device", "torch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="knot", choices=sorted(MESHES))
    ap.add_argument("--T", type=int, default=31)
    ap.add_argument("--K", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--eta", type=float, default=100.0)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--nit", type=int, default=3000)
    a = ap.parse_args()

    import numpy as np
    import torch

    from dots_socp_amd import barycenter as bary
    from dots_socp_amd import meshes, socp, torch_cost

    name, kw = MESHES[a.mesh]
    geom, _ = meshes.example(name, **kw)
    v0, tri = np.asarray(geom["vertices"], dtype=np.float64), np.asarray(geom["triangles"])
    V = v0.shape[0]
    mesh = {k: val for k, val in geom.items() if k not in ("mu0", "mu1")}
    area = np.asarray(geom["area_vertices"], dtype=np.float64)
    centres = [int(c) for c in meshes.farthest_vertices(v0, 0, a.K)]
    measures = np.stack([meshes.bump_density(v0, area, [c], 0.35, 0.05) for c in centres])
    weights = np.full(a.K, 1.0 / a.K)
    mass = float(measures[0].sum())
    start = bary.default_start(measures, weights, area, mass)
    base = dict(mesh=a.mesh, n_time=a.T, vertices=int(V), triangles=int(tri.shape[0]), K=a.K, steps=a.steps, eta=a.eta, tol=a.tol, nit=a.nit)
    rows = {k: [] for k in KINDS}

    def emit(kind, rep, wall, per_step, objective, etas, iterations, to_host):
        later = per_step[1:]
        out = dict(base, kind=kind, repeat=rep, wall_s=round(wall, 6), step_s=[round(t, 6) for t in per_step],
                   s_per_step_after_0=round(float(np.mean(later)), 6) if later else None, objective=objective, eta_per_step=etas,
                   iterations=iterations, iterations_total=int(sum(iterations)), bytes_to_host=to_host,
                   bytes_to_host_per_step_after_0=round(float(np.mean(to_host[1:])), 1) if len(to_host) > 1 else None)
        if rep >= 0:
            rows[kind].append(out)
        print(json.dumps(out), flush=True)

    def device_loop(rep):
        t0 = time.perf_counter()
        r = socp.barycenter(a.T, mesh, measures, weights, steps=a.steps, eta=a.eta, tol=a.tol, nit=a.nit, to_device=True)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        st = r["solver_stats"]
        emit("device", rep, wall, st["step_seconds"], r["objective"], r["eta"], r["iterations"], st["bytes_to_host"])
        return r["nu"].cpu().numpy()

    def torch_loop(rep):
        t0 = time.perf_counter()
        where = torch.device("cuda", 0)
        rule = bary.StepRule(a.eta)
        nu = torch.tensor(start, dtype=torch.float64, device=where)
        mus = torch.tensor(measures, dtype=torch.float64, device=where)
        w = torch.tensor(weights, dtype=torch.float64, device=where)
        x = torch.tensor(v0, dtype=torch.float64)
        per_step, objective, etas, iterations, to_host = [], [], [], [], []
        with socp.BatchSession(a.T, mesh, max_batch=a.K, slots=a.K) as bs:
            for step in range(a.steps):
                t1 = time.perf_counter()
                before = sum(s.dev.debug_counter(9) for s in bs.solvers if s is not None)
                nu_in = nu.clone().requires_grad_(True)
                costs = torch_cost.transport_costs(nu_in.unsqueeze(0).expand(a.K, V), mus, x, tri, a.T, session=bs, warm=step > 0, tol=a.tol, nit=a.nit)
                total = (w * costs).sum()
                total.backward()
                eta = rule.take(float(total))
                y = nu * torch.exp(-eta * nu_in.grad)
                nu = y * (mass / y.sum())
                torch.cuda.synchronize()
                objective.append(float(total))
                etas.append(eta)
                iterations.append(int(sum(s.counter_main + 1 for s in bs.solvers)))
                to_host.append(int(sum(s.dev.debug_counter(9) for s in bs.solvers) - before))
                per_step.append(time.perf_counter() - t1)
        emit("torch", rep, time.perf_counter() - t0, per_step, objective, etas, iterations, to_host)
        return nu.cpu().numpy()

    device_loop(-1)      # discarded: the first call of a process loads the library and the kernels
    torch_loop(-1)
    ends = {}
    for rep in range(a.reps):
        ends["device"] = device_loop(rep)
        ends["torch"] = torch_loop(rep)

    summary = dict(base, kind="summary", reps=a.reps)
    for kind in KINDS:
        for key in ("wall_s", "s_per_step_after_0", "bytes_to_host_per_step_after_0", "iterations_total"):
            vals = [r[key] for r in rows[kind] if r[key] is not None]
            summary[f"{kind}_{key}"] = round(float(np.mean(vals)), 6) if vals else None
        summary[f"{kind}_step_0_s"] = round(float(np.mean([r["step_s"][0] for r in rows[kind]])), 6) if rows[kind] else None
        summary[f"{kind}_objective_last"] = rows[kind][-1]["objective"][-1] if rows[kind] else None
        summary[f"{kind}_eta_last"] = rows[kind][-1]["eta_per_step"][-1] if rows[kind] else None
    if summary["device_s_per_step_after_0"] and summary["torch_s_per_step_after_0"]:
        summary["device_over_torch_s_per_step"] = round(summary["device_s_per_step_after_0"] / summary["torch_s_per_step_after_0"], 4)
    summary["rel_l1_between_the_two_ends"] = float(np.abs(ends["device"] - ends["torch"]).sum() / np.abs(ends["torch"]).sum()) if ends else None
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()

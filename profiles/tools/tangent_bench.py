"""Linearised transport of N bumps on one surface: what the three device calls (dots_tangent_velocities, dots_tangent_weights,
dots_tangent_gram) cost against the same quantities formed by torch on the device from the same tensors, what the embedding saves
against the N (N - 1) / 2 exact pair solves, and how far the two distance matrices are apart.

    python profiles/tools/tangent_bench.py --mesh knot --T 31 --N 8 > profiles/tangent/<name>.jsonl
    python profiles/tools/tangent_bench.py --mesh torus100k --T 31 --N 8 > profiles/tangent/<name>.jsonl

The measures: one bump (``meshes.bump_density``) at each of N vertices far from each other (``meshes.farthest_vertices``); the reference
is their mean, ``distance_matrix``'s default.  Three kinds of rows, one JSON line each:

``kernels``   one batch session solves the N problems once with the potentials left on the device; then, ``--reps`` times after one
              discarded round, the three library calls (device milliseconds of their launches, from events on their stream) alternate
              with the torch twin on the same tensors (gather + ``einsum`` for the velocities, gather + sum for the weights, a scaled
              copy + ``einsum`` -- a matrix product -- for the Gram; events on torch's stream).  The summary has the medians and the
              twin's own run-to-run spread (min and max), by which a difference is judged.
``calls``     ``socp.tangent_embedding`` and ``socp.distance_matrix(method="pairs")`` as whole calls, each building its own session,
              alternating ``--call-reps`` times after nothing discarded (each call builds plan, factor and contexts itself): seconds, the
              solves' share, the inner iterations.
``difference``  the relative difference of the linearised distance matrix from the exact one over the pairs: largest, mean, and in the
              Frobenius norm.

bench.py is unchanged; this script only reuses its mesh recipes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MESHES = {"knot": ("knot", {}), "torus100k": ("torus", dict(nu=400, nv=250))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="knot", choices=sorted(MESHES))
    ap.add_argument("--T", type=int, default=31)
    ap.add_argument("--N", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--call-reps", type=int, default=1)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--nit", type=int, default=3000)
    a = ap.parse_args()

    import numpy as np
    import torch

    from dots_socp_amd import meshes, socp

    name, kw = MESHES[a.mesh]
    geom, _ = meshes.example(name, **kw)
    v0 = np.asarray(geom["vertices"], dtype=np.float64)
    mesh = {k: val for k, val in geom.items() if k not in ("mu0", "mu1")}
    area = np.asarray(geom["area_vertices"], dtype=np.float64)
    centres = [int(c) for c in meshes.farthest_vertices(v0, 0, a.N)]
    measures = np.stack([meshes.bump_density(v0, area, [c], 0.35, 0.05) for c in centres])
    reference = np.zeros(v0.shape[0])
    for m in measures:
        reference = reference + m
    reference = reference / a.N
    base = dict(mesh=a.mesh, n_time=a.T, vertices=int(v0.shape[0]), triangles=int(np.asarray(geom["triangles"]).shape[0]), N=a.N, tol=a.tol, nit=a.nit)
    solve = dict(tol=a.tol, nit=a.nit)

    def emit(**row):
        print(json.dumps(dict(base, **row)), flush=True)

    # ---- the three calls against torch on the same tensors
    request = {"potentials": True, "stress": False, "to_device": True}
    with socp.BatchSession(a.T, mesh, max_batch=min(a.N, 8)) as bs:
        results = bs.solve_many([{"mu0": reference, "mu1": m, **solve} for m in measures], outputs=(), sensitivity=request)
        dev = bs.solvers[0].dev
        potentials = [sol["sensitivity"]["phi0"] for sol, _ in results]
        where = potentials[0].device
        tables = dev.tangent_mesh()
        tri = tables["triangles"].to(torch.int64)
        sigma = torch.as_tensor(reference, dtype=torch.float64, device=where)
        phi = torch.stack(potentials)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            return out, e0.elapsed_time(e1)

        def library():
            vel, w = dev.tangent_velocities(potentials), dev.tangent_weights(sigma)
            G = dev.tangent_gram(vel, None, w)
            return G, dict(dev.tangent_ms)

        def twin():
            vel, t_v = timed(lambda: torch.einsum("fkc,nfk->nfc", tables["hat"], phi[:, tri]))
            w, t_w = timed(lambda: (sigma / tables["mass"])[tri].sum(dim=1) * (tables["area"] * (1.0 / 3.0)))
            G, t_g = timed(lambda: torch.einsum("if,jf->ij", (vel * w[None, :, None]).reshape(a.N, -1), vel.reshape(a.N, -1)))
            return G.cpu().numpy(), {"velocities": t_v, "weights": t_w, "gram": t_g}

        rows = {"library": [], "torch": []}
        for rep in range(-1, a.reps):      # (round -1 is discarded: first launches, torch's choice of kernels)
            G_lib, ms_lib = library()
            G_twin, ms_twin = twin()
            if rep >= 0:
                rows["library"].append(ms_lib)
                rows["torch"].append(ms_twin)
                emit(kind="kernels", repeat=rep, library_ms=ms_lib, torch_ms=ms_twin)
        summary = dict(kind="kernels_summary", reps=a.reps, gram_rel_difference=float(np.max(np.abs(G_lib - G_twin)) / np.max(np.abs(G_lib))))
        for who in rows:
            for k in ("velocities", "weights", "gram"):
                vals = [r[k] for r in rows[who]]
                summary[f"{who}_{k}_ms"] = {"median": float(np.median(vals)), "min": float(np.min(vals)), "max": float(np.max(vals))}
        emit(**summary)

    # ---- the embedding against the exact pairs, as whole calls
    D_lin = D_exact = None
    for rep in range(a.call_reps):
        t0 = time.perf_counter()
        r = socp.tangent_embedding(a.T, mesh, reference, measures, **solve)
        wall = time.perf_counter() - t0
        D_lin = 0.5 * r["squared_distances"]
        emit(kind="calls", what="tangent_embedding", repeat=rep, wall_s=wall, solve_s=r["solver_stats"]["solve_seconds"], solves=a.N,
             iterations=int(np.sum(r["iterations"])), tangent_ms=r["solver_stats"]["tangent_ms"], bytes_to_host=r["solver_stats"]["bytes_to_host"],
             own_ratio=[float(r["gram"][i, i] / (2.0 * r["costs"][i])) for i in range(a.N)])
        t0 = time.perf_counter()
        D_exact = socp.distance_matrix(a.T, mesh, measures, method="pairs", **solve)
        pairs_wall = time.perf_counter() - t0
        emit(kind="calls", what="distance_matrix_pairs", repeat=rep, wall_s=pairs_wall, solves=a.N * (a.N - 1) // 2, gain_over_pairs=pairs_wall / wall)
    off = ~np.eye(a.N, dtype=bool)
    rel = np.abs(D_lin - D_exact)[off] / D_exact[off]
    emit(kind="difference", largest=float(rel.max()), mean=float(rel.mean()),
         frobenius=float(np.linalg.norm(D_lin - D_exact) / np.linalg.norm(D_exact)), exact_smallest=float(D_exact[off].min()), exact_largest=float(D_exact[off].max()))


if __name__ == "__main__":
    main()

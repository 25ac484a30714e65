"""GPU tests of solver_socp_many: problems on one surface solved in lockstep on one shared factor (dots_step_many) end where their
own solver_socp calls end -- bit for bit -- and match the reference's recorded runs."""
import numpy as np
import pytest

from conftest import has_gpu
from test_hip_solver import REL_TOL, compare, golden, rel, run_hip

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")


def problem_of(g):
    p = {"mu0": g["mu0"], "mu1": g["mu1"]}
    common = {}
    for k in g.files:
        if k.startswith("kw_"):
            val = g[k]
            val = val.tolist() if val.ndim else val.item()
            (common if k[3:] in ("eps", "lap_solver", "reorder", "nd_leaf") else p)[k[3:]] = val
    return p, common


def assert_same_run(a, b):
    (sa, ha), (sb, hb) = a, b
    assert int(ha.kkt_iteration[-1]) == int(hb.kkt_iteration[-1])
    assert np.array_equal(ha.kkt_errors, hb.kkt_errors, equal_nan=True)
    for k in STATE:
        assert np.array_equal(sa[k], sb[k]), k


def run_golden_batch(names, max_batch=4):
    from dots_socp_amd.socp import solver_socp_many

    gs = [golden(n) for n in names]
    probs, commons = zip(*[problem_of(g) for g in gs])
    assert all(c == commons[0] for c in commons)
    g0 = gs[0]
    geom = dict(vertices=g0["vertices"], triangles=g0["triangles"])
    out = solver_socp_many(int(g0["n_time"]), geom, list(probs), max_batch=max_batch, **commons[0])
    for name, g, (sol, hist) in zip(names, gs, out):
        compare(g, sol, hist, REL_TOL)
        if "ckpt_iteration" in g.files:
            assert [c["iteration"] for c in sol["checkpoints"]] == g["ckpt_iteration"].tolist()
            assert rel(np.stack([c["mu"] for c in sol["checkpoints"]]), g["ckpt_mu"]) < 1e-5
        assert_same_run((sol, hist), run_hip(g))
        assert hist.solver_stats["batch"]["size"] == len(names)
    return out


def test_refplane20_pair_in_one_batch():
    """361 and 113 iterations: the first problem runs on alone after the second stops"""
    out = run_golden_batch(["run_refplane20_T31_tol1e-3.npz", "run_refplane20_T31_cong_tol1e-3.npz"])
    assert [int(h.kkt_iteration[-1]) for _, h in out] == [361, 113]


def test_ico2_runs_in_one_batch():
    """checkpoints, congestion and is_palm in one batch"""
    run_golden_batch(["run_ico2_T15_ckpt_tol1e-3.npz", "run_ico2_T15_cong_tol1e-3.npz", "run_ico2_T15_palm_tol1e-3.npz"])


def test_knot_batch_refills_slots_bit_for_bit():
    """5 seeded density pairs with max_batch=2: slots are refilled as problems stop at different iterations"""
    from dots_socp_amd import meshes
    from dots_socp_amd.socp import solver_socp, solver_socp_many

    geom, _ = meshes.example("knot")
    v = np.asarray(geom["vertices"])
    av = meshes.vertex_areas(v.shape[0], geom["triangles"], meshes.triangle_areas(v, geom["triangles"]))
    rng = np.random.default_rng(4)
    probs = []
    for k in range(5):
        c = meshes.farthest_vertices(v, int(rng.integers(v.shape[0])), 4)
        probs.append(dict(mu0=meshes.bump_density(v, av, c[:2]), mu1=meshes.bump_density(v, av, c[2:]), tol=[1e-2, 3e-3, 1e-2, 5e-3, 2e-2][k],
                          congestion=0.01 * (k % 2), nit=400))
    mesh = dict(vertices=geom["vertices"], triangles=geom["triangles"])
    out = solver_socp_many(15, mesh, probs, max_batch=2)
    stops = set()
    for i, p in enumerate(probs):
        alone = solver_socp(15, {**mesh, "mu0": p["mu0"], "mu1": p["mu1"]}, **{k: p[k] for k in ("tol", "congestion", "nit")})
        assert_same_run(out[i], alone)
        assert out[i][1].solver_stats["batch"]["index"] == i
        stops.add(int(alone[1].kkt_iteration[-1]))
    assert len(stops) > 1      # uneven stops: the refill was exercised


def test_a_refilled_slot_builds_a_solver_with_its_own_options():
    """Three problems on the plane with max_batch=2: the third takes the slot the first to stop leaves and is built there with its own
    tau, without the z scaling and from the whole solution of the first problem; each result is its own solver_socp call's, bit for bit."""
    import session_checks as sc
    from dots_socp_amd.socp import solver_socp, solver_socp_many

    n_time, cap = sc.CASES["plane"]
    mesh, p1, p2 = sc.problems("plane")
    run = dict(tol=sc.TOL, nit=cap)
    probs = [dict(mu0=p1[0], mu1=p1[1], **run), dict(mu0=p2[0], mu1=p2[1], **run), dict(mu0=p1[1], mu1=p1[0], **run)]
    alone = [solver_socp(n_time, {**mesh, "mu0": p["mu0"], "mu1": p["mu1"]}, **run) for p in probs[:2]]
    probs[2].update(tau=1.7, is_z_scaling=False, init_solution={k: alone[0][0][k] for k in STATE})
    alone.append(solver_socp(n_time, {**mesh, "mu0": probs[2]["mu0"], "mu1": probs[2]["mu1"]},
                             **{k: v for k, v in probs[2].items() if k not in ("mu0", "mu1")}))
    out = solver_socp_many(n_time, mesh, probs, max_batch=2)
    for i, (got, want) in enumerate(zip(out, alone)):
        assert_same_run(got, want)
        assert got[1].solver_stats["batch"] == {**got[1].solver_stats["batch"], "size": 3, "index": i, "max_batch": 2}
    assert not np.array_equal(out[2][0]["phi"], out[0][0]["phi"])      # (the third ran: it did not just keep what it started from)

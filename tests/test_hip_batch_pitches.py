"""GPU tests of the batched direct solve (front_solve_many) where the single-rhs sweep is tested but the batch tests did not reach: time
pitches 32 (ragged T = 20), 64 and 128, the launches many_launch splits (NR regions of LDS above 64 KB, more right-hand sides than a
1024-thread workgroup takes), every forced sweep variant and 2 / 4 / 8 right-hand sides per launch.  Every problem of a batch must be bit
for bit its solve alone, and the solve alone must be the fp64 reference's (SuperLU per time mode)."""
import functools

import numpy as np
import pytest

from conftest import has_gpu, load_oracle
from dots_socp_amd import meshes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

# sphere(level=2), V = 162.  Leaves of these sizes make the default band rule keep the leaves' band unmerged (leaf kernels) above one
# merged band and a top band of explicit inverses; a leaf's forward LDS per rhs is 16 * leaf_nmax * TP bytes: nmax 15 at T = 20 / 127
# and 20 at T = 63, so NR = 4 splits the leaf launch at pitch 64 and 128 and NR = 2 splits it too at pitch 128 (down to one rhs).
ND_LEAF = {20: 16, 63: 20, 127: 16}
SIZES = (2, 3, 4, 5, 8, 9)      # partial chunks repeat their last problem; 9 = 8 + an m == 1 remainder at NR = 8
N_PROBLEMS = max(SIZES)


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def remove_gauge(phi, mass_v):
    w = np.broadcast_to(mass_v[None, :], phi.shape)
    return phi - np.sum(phi * w) / np.sum(w)


def pitch_of(T):
    return max(8, 1 << int(np.ceil(np.log2(T + 1))))


@functools.lru_cache(maxsize=None)
def geometry():
    return meshes.example("sphere", level=2)[0]


@functools.lru_cache(maxsize=None)
def reference(T, eps, seed):
    """distinct right-hand sides and their fp64 solutions.

    laplacian_solve_many(b) applies step 1's operator inverse as the device forms it: the factor is of K + (sigma + eps) M, the negative
    of the operator the reference's LaplacianInverse inverts (L_space + (lambda - eps) M with L_space and the time eigenvalues lambda <= 0),
    so x = -lap_inv(b), both [T+1, V] in the reference's vertex order.  At eps = 0 the operator is singular (constants in space and
    time): b is made consistent (zero sum) and x is compared without its mass-weighted mean."""
    O = load_oracle()
    s = O.OracleSolver(T, geometry(), eps=eps)
    rng = np.random.default_rng(seed)
    rhs = [rng.standard_normal((T + 1, s.V)) for _ in range(N_PROBLEMS)]
    if eps == 0.0:
        rhs = [b - b.mean() for b in rhs]
    want = [-s.lap_inv(b) for b in rhs]
    return rhs, want, s.mass_v


def make(T, eps, plan=None, **kw):
    from dots_socp_amd.device import DeviceProblem

    dev = DeviceProblem(T, geometry(), lap_solver="modal_pcg", reorder="nd", nd_leaf=ND_LEAF[T], plan=plan, **kw)
    dev.set_params(r=1.3, eps=eps)
    return dev


def family(T, eps, n, top_inverse=None):
    owner = make(T, eps)
    summary = owner.setup_frontal(eps=eps, top_inverse=top_inverse)
    devs = [owner]
    try:
        for _ in range(n - 1):
            d = make(T, eps, plan=owner.plan)
            d.share_frontal(owner)
            devs.append(d)
    except BaseException:
        close_all(devs)
        raise
    return devs, summary


def close_all(devs):
    for d in devs:
        d.close()


def check_family(devs, summary, T, eps, nr, seed=3):
    """alone == batched (bit for bit) for every batch size, alone again after the batch, alone == fp64 reference.  Returns the most launches
    of one batched solve split below their chunk (dots_debug_counter 8)."""
    from dots_socp_amd.device import laplacian_solve_many

    rhs, want, mass_v = reference(T, eps, seed)
    alone = [laplacian_solve_many([d], [b])[0] for d, b in zip(devs, rhs)]
    lps = summary["launches_per_solve"]
    assert devs[0].debug_counter(7) == lps and devs[0].debug_counter(8) == 0
    for k, (x, w) in enumerate(zip(alone, want)):
        assert np.all(np.isfinite(x)), k
        if eps == 0.0:
            x, w = remove_gauge(x, mass_v), remove_gauge(w, mass_v)
        assert rel(x, w) < 1e-9, (k, rel(x, w))
    most_split = 0
    for n in SIZES:
        got = laplacian_solve_many(devs[:n], rhs[:n])
        launches, split = devs[0].debug_counter(7), devs[0].debug_counter(8)
        chunks = -(-n // nr)
        if split == 0:
            assert launches == lps * chunks, (n, launches, lps, chunks)
        else:
            assert launches > lps * chunks and split <= launches, (n, launches, split)
        most_split = max(most_split, split)
        for k in range(n):
            assert np.array_equal(got[k], alone[k]), (n, k)
        # a batch that wrote into another context's update planes or scratch shows in a solve after it
        for k in range(n):
            assert np.array_equal(laplacian_solve_many([devs[k]], [rhs[k]])[0], alone[k]), ("after", n, k)
    # one right-hand side in two contexts of one batch: both get its solution
    got = laplacian_solve_many(devs[:5], [rhs[0], rhs[1], rhs[2], rhs[1], rhs[4]])
    for k, want_k in enumerate((0, 1, 2, 1, 4)):
        assert np.array_equal(got[k], alone[want_k]), ("same rhs", k)
    return most_split


def settings_for(T):
    """the sweep variants of test_hip_frontal.test_forward_kernel_variants_agree, two-mode lanes off, and the top band not inverted"""
    groups = 64 // max(pitch_of(T) // 2, 1)
    out = [("rule", {}, None), ("top_not_inverted", {}, False), ("fold", {"DOTS_FRONT_ROWS": "0"}, None), ("rows_everywhere", {"DOTS_FRONT_ROWS": "2"}, None),
           ("leaves_in_band_kernels", {"DOTS_FRONT_LEAFINV": "0"}, None), ("unmerged", {"DOTS_FRONT_BANDS": "off"}, None),
           ("unmerged_fold", {"DOTS_FRONT_BANDS": "off", "DOTS_FRONT_ROWS": "0"}, None),
           ("unmerged_leaves_in_band_kernels", {"DOTS_FRONT_BANDS": "off", "DOTS_FRONT_LEAFINV": "0"}, None), ("one_mode", {"DOTS_FRONT_VEC2": "0"}, None)]
    for q in (1, 2, 4, 8):
        if q <= groups:
            out.append((f"r{q}_unmerged", {"DOTS_FRONT_BANDS": "off", "DOTS_FRONT_CFG": f"fwd:r{q}"}, None))
    return out


SETTINGS = {T: {tag: (env, top) for tag, env, top in settings_for(T)} for T in ND_LEAF}
# the full product at T = 63; at T = 20 and 127 the default rule, the top band as factors, one-mode lanes and the fold kernel at every width,
# the rest at NR = 8 only
CASES = [(63, nr, tag, eps) for nr in (2, 4, 8) for tag in SETTINGS[63] for eps in (0.0, 1e-3)]
CASES += [(T, nr, tag, eps) for T in (20, 127) for nr in (2, 4, 8) for tag in ("rule", "top_not_inverted", "one_mode", "fold") for eps in (0.0, 1e-3)
          if tag in ("rule", "one_mode") or eps == 1e-3]
CASES += [(T, 8, tag, 1e-3) for T in (20, 127) for tag in SETTINGS[T] if tag not in ("rule", "top_not_inverted", "one_mode", "fold")]


@pytest.mark.parametrize("T,nr,tag,eps", CASES)
def test_batched_solve_at_pitch_split_and_variant(monkeypatch, T, nr, tag, eps):
    env, top = SETTINGS[T][tag]
    monkeypatch.setenv("DOTS_FRONT_NR", str(nr))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    devs, summary = family(T, eps, N_PROBLEMS, top_inverse=top)
    try:
        assert int(devs[0].lib.dots_front_pitch(devs[0]._h)) == pitch_of(T)
        leaves = devs[0].debug_counter(4)
        if "DOTS_FRONT_LEAFINV" in env:
            assert leaves == 0
        elif tag in ("rule", "top_not_inverted", "one_mode", "fold"):
            assert leaves > 0 and len(summary["bands"]) > 2      # the leaf kernels and a merged band of several heights
        if top is not None:
            assert summary["top_inverse"] == top
        most_split = check_family(devs, summary, T, eps, nr)
        if tag == "rule" and T >= 63 and nr >= 4:
            assert most_split > 0      # the leaf launches (LDS) split: the halving path of many_launch ran
        if tag == "rule" and T == 20 and nr == 2:
            assert most_split == 0     # pitch 32, two rhs: every launch takes its whole chunk
    finally:
        close_all(devs)


STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")
MEMBERS = [dict(congestion=0.0, palm=False), dict(congestion=0.02, palm=False), dict(congestion=0.05, palm=True)]


@pytest.mark.parametrize("T", [20, 63, 127])
def test_step_many_at_long_and_ragged_time_axes(T):
    """three problems on one factor (different congestion, one with is_palm's step 0) stepped 10 times by step_many end bit for bit where
    10 separate dots_step calls end, and stay on the oracle's trajectory (the bounds of test_hip_frontal.test_time_pitches_64_128_and_ragged).
    At T = 20 the right-hand sides k >= 1 of a launch carry 11 padding columns of the pitch: a stray value there would reach the solution."""
    from dots_socp_amd.device import DeviceProblem, step_many

    O = load_oracle()
    geom = geometry()
    refs = []
    for m in MEMBERS:
        s = O.OracleSolver(T, geom, congestion=m["congestion"])
        s.scale_z(2.0)
        for _ in range(10):
            if m["palm"]:
                s.step_q_lambda(refresh_gradients=False)
            s.iterate()
        refs.append(s)

    def setup():
        devs = []
        try:
            for i, m in enumerate(MEMBERS):
                plan = devs[0].plan if devs else None
                d = DeviceProblem(T, geom, lap_solver="modal_pcg", reorder="nd", nd_leaf=ND_LEAF[T], plan=plan)
                devs.append(d)
                if i == 0:
                    assert d.setup_frontal()["levels"] >= 3
                else:
                    d.share_frontal(devs[0])
                d.scale_z(2.0, 0.5, 2.0)
                d.set_params(scale_z=2.0, const_d=2.0, norm_d=refs[i].norm_d, congestion=m["congestion"])
                d.step_flags(palm=m["palm"])
        except BaseException:
            close_all(devs)
            raise
        return devs

    runs = []
    for batched in (True, False):
        devs = setup()
        try:
            for _ in range(10):
                if batched:
                    step_many(devs)
                else:
                    for d in devs:
                        d.step(1)
            runs.append([({k: d.download(k) for k in STATE}, d.kkt(range(7))) for d in devs])
        finally:
            close_all(devs)
    for i, ((sa, ka), (sb, kb)) in enumerate(zip(*runs)):
        for k in STATE:
            assert np.all(np.isfinite(sa[k])), (i, k)
            assert np.array_equal(sa[k], sb[k]), (i, k)
        assert all(ka[j][0] == kb[j][0] for j in range(7)), (i, ka, kb)
    for i, ((st, kkt), s) in enumerate(zip(runs[0], refs)):
        for k in ("A", "B", "mu", "E", "z_mid", "beta_mid"):
            assert rel(st[k], getattr(s, k)) < 1e-8, (T, i, k)
        want = s.kkt_all()
        for j in range(7):
            assert abs(kkt[j][0] - want[j]) <= 1e-7 * abs(want[j]) + 1e-14, (T, i, j)

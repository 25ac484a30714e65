"""The deep forms of the launches around the direct solve (k_rhs_modes2_deep, k_time_modes_tile_fast: pitch 8, 16, 32) against the
launches they stand in for, and the rule that chooses between them.

DOTS_RHS_DEEP=0 runs the kernels as they were, =1 the deep forms wherever they exist; dots_debug_counter 15 says which ran.  The deep
forms change which loads are in flight together, never the order of a sum: every array must come out bit for bit the same.  The shapes
are the ones at which this code can still go wrong: a corner list longer than one pass of DEEP_BATCH = 8 (the fan's hub, valence 9), lists
shorter than a pass (valence 1 and 2), a tile that is not full and a tile count that is not whole (V = 11, 42, 162 against 128, 64 and 32
vertices per tile), padded mode columns (T = 20 at pitch 32: eleven of them) and the last node without a partner (T even)."""
import numpy as np
import pytest

import step_checks as sc

pytestmark = pytest.mark.gpu

MESHES = ("fan", "ops_ico1", "ico2")      # V = 11 (valences 1, 2 and 9), 42, 162
T_PITCH = (6, 15, 20, 31)                 # pitch 8, 16, 32 with eleven padded columns, 32 full


@pytest.fixture(scope="module")
def geoms():
    from dots_socp_amd import meshes

    out = {m: sc.geometry(m) for m in ("fan", "ops_ico1")}
    out["ico2"] = meshes.example("sphere", level=2)[0]
    assert [len(out[m]["vertices"]) for m in MESHES] == [11, 42, 162]
    return out


def make_device(T, geom, deep, monkeypatch, params=None):
    """A context with an installed factor whose launches are forced to one form (``deep`` 0 / 1) or left to the rule (None)."""
    from dots_socp_amd.device import DeviceProblem

    if deep is None:
        monkeypatch.delenv("DOTS_RHS_DEEP", raising=False)
    else:
        monkeypatch.setenv("DOTS_RHS_DEEP", str(deep))      # (read when the context is created)
    dev = DeviceProblem(T, geom, lap_solver="modal_pcg")
    assert dev.setup_frontal(leaf=4)["levels"] >= 1
    if params:
        dev.set_params(**params)
    return dev


def deep_path(dev):
    from dots_socp_amd import _lib

    return dev.debug_counter(_lib.DEEP_PATH_COUNTER)


@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("T", T_PITCH)
def test_deep_launches_are_bit_identical_and_agree_with_the_oracle(geoms, mesh, T, monkeypatch):
    """Six iterations with the gathers carried, on the planted state of step_checks: a first step that carries nothing yet, a carried
    one, one whose right-hand side is enqueued ahead by the residuals' read-back, the step that takes it, one with a pending penalty
    division (the carried sums are dropped: the dividing launch has no deep form) and a carried one after it.  After every step all twelve
    arrays of the two contexts are equal bit for bit, the counter names the form that ran, and the deep context's step agrees with the
    oracle within the bounds of step_checks.check_one_step."""
    from dots_socp_amd import _lib

    D = _lib.DEEP_PATH
    s = sc.make_oracle(T, geoms[mesh], 0.05)
    devs = [make_device(T, geoms[mesh], deep, monkeypatch, sc.device_params(s)) for deep in (0, 1)]
    try:
        sc.edge_state(s, seed=T, zero_preimage=False)
        before = sc.snapshot(s)
        for dev in devs:
            for k in sc.STATE:
                dev.upload(k, before[k])
            assert deep_path(dev) == 0
        # (what the step does before it, the flags, whether the carried right-hand side runs inside this step)
        plan = [(None, dict(carry=True), False), (None, dict(carry=True), True), (None, dict(carry=True, rhs_ahead=True), True),
                ("ahead", dict(carry=True), False), ("penalty", dict(carry=True), False), (None, dict(carry=True), True)]
        for k, (first, flags, carried) in enumerate(plan):
            if first == "penalty":
                for dev in devs:
                    dev.adjust_penalty(sc.FACTOR)
                    dev.set_params(r=s.r * sc.FACTOR)
                before = sc.apply_penalty(s, before, sc.FACTOR)
            for dev in devs:
                dev.step_flags(**flags)
                dev.step(1, wait=False)
            # (the step of k = 3 took the right-hand side its predecessor's read-back enqueued: a carried launch, deep on devs[1])
            want = (D["rhs"] if carried or first == "ahead" else 0) | D["inverse"]
            assert deep_path(devs[0]) == 0 and deep_path(devs[1]) == want, (k, deep_path(devs[0]), deep_path(devs[1]))
            if flags.get("rhs_ahead"):
                res = [dev.kkt([0, 2, 3]) for dev in devs]      # forms the next right-hand side ahead: a new record
                assert res[0] == res[1]
                assert deep_path(devs[0]) == 0 and deep_path(devs[1]) == D["rhs"], (k, deep_path(devs[1]))
            after = [{name: dev.download(name) for name in sc.STATE} for dev in devs]
            for name in sc.STATE:
                assert np.array_equal(after[0][name], after[1][name], equal_nan=True), (k, name)
            figures = sc.check_one_step(s, before, after[1])
            print(mesh, T, k, figures)
            before = after[1]
    finally:
        for dev in devs:
            dev.close()


@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("T", T_PITCH)
def test_solve_many_is_bit_identical_on_both_paths(geoms, mesh, T, monkeypatch):
    """dots_laplacian_solve_many transforms back with the same launch as step 1: the same phi bit for bit from either form."""
    from dots_socp_amd import _lib
    from dots_socp_amd.device import laplacian_solve_many

    rng = np.random.default_rng(100 + T)
    V = len(geoms[mesh]["vertices"])
    rhs = rng.standard_normal((T + 1, V))
    rhs -= rhs.mean()
    out = []
    for deep in (0, 1):
        dev = make_device(T, geoms[mesh], deep, monkeypatch)
        try:
            out.append(laplacian_solve_many([dev], [rhs])[0])
            assert deep_path(dev) == (_lib.DEEP_PATH["inverse"] if deep else 0)
        finally:
            dev.close()
    assert np.isfinite(out[0]).all() and np.abs(out[0]).max() > 0.0
    assert np.array_equal(out[0], out[1])


def carried_step_path(dev):
    """dots_debug_counter 15 after a step that streams the carried gathers (the second of two with DOTS_STEP_CARRY)."""
    dev.step_flags(carry=True)
    dev.step(2, wait=False)
    dev.download("phi")
    return deep_path(dev)


def test_rule_small_mesh_takes_the_deep_launches(geoms, monkeypatch):
    from dots_socp_amd import _lib

    dev = make_device(6, geoms["ops_ico1"], None, monkeypatch)
    try:
        assert carried_step_path(dev) == _lib.DEEP_PATH["rhs"] | _lib.DEEP_PATH["inverse"]
    finally:
        dev.close()


def test_rule_past_the_threshold_keeps_the_launches_as_they_were(monkeypatch):
    """The rule counts the right-hand-side launch's workgroups (one per tile of 32 vertices at pitch 32, rounded up to a multiple of 8,
    and as many riders) against DEEP_WGS_PER_CU per compute unit: a torus with just enough vertices to pass it.  (The inverse
    transform has no 1024-thread launch above 512 tiles, deep or not.)"""
    import torch

    from dots_socp_amd import _lib, meshes
    from dots_socp_amd.device import DeviceProblem

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = _lib.DEEP_WGS_PER_CU * n_cu // 2 + 1           # 2 * xcd_grid(tiles) > DEEP_WGS_PER_CU * n_cu
    nv = 64
    nu = -(-((tiles - 1) * 32 + 1) // nv)
    geom = meshes.example("torus", nu=nu, nv=nv)[0]
    assert (tiles - 1) * 32 < len(geom["vertices"]) <= (tiles + 1) * 32
    monkeypatch.delenv("DOTS_RHS_DEEP", raising=False)
    with DeviceProblem(20, geom, lap_solver="modal_pcg") as dev:
        assert dev.setup_frontal()["levels"] >= 1
        assert carried_step_path(dev) == 0

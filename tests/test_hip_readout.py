"""GPU tests of the device read-out (dots_readout) through the C ABI: mu and E against the numpy specification
(readout.read_out_host of the downloaded arrays) bit for bit at every time pitch, the state hygiene of the entry point, its layer
sums against math.fsum within the first-order bound of any summation order, the six solver plug-ins with ``readout="device"``
against ``readout="host"``, the bytes that cross to the host, and the error codes."""
import math

import numpy as np
import pytest

from conftest import has_gpu
from dots_socp_amd import _lib, meshes
from dots_socp_amd.readout import read_out_host

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")
MESHES = ("ico1", "ico2", "torus", "plane", "knot")
N_TIMES = (1, 2, 6, 7, 31, 100, 255, 383, 1023)      # time pitches 8 ... 1024, with and without padding columns


def mesh(name):
    if name == "ico1":
        return meshes.example("sphere", level=1)[0]
    if name == "ico2":
        return meshes.example("sphere", level=2)[0]
    if name == "torus":
        return meshes.example("torus", nu=8, nv=6)[0]
    if name == "plane":
        return meshes.example("plane", n=8)[0]      # (a mesh with boundary)
    return meshes.example("knot")[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def stepped(n_time, geom, reorder=True, lap_solver="spacetime_pcg", steps=2, seed=0):
    """A context a few ALM steps away from a random upload of phi, mu, E and the vertex multipliers."""
    from dots_socp_amd.device import DeviceProblem

    dev = DeviceProblem(n_time, geom, lap_solver="modal_pcg" if lap_solver == "modal_direct" else lap_solver, reorder=reorder)
    if lap_solver == "modal_direct":
        dev.setup_frontal()
    else:
        dev.set_params(cg_tol=1e-2, cg_max_iter=4)      # (what the solve returns does not matter here: any state will do)
    rng = np.random.default_rng(seed + 7 * n_time)
    for name in ("phi", "mu", "E", "beta_fst", "beta_end", "lambda_c"):
        dev.upload(name, rng.standard_normal(dev.shape(name)))
    if steps:
        dev.step(steps)
    return dev


def weights(dev, seed=3):
    rng = np.random.default_rng(seed)
    return {"w_vertex": rng.uniform(0.2, 2.0, dev.V), "w_triangle": rng.uniform(0.2, 2.0, dev.F),
            "mu0": rng.standard_normal(dev.V), "mu1": rng.standard_normal(dev.V)}


def check_against_host(dev, factor=0.37, with_sums=True):
    """Every combination of centred / staggered and with / without weights against read_out_host of the downloads."""
    w = weights(dev)
    arrays = {"mu": dev.download("mu"), "E": dev.download("E")}
    assert np.any(arrays["mu"] != 0.0) and np.any(arrays["E"] != 0.0)
    for centred in (False, True):
        for weighted in (False, True):
            kw = dict(w_vertex=w["w_vertex"] if weighted else None, w_triangle=w["w_triangle"] if weighted else None, centred=centred,
                      mu0=w["mu0"] if centred else None, mu1=w["mu1"] if centred else None)
            want_mu, want_E = read_out_host(arrays, factor, **kw)
            mu, E, mass, neg = dev.readout(factor, **kw)
            assert same(mu, want_mu), (centred, weighted)
            assert same(E, want_E), (centred, weighted)
            assert dev.readout_bytes == mu.nbytes + E.nbytes
            if with_sums:
                check_sums(want_mu, mass, neg)
                _, _, mass2, neg2 = dev.readout(factor, mu=False, E=False, **kw)      # (the sums alone, a second time)
                assert same(mass, mass2) and same(neg, neg2)


def check_sums(mu, mass, neg):
    """|sum - fsum| <= V 2^-52 sum |x|: the first-order bound n u sum |x| of any order of summation."""
    V = mu.shape[1]
    worst = 0.0
    for l in range(mu.shape[0]):
        row = mu[l]
        bound = V * 2.0 ** -52 * float(math.fsum(np.abs(row)))
        exact, exact_neg = math.fsum(row), math.fsum(row[row < 0.0])
        if bound > 0.0:
            worst = max(worst, abs(mass[l] - exact) / bound, abs(neg[l] - exact_neg) / bound)
        assert abs(mass[l] - exact) <= bound, (l, mass[l], exact, bound)
        assert abs(neg[l] - exact_neg) <= bound, (l, neg[l], exact_neg, bound)
    print(f"layer sums of {mu.shape}: largest error / bound = {worst:.3e}")


@pytest.mark.parametrize("n_time", N_TIMES)
@pytest.mark.parametrize("name", MESHES)
def test_readout_equals_the_host_path_bit_for_bit(name, n_time):
    geom = mesh(name)
    for reorder in (True, False):
        dev = stepped(n_time, geom, reorder=reorder)
        try:
            assert (dev.plan.perm_vert is not None) == reorder
            check_against_host(dev)
        finally:
            dev.close()


@pytest.mark.parametrize("lap_solver", ["spacetime_pcg", "modal_pcg", "modal_direct"])
def test_readout_carries_out_a_pending_penalty_division(lap_solver):
    dev = stepped(12, mesh("torus"), lap_solver=lap_solver, steps=3)
    try:
        dev.adjust_penalty(1.7)      # (left to the next iteration's kernels: the read-out must carry it out first)
        mu, E, _, _ = dev.readout(2.5)
        want_mu, want_E = read_out_host({"mu": dev.download("mu"), "E": dev.download("E")}, 2.5)
        assert same(mu, want_mu) and same(E, want_E)
        check_against_host(dev)
    finally:
        dev.close()


@pytest.mark.parametrize("lap_solver", ["spacetime_pcg", "modal_direct"])
def test_readout_needs_no_z_mid(lap_solver):
    dev = stepped(9, mesh("ico2"), lap_solver=lap_solver, steps=1)
    try:
        dev.step_flags(skip_z_mid=True)
        dev.step(2)
        check_against_host(dev)
        with pytest.raises(_lib.HipLibraryError) as err:      # (and it did not materialise z_mid)
            dev.download("z_mid")
        assert err.value.status == _lib.ERR_STATE
        dev.step_flags()
        dev.step(1)
        dev.download("z_mid")
        check_against_host(dev, with_sums=False)
    finally:
        dev.close()


@pytest.mark.parametrize("lap_solver", ["spacetime_pcg", "modal_direct"])
def test_readout_leaves_the_state_untouched(lap_solver):
    geom = mesh("torus")
    a, b = (stepped(20, geom, lap_solver=lap_solver, steps=3, seed=5) for _ in range(2))
    try:
        before = {n: a.download(n) for n in STATE}
        w = weights(a)
        a.readout(0.5, w["w_vertex"], w["w_triangle"], True, w["mu0"], w["mu1"])
        after = {n: a.download(n) for n in STATE}
        for n in STATE:
            assert same(before[n], after[n]), n
        # the iteration goes on as on a twin that was never read out -- with the hints of the driver's loop set, and a read-out between steps
        for dev in (a, b):
            dev.step_flags(carry=lap_solver == "modal_direct", kkt_sums=lap_solver == "modal_direct")
            dev.step(1)
        a.readout(1.0)
        for dev in (a, b):
            dev.step(2)
        for n in STATE:
            assert same(a.download(n), b.download(n)), n
    finally:
        a.close()
        b.close()


# ---- the plug-ins ----------------------------------------------------------------------------------------------------------
def fixtures():
    torus = meshes.example("torus", nu=16, nv=10)[0]
    ico = meshes.example("sphere", level=2)[0]
    return {"checkpoints": (torus, dict(nit=150, tol=1e-3, tol_checkpoints=[5e-1, 1e-1, 1e-2])),
            "congestion": (ico, dict(nit=80, tol=1e-3, congestion=0.05))}


def compare_results(dev_result, host_result, want_checkpoints):
    (sol_d, hist_d), (sol_h, hist_h) = dev_result, host_result
    assert set(sol_d) == set(sol_h)
    assert same(sol_d["mu"], sol_h["mu"]) and same(sol_d["E"], sol_h["E"])
    cps_d, cps_h = sol_d.get("checkpoints") or [], sol_h.get("checkpoints") or []
    assert len(cps_d) == len(cps_h)
    if want_checkpoints:
        assert len(cps_d) >= 1
    for cd, ch in zip(cps_d, cps_h):
        assert same(cd["mu"], ch["mu"]) and same(cd["E"], ch["E"]) and cd["iteration"] == ch["iteration"]
        assert np.array_equal(np.asarray(cd["kkt"], dtype=np.float64), np.asarray(ch["kkt"], dtype=np.float64), equal_nan=True)
    assert np.array_equal(np.asarray(hist_d.kkt_errors, dtype=np.float64), np.asarray(hist_h.kkt_errors, dtype=np.float64), equal_nan=True)
    assert np.array_equal(hist_d.kkt_iteration, hist_h.kkt_iteration)      # (the stopping iteration with them)
    assert hist_d.last_record_it == hist_h.last_record_it
    for key in hist_h.history:
        assert np.array_equal(np.asarray(hist_d.history[key], dtype=np.float64), np.asarray(hist_h.history[key], dtype=np.float64), equal_nan=True), key
    ro = hist_d.solver_stats["readout"]
    assert set(ro) == {"layer_mass", "layer_negative", "ms", "bytes"} and "readout" not in hist_h.solver_stats
    assert ro["bytes"] == sol_d["mu"].nbytes + sol_d["E"].nbytes
    check_sums(sol_d["mu"], ro["layer_mass"], ro["layer_negative"])


@pytest.mark.parametrize("fixture", ["checkpoints", "congestion"])
@pytest.mark.parametrize("plugin", ["solver", "solver_raw", "solver_cascade", "solver_raw_cascade"])
def test_plug_ins_device_against_host(plugin, fixture):
    from dots_socp_amd import socp

    geom, kw = fixtures()[fixture]
    run = getattr(socp, plugin)
    got = run(31, geom, readout="device", **kw)
    ref = run(31, geom, readout="host", **kw)
    compare_results(got, ref, fixture == "checkpoints")
    assert got[0]["mu"].shape[0] == (32 if plugin in ("solver", "solver_cascade") else 31)


@pytest.mark.parametrize("fixture", ["checkpoints", "congestion"])
@pytest.mark.parametrize("plugin", ["solver_many", "solver_raw_many"])
def test_batched_plug_ins_device_against_host(plugin, fixture):
    from dots_socp_amd import socp

    geom, kw = fixtures()[fixture]
    problems = [dict(kw), dict(kw, mu0=geom["mu1"], mu1=geom["mu0"]), dict(kw, nit=40)]
    mesh_only = {k: v for k, v in geom.items() if k not in ("mu0", "mu1")}
    mesh_only.update(mu0=geom["mu0"], mu1=geom["mu1"])
    run = getattr(socp, plugin)
    got = run(15, mesh_only, problems, readout="device")
    ref = run(15, mesh_only, problems, readout="host")
    assert len(got) == len(ref) == 3
    for g, r in zip(got, ref):
        compare_results(g, r, False)
    if fixture == "checkpoints":
        assert any(g[0].get("checkpoints") for g in got)


@pytest.mark.parametrize("name,n_time", [("torus", 6), ("knot", 31), ("ico2", 383)])
def test_readout_through_the_pinned_slots(monkeypatch, name, n_time):
    """DOTS_READOUT_PINNED=<KB per slot>: the copies go through two pinned slots.  4 KB slots: every array takes many rounds of both."""
    monkeypatch.setenv("DOTS_READOUT_PINNED", "4")
    dev = stepped(n_time, mesh(name))
    try:
        assert dev.download("E").nbytes > 2 * 4096
        check_against_host(dev)
    finally:
        dev.close()


def test_solver_socp_outputs():
    from dots_socp_amd.socp import solver_socp

    geom, kw = fixtures()["checkpoints"]
    full, _ = solver_socp(15, geom, **kw)
    part, _ = solver_socp(15, geom, outputs=("mu", "E"), **kw)
    assert set(part) == {"mu", "E", "checkpoints"} and set(full) == set(STATE) | {"checkpoints"}
    assert same(part["mu"], full["mu"]) and same(part["E"], full["E"])
    assert len(part["checkpoints"]) == len(full["checkpoints"]) >= 1
    with pytest.raises(ValueError):
        solver_socp(15, geom, outputs=("mu",), read_out={"dot_units": True, "centred": True}, **kw)


def test_bytes_that_cross_to_the_host():
    from dots_socp_amd.socp.solver_socp import AlmSolver

    geom, kw = fixtures()["congestion"]
    T, V, F = 15, geom["vertices"].shape[0], geom["triangles"].shape[0]
    moved = {}
    for readout in ("device", "host"):
        alm = AlmSolver(T, geom, **kw)
        try:
            for _ in range(kw["nit"]):
                if alm.iterate():
                    break
            before = alm.dev.debug_counter(9)
            sol, _ = alm.finalize(read_out={"dot_units": True, "centred": True} if readout == "device" else None)
            moved[readout] = alm.dev.debug_counter(9) - before
            if readout == "device":
                assert moved[readout] <= sol["mu"].nbytes + sol["E"].nbytes
        finally:
            alm.close()
    S = 8 * ((T + 1) * V + 7 * T * V + 6 * (T + 1) * F + 36 * T * F)
    print(f"bytes to the host at the end of a solve: device {moved['device']}, host {moved['host']}, S = {S}")
    assert moved["host"] >= S


def test_errors_leave_the_context_usable():
    import ctypes as C

    from dots_socp_amd.device import DeviceProblem

    geom = mesh("torus")
    dev = stepped(6, geom)
    try:
        with pytest.raises(_lib.HipLibraryError) as err:
            dev.readout(1.0, centred=True)      # (no mu0 / mu1)
        assert err.value.status == _lib.ERR_ARGUMENT
        check_against_host(dev, with_sums=False)
        with pytest.raises(_lib.HipLibraryError) as err:
            dev.readout(1.0, mu=False, E=False, sums=False)
        assert err.value.status == _lib.ERR_ARGUMENT
        assert dev.lib.dots_readout(dev._h, None) == _lib.ERR_ARGUMENT
        check_against_host(dev, with_sums=False)
    finally:
        dev.close()
    slab = DeviceProblem(7, geom, lap_solver="modal_pcg", time_slab=(0, 2))
    try:
        out = np.empty((slab.T, slab.V))
        d = _lib.ReadoutDesc()
        d.factor = 1.0
        d.mu = out.ctypes.data_as(C.POINTER(C.c_double))
        assert slab.lib.dots_readout(slab._h, C.byref(d)) == _lib.ERR_STATE
        assert slab.download("mu").shape == slab.shape("mu")
    finally:
        slab.close()

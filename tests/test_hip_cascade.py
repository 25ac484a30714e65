"""GPU tests of the coarse-to-fine time cascade: the transfer of the state between two time grids on the device (dots_prolong_time)
against its host specification (cascade.prolong_time) bit for bit, the state hygiene of the entry point on both contexts, its error
codes, the driver against the same cascade over the host and against the oracle, and a long horizon end to end."""
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu, load_oracle
from dots_socp_amd import _lib, cascade, meshes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")
# (1, 3): one source interval, the clamp min(j + 1, ns - 1) acts on every interval column; (31, 7): coarsening, the source pitch is the larger
GRIDS = [(7, 15), (15, 31), (31, 63), (20, 50), (31, 31), (63, 127), (255, 511), (300, 1023), (1, 3), (31, 7)]


def delaunay_patch(seed=11, n=150):
    """A random Delaunay patch: points in the unit square lifted onto a gentle bump, one bump of mass at either end."""
    from scipy.spatial import Delaunay

    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2))
    tri = Delaunay(xy).simplices.astype(np.int64)
    v = np.column_stack([xy, 0.2 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1])])
    area = meshes.triangle_areas(v, tri)
    tri = tri[area > 1e-6]      # (slivers on the hull)
    used = np.unique(tri)
    inv = np.full(n, -1)
    inv[used] = np.arange(used.size)
    v, tri = v[used], inv[tri]
    geom, _ = meshes.make_geometry(v, tri)
    c = meshes.farthest_vertices(geom["vertices"], 0, 2)
    geom["mu0"] = meshes.bump_density(geom["vertices"], geom["area_vertices"], [c[0]], 0.5, 0.1)
    geom["mu1"] = meshes.bump_density(geom["vertices"], geom["area_vertices"], [c[1]], 0.5, 0.1)
    return geom


def mesh(name):
    return meshes.example("torus", nu=16, nv=10)[0] if name == "torus" else delaunay_patch()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def scaled_source(geom, n_time, **kw):
    """A finalised solver whose iterate is scaled: a few iterations with penalty updates, then a primal / dual rescaling and a z
    rescale, so that every factor of the recovered solution differs from 1."""
    from dots_socp_amd.socp.solver_socp import AlmSolver

    alm = AlmSolver(n_time, geom, nit=40, tol=1e-12, check_kkt_step_by_step=True, **kw)
    for _ in range(12):
        alm.iterate()
    alm.scale_prim_dual(scale_factor=(5.0, 0.7))      # (the rescaling of is_constant_scaling, with factors that are sure to be applied)
    alm.scale_variable_z(1.5)
    alm.iterate()
    alm.finalize(download=False)
    assert alm.r != 1.0 and alm.scale_z not in (1.0, 2.0) and alm.prim_scale != 1.0 and alm.dual_scale != 1.0
    assert all(f != 1.0 for f in alm.recovery_factors())
    return alm


def host_prolongation(alm, n_dst):
    """What the host path uploads: the recovered arrays of the source, interpolated by the specification."""
    return {k: cascade.prolong_time(alm.recovered(k, alm.dev.download(k)), k, alm.n_time, n_dst) for k in STATE}


_sources = {}


def source(name, n_src):
    if (name, n_src) not in _sources:
        _sources[name, n_src] = scaled_source(mesh(name), n_src)
    return _sources[name, n_src]


@pytest.fixture(scope="module", autouse=True)
def _close_sources():
    yield
    for alm in _sources.values():
        alm.close()
    _sources.clear()


@pytest.mark.parametrize("name", ["torus", "patch"])
@pytest.mark.parametrize("n_src,n_dst", GRIDS)
def test_prolongation_matches_the_host_specification(name, n_src, n_dst):
    from dots_socp_amd.device import DeviceProblem

    geom = mesh(name)
    alm = source(name, n_src)
    want = host_prolongation(alm, n_dst)
    orders = ["nd"]
    probe = DeviceProblem(n_dst, geom, lap_solver="modal_pcg", reorder="nd")
    if cascade.row_map(probe.plan.perm_vert, alm.dev.plan.perm_vert, probe.V) is None:
        orders.append(False)      # both sides planned the same bands: the second pass has really different numberings
    probe.close()
    for reorder in orders:
        with DeviceProblem(n_dst, geom, lap_solver="modal_pcg", reorder=reorder) as dst:
            if reorder is False:
                assert cascade.row_map(dst.plan.perm_vert, alm.dev.plan.perm_vert, dst.V) is not None
                assert cascade.row_map(dst.plan.perm_tri, alm.dev.plan.perm_tri, dst.F) is not None
            ms = dst.prolong_from(alm.dev, alm.recovery_factors())
            assert ms >= 0.0
            for k in STATE:
                got = dst.download(k)
                assert got.shape == want[k].shape
                assert np.array_equal(bits(got), bits(want[k])), (k, reorder, float(np.max(np.abs(got - want[k]))))


def test_prolongation_with_and_without_row_maps():
    """The one runtime branch of the carrier's space mode "same": both row maps null (neither side renumbered) and both passed (only the
    destination renumbered), from one source, each against the host specification."""
    from dots_socp_amd.device import DeviceProblem

    geom = mesh("torus")
    alm = scaled_source(geom, 7, reorder=False)
    try:
        want = host_prolongation(alm, 15)
        for reorder in (False, "nd"):
            with DeviceProblem(15, geom, lap_solver="modal_pcg", reorder=reorder) as dst:
                maps = (cascade.row_map(dst.plan.perm_vert, alm.dev.plan.perm_vert, dst.V), cascade.row_map(dst.plan.perm_tri, alm.dev.plan.perm_tri, dst.F))
                assert all((m is None) == (reorder is False) for m in maps)
                dst.prolong_from(alm.dev, alm.recovery_factors())
                for k in STATE:
                    assert np.array_equal(bits(dst.download(k)), bits(want[k])), (k, reorder)
    finally:
        alm.close()


def test_some_default_pair_has_different_numberings():
    """The sweep order follows the bands planned with the mode pitch: on the knot the levels 31 and 63 are numbered differently."""
    from dots_socp_amd.geometry import build_level_plans

    geom, _ = meshes.example("knot")
    a, b = build_level_plans([31, 63], geom, reorder="nd")
    assert cascade.row_map(b.perm_vert, a.perm_vert, a.n_vertices) is not None


def raw_prolong(dst, src, n_src, null_table=False):
    nj, nw = cascade.time_weights(n_src, dst.T, True)
    ij, iw = cascade.time_weights(n_src, dst.T, False)
    d = _lib.ProlongDesc()
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    d.node_j, d.node_w, d.interval_j, d.interval_w = p(nj, C.c_int32), p(nw, C.c_double), p(ij, C.c_int32), p(iw, C.c_double)
    if null_table:
        d.interval_w = None
    for i in range(4):
        d.factor[i] = 1.0
    return dst.lib.dots_prolong_time(dst._h, src._h, C.byref(d))


def test_error_codes():
    from dots_socp_amd.device import DeviceProblem

    geom = mesh("torus")
    other, _ = meshes.example("torus", nu=12, nv=8)
    with DeviceProblem(15, geom, lap_solver="modal_pcg") as src, DeviceProblem(31, geom, lap_solver="modal_pcg") as dst, \
            DeviceProblem(31, other, lap_solver="modal_pcg") as alien, DeviceProblem(31, geom, lap_solver="modal_pcg", time_slab=(0, 2)) as slab:
        assert raw_prolong(dst, src, 15) == 0
        assert raw_prolong(alien, src, 15) == _lib.ERR_ARGUMENT
        assert raw_prolong(dst, src, 15, null_table=True) == _lib.ERR_ARGUMENT
        assert raw_prolong(dst, dst, 31) == _lib.ERR_ARGUMENT
        assert raw_prolong(slab, src, 15) == _lib.ERR_STATE
        assert raw_prolong(dst, slab, 31) == _lib.ERR_STATE
        assert raw_prolong(dst, src, 31) == _lib.ERR_ARGUMENT      # tables of a longer source: entries beyond its last node
        with pytest.raises(ValueError):
            dst.prolong_from(alien)
        with pytest.raises(ValueError):
            slab.prolong_from(src)


def test_source_is_brought_up_to_date_or_refused():
    """After a quiet step (z_mid not stored, a penalty division pending, carried sums set) the call refuses; after a step that keeps z_mid
    (deferred: rebuilt on demand) with a division pending it carries both out first -- it never prolongs stale arrays."""
    from dots_socp_amd.device import DeviceProblem
    from dots_socp_amd.socp.solver_socp import AlmSolver

    geom = mesh("torus")
    alm = AlmSolver(15, geom, nit=100, tol=1e-12)
    try:
        for _ in range(5):
            alm.iterate()
        dev = alm.dev
        with DeviceProblem(31, geom, lap_solver="modal_pcg", reorder="nd") as dst:
            dev.step_flags(skip_z_mid=True, carry=True)
            dev.step(1, wait=False)
            alm.adjust_penalty(1.3)      # (pending: carried out by the next reader of the dual arrays)
            with pytest.raises(_lib.HipLibraryError) as err:
                dst.prolong_from(dev, alm.recovery_factors())
            assert err.value.status == _lib.ERR_STATE
            dev.step_flags(carry=True, kkt_sums=True)
            dev.step(1, wait=False)      # z_mid of this iterate exists, on demand
            alm.adjust_penalty(1.0 / 1.7)
            dst.prolong_from(dev, alm.recovery_factors())
            got = {k: dst.download(k) for k in STATE}
            want = host_prolongation(alm, 31)
            for k in STATE:
                assert np.array_equal(bits(got[k]), bits(want[k])), k
            assert np.any(want["z_mid"] != 0.0) and np.any(want["beta_mid"] != 0.0)
    finally:
        alm.close()


def test_destination_steps_as_after_the_uploads():
    """A step with DOTS_STEP_CARRY right after the call gives the iterate the same step gives after the equivalent uploads: whatever the
    destination carried from its own earlier iterations is dropped."""
    from dots_socp_amd.socp.solver_socp import AlmSolver

    geom = mesh("torus")
    src = source("torus", 15)
    want = host_prolongation(src, 31)
    finals = []
    for via_device in (True, False):
        alm = AlmSolver(31, geom, nit=100, tol=1e-12)
        try:
            for _ in range(4):      # carried sums, fused KKT sums, possibly a launch ahead and a deferred z_mid are in place
                alm.iterate()
            dev = alm.dev
            if via_device:
                dev.prolong_from(src.dev, src.recovery_factors())
            else:
                for k in STATE:
                    dev.upload(k, want[k])
            dev.step_flags(carry=True, kkt_sums=True)
            dev.step(1, wait=False)
            dev.step_flags(carry=True, kkt_sums=True)
            dev.step(1, wait=False)
            finals.append({k: dev.download(k) for k in STATE})
        finally:
            alm.close()
    for k in STATE:
        assert np.array_equal(bits(finals[0][k]), bits(finals[1][k])), k


def test_cascade_equals_the_cascade_over_the_host():
    """The finest level of solver_socp_cascade against solver_socp warm-started with the host prolongation of the level-15 solution."""
    from dots_socp_amd.socp import solver_socp, solver_socp_cascade

    geom, _ = meshes.example("knot")
    kw = dict(tol=1e-3, nit=2000)
    sol15, _ = solver_socp(15, geom, **kw)
    sol_h, hist_h = solver_socp(31, geom, init_solution=cascade.prolong_solution(sol15, 15, 31), **kw)
    sol_c, hist_c = solver_socp_cascade(31, geom, levels=[15, 31], **kw)
    assert int(hist_c.kkt_iteration[-1]) == int(hist_h.kkt_iteration[-1])
    assert hist_c.kkt_errors.shape == hist_h.kkt_errors.shape
    assert np.array_equal(np.isnan(hist_c.kkt_errors), np.isnan(hist_h.kkt_errors)), "lazy KKT schedule differs"
    assert np.array_equal(hist_c.kkt_errors, hist_h.kkt_errors, equal_nan=True)
    for key in ("Transportation cost", "Objective value"):
        assert np.array_equal(hist_c.history[key], hist_h.history[key], equal_nan=True), key
    for k in STATE:
        assert np.array_equal(bits(sol_c[k]), bits(sol_h[k])), (k, float(np.max(np.abs(sol_c[k] - sol_h[k]))))
    rec = hist_c.solver_stats["cascade"]["levels"]
    assert [r["n_time"] for r in rec] == [15, 31] and rec[1]["iterations"] == int(hist_h.kkt_iteration[-1]) + 1


@pytest.mark.parametrize("congestion,counts", [(0.0, (327, 51)), (0.1, (105, 29))])
def test_cascade_matches_the_oracle_cascade(congestion, counts):
    """Plane n = 20, levels [15, 31], tol 1e-3: every level stops at the iteration of the oracle's cascade (the counts measured when the
    scheme was proposed), cost within the project's parity budget of 1e-6 relative."""
    from dots_socp_amd.socp import solver_socp_cascade

    O = load_oracle()
    geom, _ = meshes.example("plane", n=20)
    kw = dict(congestion=congestion, nit=4000, tol=1e-3)
    sol15, h15 = O.solver_socp(15, geom, **kw)
    _, h31 = O.solver_socp(31, geom, init_solution=cascade.prolong_solution(sol15, 15, 31), **kw)
    want = (h15.last_record_it + 1, h31.last_record_it + 1)
    _, hist = solver_socp_cascade(31, geom, levels=[15, 31], **kw)
    rec = hist.solver_stats["cascade"]["levels"]
    got = tuple(r["iterations"] for r in rec)
    costs = (h15.history["Transportation cost"][-1], h31.history["Transportation cost"][-1])
    print(f"congestion {congestion}: iterations device {got}, oracle {want}; cost device {[r['cost'] for r in rec]}, oracle {costs}")
    assert want == counts
    assert got == want
    for r, c in zip(rec, costs):
        assert abs(r["cost"] - c) <= 1e-6 * abs(c)
    assert abs(hist.history["Transportation cost"][-1] - costs[1]) <= 1e-6 * abs(costs[1])


def test_long_horizon_end_to_end():
    """Knot at n_time = 255, default levels, tol 1e-3: converged, mass conserved per layer, fewer finest-level iterations than the cold
    run, and complete records.  (The mass bound is the tolerance of the solve: the continuity equation is one of the residuals.)"""
    from dots_socp_amd import evaluate
    from dots_socp_amd.socp import solver_raw_cascade, solver_socp

    geom, _ = meshes.example("knot")
    tol = 1e-3
    kw = dict(tol=tol, nit=4000)
    _, cold = solver_socp(255, geom, **kw)
    sol, hist = solver_raw_cascade(255, geom, **kw)
    stats = hist.solver_stats["cascade"]
    rec = stats["levels"]
    assert [r["n_time"] for r in rec] == [15, 31, 63, 127, 255]
    last = np.asarray(hist.kkt_errors[-1], dtype=np.float64)
    assert last.shape == (7,) and np.all(np.isfinite(last)) and np.all(last < tol), last
    assert sol["mu"].shape == (255, np.asarray(geom["vertices"]).shape[0])
    mass = evaluate.check_mass_conservation(sol["mu"])
    n_cold, n_fine = int(cold.kkt_iteration[-1]) + 1, rec[-1]["iterations"]
    print(f"knot T = 255: cold {n_cold} iterations in {cold.running_time:.3f} s; cascade per level "
          f"{[(r['n_time'], r['iterations'], round(r['running_time'], 3), round(r['setup_seconds'], 3), r['prolong_ms']) for r in rec]}, "
          f"total {stats['total_seconds']:.3f} s; finest-level ratio {n_cold / n_fine:.2f}; mass conservation {mass:.2e}")
    assert mass < tol
    assert n_fine < n_cold
    assert n_fine == int(hist.kkt_iteration[-1]) + 1
    for i, r in enumerate(rec):
        assert set(r) >= {"n_time", "tol", "iterations", "running_time", "setup_seconds", "prolong_ms", "kkt_max", "cost"}
        assert r["iterations"] >= 1 and r["running_time"] > 0 and r["setup_seconds"] > 0 and r["kkt_max"] < tol
        assert (r["prolong_ms"] is None) if i == 0 else (r["prolong_ms"] > 0)
    assert hist.running_time == rec[-1]["running_time"] and stats["total_seconds"] >= sum(r["running_time"] for r in rec)

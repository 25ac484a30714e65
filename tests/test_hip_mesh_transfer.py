"""GPU tests of the cascade in space between independent triangulations of one surface: the barycentric transfer of the state on the
device (dots_transfer_space) against its host specification (cascade.transfer_space) bit for bit at every pitch and under every
pairing of device numberings, the driver against the same cascade over the host (located levels alone and mixed with a nested one),
convergence against the cold solve, the order of release and factorisation, the error codes of the entry point and the state of the
source."""
import ctypes as C

import numpy as np
import pytest

from carry_checks import STATE, bits, check_carry, with_bumps
from conftest import has_gpu
from dots_socp_amd import _lib, cascade, meshes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

CONVERGENCE_TOL = 1e-5


def rotation(az, ax):
    """Rz(az) . Rx(ax)"""
    rz = np.array([[np.cos(az), -np.sin(az), 0.0], [np.sin(az), np.cos(az), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(ax), -np.sin(ax)], [0.0, np.sin(ax), np.cos(ax)]])
    return rz @ rx


def rotated_icosphere(level, az, ax):
    v, t = meshes.icosphere(level)
    return v @ rotation(az, ax).T, t


_pairs = {}


def pair(name):
    """(coarse geometry, fine geometry, transfer) of two independent triangulations: plane(4) -> plane(7) (25 -> 72 vertices, 14 of them
    outside the coarse patch), icosphere(1) -> icosphere(2) rotated (42 -> 162, no shared vertex), torus (8, 6) -> (13, 9) (48 -> 117)."""
    if name not in _pairs:
        if name == "plane":
            coarse, fine = meshes.plane(4), meshes.plane(7)
        elif name == "icosphere":
            coarse, fine = meshes.icosphere(1), rotated_icosphere(2, 0.7, 0.4)
        else:
            coarse, fine = meshes.torus(8, 6), meshes.torus(13, 9)
        coarse, fine = with_bumps(*coarse), with_bumps(*fine)
        _pairs[name] = (coarse, fine, cascade.mesh_transfer(coarse, fine))
    return _pairs[name]


def sphere_parts():
    """The normalised icosphere(1) with the three bumps of the nested tests, the map that normalised it, and the bumps as a function of
    (vertices, area_vertices): around the POINTS of the three coarse centres, so that every triangulation gets the same densities."""
    v, t = meshes.icosphere(1)
    geom, scale = meshes.make_geometry(v, t)
    lo = v.min(axis=0)
    place = lambda p: (p - lo) * scale      # noqa: E731
    centres = geom["vertices"][meshes.farthest_vertices(geom["vertices"], 0, 3)]

    def bump(vv, area, points):
        mu = np.zeros(vv.shape[0])
        for p in points:
            d = np.linalg.norm(vv - p, axis=1)
            mu += area * np.where(d < 0.6, np.exp(-d ** 2 / 0.2), 0.0)
        return mu / mu.sum()

    dens = lambda vv, a: (bump(vv, a, centres[:1]), bump(vv, a, centres[1:]))      # noqa: E731
    geom["mu0"], geom["mu1"] = dens(geom["vertices"], geom["area_vertices"])
    return geom, place, dens


def placed(mesh, place):
    return meshes.make_geometry(place(mesh[0]), mesh[1], normalize=False)[0]


def located_sphere_levels():
    """Three triangulations of one sphere, none nested in another: icosphere(1), icosphere(2) rotated by Rz(0.7) Rx(0.4), icosphere(3)
    rotated by Rz(-0.3) Rx(1.1), normalised together, linked by meshes.link_levels with the same three bumps on every level."""
    geom, place, dens = sphere_parts()
    return meshes.link_levels([geom, placed(rotated_icosphere(2, 0.7, 0.4), place), placed(rotated_icosphere(3, -0.3, 1.1), place)], densities=dens)


def mixed_sphere_levels():
    """icosphere 1 -> 2 nested (``parents``), then the rotated icosphere(3) located on level 2 (``transfer``)"""
    geom, place, dens = sphere_parts()
    centre = geom["vertices"].mean(axis=0)
    radius = np.linalg.norm(geom["vertices"][0] - centre)
    project = lambda p: centre + radius * (p - centre) / np.linalg.norm(p - centre, axis=1, keepdims=True)      # noqa: E731
    nested = meshes.refine_levels(geom, 2, project=project, densities=dens)
    return meshes.link_levels(nested + [placed(rotated_icosphere(3, -0.3, 1.1), place)], densities=dens)


def carry_up(solution, fine):
    """The host's transfer of a solution to the level ``fine``, by whichever map the level carries"""
    if fine.get("parents") is not None:
        return cascade.prolong_space_solution(solution, fine["parents"])
    return cascade.transfer_space_solution(solution, fine["transfer"])


def check_pair(name, n_time, **orders):
    coarse, fine, transfer = pair(name)
    check_carry(coarse, fine, n_time, carry=lambda dst, src, factors: dst.transfer_space_from(src, transfer, factors),
                host=lambda solution: cascade.transfer_space_solution(solution, transfer),
                bytes_ok=lambda dst, pitch: dst.prolong_bytes == 8 * pitch * (32 * dst.V + 84 * dst.F), **orders)


@pytest.mark.parametrize("name", ["plane", "icosphere", "torus"])
@pytest.mark.parametrize("n_time", [1, 3, 6, 15, 31])
def test_transfer_matches_the_host_specification(name, n_time):
    check_pair(name, n_time)


def test_transfer_in_column_chunks():
    """T + 1 = 257 nodes: a pitch of 512, rows walked in two chunks of 256 columns."""
    check_pair("icosphere", 256, src_orders=(True,), dst_orders=("nd",))


def check_driver_against_the_host_chain(levels, kinds):
    from dots_socp_amd.socp import solver_socp, solver_socp_mesh_cascade

    kw = dict(tol=1e-3, nit=4000)
    sol, _ = solver_socp(7, levels[0], **kw)
    sol, _ = solver_socp(7, levels[1], init_solution=carry_up(sol, levels[1]), **kw)
    sol_h, hist_h = solver_socp(7, levels[2], init_solution=carry_up(sol, levels[2]), **kw)
    sol_c, hist_c = solver_socp_mesh_cascade(7, levels, **kw)
    assert int(hist_c.kkt_iteration[-1]) == int(hist_h.kkt_iteration[-1])
    assert hist_c.kkt_errors.shape == hist_h.kkt_errors.shape
    assert np.array_equal(hist_c.kkt_errors, hist_h.kkt_errors, equal_nan=True)
    for key in ("Transportation cost", "Objective value"):
        assert np.array_equal(hist_c.history[key], hist_h.history[key], equal_nan=True), key
    for k in STATE:
        assert np.array_equal(bits(sol_c[k]), bits(sol_h[k])), (k, float(np.max(np.abs(sol_c[k] - sol_h[k]))))
    rec = hist_c.solver_stats["mesh_cascade"]["levels"]
    assert [r["n_vertices"] for r in rec] == [42, 162, 642] and rec[2]["iterations"] == int(hist_h.kkt_iteration[-1]) + 1
    assert [r["transfer"] for r in rec] == [None] + list(kinds)
    assert rec[0]["prolong_ms"] is None and all(r["prolong_ms"] > 0 and r["prolong_bytes"] > 0 for r in rec[1:])
    for r, g in zip(rec[1:], levels[1:]):
        assert r["max_distance"] == (g["transfer"]["max_distance"] if r["transfer"] == "located" else None)


def test_cascade_equals_the_cascade_over_the_host():
    """Three sphere triangulations, none nested, at T = 7: the finest level of solver_socp_mesh_cascade against solver_socp warm-started
    with the host transfer of the level-2 solution (itself warm-started from level 1 the same way)."""
    check_driver_against_the_host_chain(located_sphere_levels(), ("located", "located"))


def test_mixed_hierarchy_equals_the_cascade_over_the_host():
    """Level 2 nested in level 1 (``parents``), level 3 located on level 2 (``transfer``)"""
    levels = mixed_sphere_levels()
    assert "parents" in levels[1] and "transfer" not in levels[1] and "transfer" in levels[2] and "parents" not in levels[2]
    check_driver_against_the_host_chain(levels, ("nested", "located"))


def test_every_level_converges_and_the_cost_is_the_cold_solve_s():
    """The three located sphere levels at T = 7, tol 1e-5: every level ends with all seven residuals below tol, and the finest level's
    cost is within 1e-6 relative (the project's parity budget) of the cold solve's at the same tol.  The bound comes from the oracle on
    the CPU (oracle/dots_oracle.py on these levels at tol 1e-5): its cold solve of the finest level and its solve warm-started from
    transfer_space_solution of its level-2 solution (itself started from level 1 the same way) end at costs 0.2574510992328948 and
    0.257450977886939, 4.7e-7 relative apart: within 1e-6, so 1e-6 is asserted (the nested hierarchy measured 6.6e-10)."""
    from dots_socp_amd.socp import solver_raw_mesh_cascade, solver_socp, solver_socp_mesh_cascade

    levels = located_sphere_levels()
    kw = dict(tol=CONVERGENCE_TOL, nit=20000)
    _, cold = solver_socp(7, levels[2], outputs=("mu",), **kw)
    _, hist = solver_socp_mesh_cascade(7, levels, **kw)
    rec = hist.solver_stats["mesh_cascade"]["levels"]
    c_cold, c_warm = float(cold.history["Transportation cost"][-1]), float(hist.history["Transportation cost"][-1])
    print(f"cold: {int(cold.kkt_iteration[-1]) + 1} iterations, cost {c_cold!r}; cascade: {[r['iterations'] for r in rec]} iterations, "
          f"cost {c_warm!r}; relative difference {abs(c_warm - c_cold) / abs(c_cold):.3e}; kkt_max per level {[r['kkt_max'] for r in rec]}")
    for r in rec:
        assert r["kkt_max"] < CONVERGENCE_TOL, r
    for h in (cold, hist):
        last = np.asarray(h.kkt_errors[-1], dtype=np.float64)
        assert last.shape == (7,) and np.all(np.isfinite(last)) and np.all(last < CONVERGENCE_TOL), last
    assert abs(c_warm - c_cold) <= 1e-6 * abs(c_cold)
    # the plug-in returns the transport of the finest level in DOT units
    sol, hist_p = solver_raw_mesh_cascade(7, levels, tol=1e-3, nit=4000)
    assert sol["mu"].shape == (7, 642) and sol["E"].shape == (8, 1280, 3)
    assert abs(sol["mu"].sum(axis=1) - 1.0).max() < 1e-3
    assert [r["transfer"] for r in hist_p.solver_stats["mesh_cascade"]["levels"]] == [None, "located", "located"]


def test_the_fine_factor_is_built_after_the_coarse_context_is_released(monkeypatch):
    from dots_socp_amd.device import DeviceProblem
    from dots_socp_amd.socp.solver_socp import AlmSolver

    coarse_geom, fine_geom = located_sphere_levels()[:2]
    coarse = AlmSolver(7, coarse_geom, nit=50, tol=1e-12, check_kkt_step_by_step=True)      # (every step leaves z_mid in place)
    fine = None
    try:
        for _ in range(5):
            coarse.iterate()
        coarse.finalize(download=False)
        assert coarse.dev.debug_counter(4) >= 0 and coarse.front_summary is not None      # the coarse context holds a factor
        seen = []
        setup = DeviceProblem.setup_frontal

        def spy(self, *args, **kwargs):
            before = (self.front_launches(), self.device_bytes(), bool(np.any(self.download("phi") != 0.0)))
            out = setup(self, *args, **kwargs)
            seen.append((bool(coarse.dev._h.value), before, self.front_launches()))
            return out

        monkeypatch.setattr(DeviceProblem, "setup_frontal", spy)
        fine = AlmSolver(7, fine_geom, nit=50, tol=1e-12, init_from=coarse, init_transfer=fine_geom["transfer"], release_init_from=True)
        assert len(seen) == 1
        coarse_open, (launches_before, state_bytes, filled), launches_after = seen[0]
        assert not coarse_open, "the coarse context was still open when the fine factor was built"
        # the fine context held its state, already the transferred one, and no factor; the factor arrived with this call
        assert state_bytes > 0 and filled and launches_before == -1 and launches_after > 0
        assert coarse.dev.debug_counter(4) == -1 and coarse.dev.device_bytes() == -1      # (a closed handle)
        assert fine.prolong_ms > 0
        fine.iterate()
    finally:
        coarse.close()
        if fine is not None:
            fine.close()


def raw_transfer_space(dst, src, tables, n_vertices=None, n_triangles=None, null=None, edit=None):
    """The entry point itself with the tables ``tables`` = (vsrc, vw, fsrc, csrc), nothing checked on the way; ``null``: the table passed
    as NULL; ``edit`` = (table, flat index, value): one entry replaced."""
    t = {k: a.copy() for k, a in zip(("vsrc", "vw", "fsrc", "csrc"), tables)}
    if edit is not None:
        t[edit[0]].reshape(-1)[edit[1]] = edit[2]
    d = _lib.TransferSpaceDesc()
    for k, a in t.items():
        setattr(d, k, None if k == null else a.ctypes.data_as(C.POINTER(C.c_double if k == "vw" else C.c_int32)))
    d.n_vertices = t["vsrc"].shape[0] if n_vertices is None else n_vertices
    d.n_triangles = t["fsrc"].shape[0] if n_triangles is None else n_triangles
    for i in range(4):
        d.factor[i] = 1.0
    return dst.lib.dots_transfer_space(dst._h, src._h, C.byref(d))


def test_error_codes_leave_both_contexts_usable():
    from dots_socp_amd.device import DeviceProblem

    coarse, fine, transfer = pair("torus")
    other = pair("icosphere")[1]
    mk = lambda T, g, **kw: DeviceProblem(T, g, lap_solver="modal_pcg", reorder=False, **kw)      # noqa: E731
    rng = np.random.default_rng(3)
    with mk(7, coarse) as src, mk(7, fine) as dst, mk(15, fine) as longer, mk(7, other) as alien, mk(7, fine, time_slab=(0, 2)) as slab, \
            mk(7, coarse, time_slab=(0, 2)) as src_slab:
        x = rng.standard_normal(src.shape("mu"))
        src.upload("mu", x)
        tables = cascade.transfer_row_maps(transfer)      # (neither context is renumbered)
        assert raw_transfer_space(longer, src, tables) == _lib.ERR_ARGUMENT                   # another n_time
        assert raw_transfer_space(alien, src, tables) == _lib.ERR_ARGUMENT                    # tables of another mesh
        assert raw_transfer_space(dst, src, tables, n_vertices=dst.V - 1) == _lib.ERR_ARGUMENT
        assert raw_transfer_space(dst, src, tables, n_triangles=dst.F + 4) == _lib.ERR_ARGUMENT
        for name in ("vsrc", "vw", "fsrc", "csrc"):
            assert raw_transfer_space(dst, src, tables, null=name) == _lib.ERR_ARGUMENT
        assert raw_transfer_space(dst, src, tables, edit=("vsrc", -1, src.V)) == _lib.ERR_ARGUMENT      # a row the source does not have
        assert raw_transfer_space(dst, src, tables, edit=("vsrc", 4, -1)) == _lib.ERR_ARGUMENT
        assert raw_transfer_space(dst, src, tables, edit=("fsrc", 0, src.F)) == _lib.ERR_ARGUMENT
        assert raw_transfer_space(dst, src, tables, edit=("csrc", 7, 3)) == _lib.ERR_ARGUMENT
        assert raw_transfer_space(dst, src, tables, edit=("vw", 5, -0.25)) == _lib.ERR_ARGUMENT
        assert raw_transfer_space(dst, src, tables, edit=("vw", 2, np.nan)) == _lib.ERR_ARGUMENT
        assert raw_transfer_space(dst, src, tables, edit=("vw", 2, np.inf)) == _lib.ERR_ARGUMENT
        assert raw_transfer_space(dst, dst, tables) == _lib.ERR_ARGUMENT
        assert raw_transfer_space(slab, src, tables) == _lib.ERR_STATE
        assert raw_transfer_space(dst, src_slab, tables) == _lib.ERR_STATE
        with pytest.raises(ValueError):
            longer.transfer_space_from(src, transfer)
        with pytest.raises(ValueError):
            alien.transfer_space_from(src, transfer)
        with pytest.raises(ValueError):
            dst.transfer_space_from(src, pair("icosphere")[2])
        with pytest.raises(ValueError):
            slab.transfer_space_from(src, transfer)
        with pytest.raises(ValueError):
            dst.transfer_space_from(src_slab, transfer)
        # both contexts are as they were, and the call still works
        assert np.array_equal(src.download("mu"), x) and not np.any(dst.download("mu"))
        assert raw_transfer_space(dst, src, tables) == 0
        assert np.array_equal(bits(dst.download("mu")), bits(cascade.transfer_space(x, "mu", transfer)))
        src.step(1)
        dst.step(1)


def test_source_is_brought_up_to_date_or_refused():
    """After a quiet step (z_mid not stored, a penalty division pending, carried sums set) the call refuses; after a step that keeps z_mid
    (deferred: rebuilt on demand) with a division pending it carries both out first -- it never transfers stale arrays."""
    from dots_socp_amd.device import DeviceProblem
    from dots_socp_amd.socp.solver_socp import AlmSolver

    coarse, fine, transfer = pair("torus")
    alm = AlmSolver(15, coarse, nit=100, tol=1e-12)
    try:
        for _ in range(5):
            alm.iterate()
        dev = alm.dev
        with DeviceProblem(15, fine, lap_solver="modal_pcg", reorder="nd") as dst:
            dev.step_flags(skip_z_mid=True, carry=True)
            dev.step(1, wait=False)
            alm.adjust_penalty(1.3)      # (pending: carried out by the next reader of the dual arrays)
            with pytest.raises(_lib.HipLibraryError) as err:
                dst.transfer_space_from(dev, transfer, alm.recovery_factors())
            assert err.value.status == _lib.ERR_STATE
            dev.step_flags(carry=True, kkt_sums=True)
            dev.step(1, wait=False)      # z_mid of this iterate exists, on demand
            alm.adjust_penalty(1.0 / 1.7)
            dst.transfer_space_from(dev, transfer, alm.recovery_factors())
            got = {k: dst.download(k) for k in STATE}
            want = cascade.transfer_space_solution({k: alm.recovered(k, dev.download(k)) for k in STATE}, transfer)
            for k in STATE:
                assert np.array_equal(bits(got[k]), bits(want[k])), k
            assert np.any(want["z_mid"] != 0.0) and np.any(want["beta_mid"] != 0.0)
    finally:
        alm.close()

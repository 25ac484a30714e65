"""GPU tests of the cascade in space and time at once: the fused carrier (dots_carry_spacetime) against its host specification
(cascade.carry_spacetime: space first, then time) and against the two existing kernels run one after the other through a context in
between, bit for bit; the error codes of the entry point; the driver against the same cascade over the host and, on one time grid,
against solver_socp_mesh_cascade; convergence; the order of release and factorisation.  Everything is compared on the bit pattern, so
no tolerance appears."""
import ctypes as C

import numpy as np
import pytest

from carry_checks import STATE, bits, scaled_source, with_bumps
from conftest import has_gpu
from dots_socp_amd import _lib, cascade, evaluate, meshes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]


def on_sphere(p):
    return p / np.linalg.norm(p, axis=1, keepdims=True)


def rotation(az, ax):
    """Rz(az) . Rx(ax)"""
    rz = np.array([[np.cos(az), -np.sin(az), 0.0], [np.sin(az), np.cos(az), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(ax), -np.sin(ax)], [0.0, np.sin(ax), np.cos(ax)]])
    return rz @ rx


def rotated_icosphere(level, az, ax):
    v, t = meshes.icosphere(level)
    return v @ rotation(az, ax).T, t


PAIRS = ("nested-icosphere", "nested-plane", "located-plane", "located-icosphere", "located-torus")
_pairs = {}


def pair(name):
    """(coarse geometry, fine geometry, the map as a keyword of carry_spacetime): nested icosphere(1) -> its subdivision (42 -> 162) and
    plane(4) -> its subdivision (a boundary); located plane(4) -> plane(7) (points beyond the patch), icosphere(1) -> the rotated
    icosphere(2) (no shared vertex), torus (8, 6) -> (13, 9)."""
    if name not in _pairs:
        kind, mesh = name.split("-")
        if kind == "nested":
            coarse, project = (with_bumps(*meshes.icosphere(1)), on_sphere) if mesh == "icosphere" else (with_bumps(*meshes.plane(4)), None)
            coarse, fine = meshes.refine_levels(coarse, 2, project=project)
            _pairs[name] = (coarse, fine, {"parents": fine["parents"]})
        else:
            both = {"plane": (meshes.plane(4), meshes.plane(7)), "icosphere": (meshes.icosphere(1), rotated_icosphere(2, 0.7, 0.4)),
                    "torus": (meshes.torus(8, 6), meshes.torus(13, 9))}[mesh]
            coarse, fine = with_bumps(*both[0]), with_bumps(*both[1])
            _pairs[name] = (coarse, fine, {"transfer": cascade.mesh_transfer(coarse, fine)})
    return _pairs[name]


def pitch(n_time):
    return max(8, 1 << int(np.ceil(np.log2(n_time + 1))))


def expected_bytes(dst, src, how):
    rows = 8 * dst.V + 42 * dst.F
    src_rows = 8 * src.V + 42 * src.F if "parents" in how else 24 * dst.V + 42 * dst.F
    return 8 * (pitch(dst.T) * rows + pitch(src.T) * src_rows)


def check_spacetime(name, n_src, n_dst, src_orders=(True, False), dst_orders=("nd", False)):
    """The fused carrier from a scaled random source against an upload of the host specification of its recovered solution: all twelve
    arrays bit for bit, and -- where a context without a factor can step -- once more after one step from either, which the columns
    beyond the arrays' time points take part in."""
    from dots_socp_amd.device import DeviceProblem

    coarse, fine, how = pair(name)
    for src_order in src_orders:
        alm = scaled_source(coarse, n_src, src_order, seed=100 * n_src + n_dst)
        try:
            assert (alm.dev.plan.perm_vert is not None) == bool(src_order)
            want = cascade.carry_spacetime_solution({k: alm.recovered(k, alm.dev.download(k)) for k in STATE}, n_src, n_dst, **how)
            for dst_order in dst_orders:
                with DeviceProblem(n_dst, fine, lap_solver="modal_pcg", reorder=dst_order) as dst, \
                        DeviceProblem(n_dst, fine, lap_solver="modal_pcg", reorder=dst_order) as ref:
                    ms = dst.carry_spacetime_from(alm.dev, alm.recovery_factors(), **how)
                    assert ms >= 0.0 and dst.prolong_bytes == expected_bytes(dst, alm.dev, how)
                    for k in STATE:
                        ref.upload(k, want[k])
                    for k in STATE:
                        got, up = dst.download(k), ref.download(k)
                        assert got.shape == want[k].shape
                        assert np.array_equal(bits(got), bits(up)), (k, src_order, dst_order, float(np.max(np.abs(got - up))))
                        assert np.array_equal(bits(got), bits(want[k])), (k, src_order, dst_order)
                    if n_dst + 1 <= 256:      # (above, only a context with a factor steps)
                        for dev in (dst, ref):
                            dev.step(1)
                        for k in STATE:
                            assert np.array_equal(bits(dst.download(k)), bits(ref.download(k))), (k, "after a step", src_order, dst_order)
        finally:
            alm.close()


@pytest.mark.parametrize("name", PAIRS)
@pytest.mark.parametrize("grids", [(1, 3), (3, 7), (5, 7), (6, 13), (15, 31), (31, 7)], ids=lambda g: f"{g[0]}to{g[1]}")
def test_carrier_matches_the_host_specification(name, grids):
    """One source interval; 3 -> 7; the same pitch on both sides; padding on both sides; 15 -> 31; coarsening.  Both device numberings on
    either side."""
    check_spacetime(name, *grids)


@pytest.mark.parametrize("name", PAIRS)
def test_carrier_in_column_chunks(name):
    """127 -> 256: T + 1 = 257 nodes, a destination pitch of 512: the rows of a pass are written in two chunks of 256 columns"""
    check_spacetime(name, 127, 256, src_orders=(True,), dst_orders=("nd",))


def test_carrier_at_the_largest_pitches():
    """255 -> 1023: a source pitch of 256 and the largest destination pitch, 1024 (two rows per pass)"""
    check_spacetime("located-icosphere", 255, 1023, src_orders=(True,), dst_orders=("nd",))


@pytest.mark.parametrize("name,grids", [("nested-icosphere", (7, 15)), ("located-torus", (6, 13))])
def test_carrier_equals_the_two_existing_kernels(name, grids):
    """The fused call against two calls into the same kernel family: the carrier in space (the run kernel) into a context on the fine mesh
    at the source's n_time, then dots_prolong_time (the staged kernel with the same row as its space stage) with factors of 1 from there"""
    from dots_socp_amd.device import DeviceProblem

    n_src, n_dst = grids
    coarse, fine, how = pair(name)
    alm = scaled_source(coarse, n_src, True, seed=7)
    try:
        factors = alm.recovery_factors()
        with DeviceProblem(n_dst, fine, lap_solver="modal_pcg", reorder="nd") as fused, \
                DeviceProblem(n_src, fine, lap_solver="modal_pcg", reorder="nd") as between, \
                DeviceProblem(n_dst, fine, lap_solver="modal_pcg", reorder="nd") as chained:
            fused.carry_spacetime_from(alm.dev, factors, **how)
            if "parents" in how:
                between.prolong_space_from(alm.dev, how["parents"], factors)
            else:
                between.transfer_space_from(alm.dev, how["transfer"], factors)
            chained.prolong_from(between)
            for k in STATE:
                a, b = fused.download(k), chained.download(k)
                assert np.any(a != 0.0) and np.array_equal(bits(a), bits(b)), (k, float(np.max(np.abs(a - b))))
    finally:
        alm.close()


def raw_carry(dst, src, tables, n_vertices=None, n_triangles=None, null=None, edit=None):
    """The entry point itself with ``tables`` (a dict of the eight tables; vw / csrc may be None), nothing checked on the way; ``null``:
    the table passed as NULL; ``edit`` = (table, flat index, value): one entry replaced."""
    t = {k: (None if a is None else a.copy()) for k, a in tables.items()}
    if edit is not None:
        t[edit[0]].reshape(-1)[edit[1]] = edit[2]
    d = _lib.CarrySpacetimeDesc()
    for k, a in t.items():
        setattr(d, k, None if (k == null or a is None) else a.ctypes.data_as(C.POINTER(C.c_double if k in ("vw", "node_w", "interval_w") else C.c_int32)))
    d.n_vertices = t["vsrc"].shape[0] if n_vertices is None else n_vertices
    d.n_triangles = t["fsrc"].shape[0] if n_triangles is None else n_triangles
    for i in range(4):
        d.factor[i] = 1.0
    return dst.lib.dots_carry_spacetime(dst._h, src._h, C.byref(d))


def tables_of(how, n_src, n_dst):
    nj, nw = cascade.time_weights(n_src, n_dst, node=True)
    ij, iw = cascade.time_weights(n_src, n_dst, node=False)
    t = {"node_j": nj, "node_w": nw, "interval_j": ij, "interval_w": iw}
    if "parents" in how:
        coarse = how["coarse"]
        vsrc, fsrc = cascade.space_row_maps(how["parents"], coarse["vertices"].shape[0], coarse["triangles"].shape[0])
        return dict(t, vsrc=vsrc, vw=None, fsrc=fsrc, csrc=None)
    vsrc, vw, fsrc, csrc = cascade.transfer_row_maps(how["transfer"])
    return dict(t, vsrc=vsrc, vw=vw, fsrc=fsrc, csrc=csrc)


@pytest.mark.parametrize("name", ["nested-icosphere", "located-torus"])
def test_error_codes_leave_both_contexts_as_they_were(name):
    """Every refusal comes from the host-side validation, before a table is copied or a kernel launched"""
    from dots_socp_amd.device import DeviceProblem

    coarse, fine, how = pair(name)
    located = "transfer" in how
    mk = lambda T, g, **kw: DeviceProblem(T, g, lap_solver="modal_pcg", reorder=False, **kw)      # noqa: E731
    rng = np.random.default_rng(3)
    with mk(7, coarse) as src, mk(15, fine) as dst, mk(7, fine) as same, mk(15, coarse) as alien, mk(15, fine, time_slab=(0, 2)) as slab:
        before = {}
        for dev, tag in ((src, "src"), (dst, "dst")):
            for k in STATE:
                x = rng.standard_normal(dev.shape(k))
                dev.upload(k, x)
                before[tag, k] = dev.download(k)
        tab = tables_of(dict(how, coarse=coarse), 7, 15)
        bad = _lib.ERR_ARGUMENT
        assert raw_carry(same, src, tables_of(dict(how, coarse=coarse), 7, 7)) == bad         # one time grid: the carriers in space
        message = dst.lib.dots_last_error().decode()
        assert "dots_prolong_space" in message and "dots_transfer_space" in message, message      # (names the carriers in space)
        assert raw_carry(dst, dst, tab) == bad
        for k in ("node_j", "node_w", "interval_j", "interval_w", "vsrc", "fsrc"):
            assert raw_carry(dst, src, tab, null=k) == bad, k
        assert raw_carry(alien, src, tab) == bad                                               # tables of another mesh
        assert raw_carry(dst, src, tab, n_vertices=dst.V - 1) == bad
        assert raw_carry(dst, src, tab, n_triangles=dst.F + 4) == bad
        assert raw_carry(dst, src, tab, edit=("vsrc", -1, src.V)) == bad                       # a row the source does not have
        assert raw_carry(dst, src, tab, edit=("vsrc", 4, -1)) == bad
        assert raw_carry(dst, src, tab, edit=("fsrc", 0, src.F)) == bad
        assert raw_carry(dst, src, tab, edit=("fsrc", 3, -2)) == bad
        assert raw_carry(dst, src, tab, edit=("node_j", 5, 7)) == bad                          # j + 1 would be past the last source node
        assert raw_carry(dst, src, tab, edit=("interval_j", 0, -1)) == bad
        assert raw_carry(dst, src, tab, edit=("interval_j", 14, 6)) == bad
        assert raw_carry(dst, src, tab, edit=("node_w", 2, 1.5)) == bad
        assert raw_carry(dst, src, tab, edit=("interval_w", 2, np.nan)) == bad
        if located:
            assert raw_carry(dst, src, tab, edit=("csrc", 7, 3)) == bad
            assert raw_carry(dst, src, tab, edit=("csrc", 0, -1)) == bad
            assert raw_carry(dst, src, tab, edit=("vw", 5, -0.25)) == bad
            assert raw_carry(dst, src, tab, edit=("vw", 2, np.inf)) == bad
        assert raw_carry(slab, src, tab) == _lib.ERR_STATE
        maps = {k: v for k, v in how.items()}
        with pytest.raises(ValueError):
            same.carry_spacetime_from(src, **maps)                                             # one time grid
        with pytest.raises(ValueError):
            alien.carry_spacetime_from(src, **maps)
        with pytest.raises(ValueError):
            slab.carry_spacetime_from(src, **maps)
        with pytest.raises(ValueError):
            dst.carry_spacetime_from(src)                                                      # neither map
        with pytest.raises(ValueError):
            dst.carry_spacetime_from(src, parents=pair("nested-icosphere")[2]["parents"], transfer=pair("located-torus")[2]["transfer"])
        # both contexts are as they were, and the call still works
        for dev, tag in ((src, "src"), (dst, "dst")):
            for k in STATE:
                assert np.array_equal(bits(dev.download(k)), bits(before[tag, k])), (tag, k)
        assert raw_carry(dst, src, tab) == 0
        want = cascade.carry_spacetime_solution({k: before["src", k] for k in STATE}, 7, 15, **how)
        for k in STATE:
            assert np.array_equal(bits(dst.download(k)), bits(want[k])), k
        src.step(1)
        dst.step(1)


def test_a_stale_z_mid_is_refused_and_a_deferred_one_is_rebuilt():
    """After a quiet step (z_mid not stored) the call refuses with DOTS_ERR_STATE and the destination keeps what it held; after a step
    that keeps z_mid on demand, with a penalty division pending, both are carried out first"""
    from dots_socp_amd.device import DeviceProblem
    from dots_socp_amd.socp.solver_socp import AlmSolver

    coarse, fine, how = pair("located-torus")
    alm = AlmSolver(7, coarse, nit=100, tol=1e-12)
    try:
        for _ in range(5):
            alm.iterate()
        dev = alm.dev
        with DeviceProblem(15, fine, lap_solver="modal_pcg", reorder="nd") as dst:
            x = np.random.default_rng(5).standard_normal(dst.shape("mu"))
            dst.upload("mu", x)
            dev.step_flags(skip_z_mid=True, carry=True)
            dev.step(1, wait=False)
            alm.adjust_penalty(1.3)      # (pending: carried out by the next reader of the dual arrays)
            with pytest.raises(_lib.HipLibraryError) as err:
                dst.carry_spacetime_from(dev, alm.recovery_factors(), **how)
            assert err.value.status == _lib.ERR_STATE
            assert np.array_equal(bits(dst.download("mu")), bits(x))
            dev.step_flags(carry=True, kkt_sums=True)
            dev.step(1, wait=False)      # z_mid of this iterate exists, on demand
            alm.adjust_penalty(1.0 / 1.7)
            dst.carry_spacetime_from(dev, alm.recovery_factors(), **how)
            got = {k: dst.download(k) for k in STATE}
            want = cascade.carry_spacetime_solution({k: alm.recovered(k, dev.download(k)) for k in STATE}, 7, 15, **how)
            for k in STATE:
                assert np.array_equal(bits(got[k]), bits(want[k])), k
            assert np.any(want["z_mid"] != 0.0) and np.any(want["beta_mid"] != 0.0)
    finally:
        alm.close()


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def sphere_parts():
    """The normalised icosphere(1), the map that normalised it, and three bumps as a function of (vertices, area_vertices) around the
    POINTS of three far-apart coarse vertices, so that every triangulation gets the same densities."""
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
    centre = geom["vertices"].mean(axis=0)
    radius = np.linalg.norm(geom["vertices"][0] - centre)
    project = lambda p: centre + radius * on_sphere(p - centre)      # noqa: E731
    return geom, place, dens, project


_levels = {}


def sphere_levels(kind):
    """Icosphere 42 / 162 / 642 with the three bumps: "nested" (1 -> 2 -> 3 by subdivision) or "mixed" (1 -> 2 nested, then the rotated
    icosphere(3) located on level 2)"""
    if kind not in _levels:
        geom, place, dens, project = sphere_parts()
        if kind == "nested":
            _levels[kind] = meshes.refine_levels(geom, 3, project=project, densities=dens)
        else:
            nested = meshes.refine_levels(geom, 2, project=project, densities=dens)
            top = meshes.make_geometry(place(rotated_icosphere(3, -0.3, 1.1)[0]), meshes.icosphere(3)[1], normalize=False)[0]
            _levels[kind] = meshes.link_levels(nested + [top], densities=dens)
    return _levels[kind]


def level_map(geom):
    return {"parents": geom["parents"]} if geom.get("parents") is not None else {"transfer": geom["transfer"]}


def assert_same_run(sol_c, hist_c, sol_h, hist_h):
    assert int(hist_c.kkt_iteration[-1]) == int(hist_h.kkt_iteration[-1])
    assert hist_c.kkt_errors.shape == hist_h.kkt_errors.shape
    assert np.array_equal(hist_c.kkt_errors, hist_h.kkt_errors, equal_nan=True)
    for key in ("Transportation cost", "Objective value"):
        assert np.array_equal(hist_c.history[key], hist_h.history[key], equal_nan=True), key
    for k in STATE:
        assert np.array_equal(bits(sol_c[k]), bits(sol_h[k])), (k, float(np.max(np.abs(sol_c[k] - sol_h[k]))))


@pytest.mark.parametrize("kind,kinds", [("nested", ("nested", "nested")), ("mixed", ("nested", "located"))])
def test_driver_equals_the_cascade_over_the_host(kind, kinds):
    """levels = [3, 7, 15] on 42 / 162 / 642 vertices: the finest level of the driver against solver_socp warm-started with
    carry_spacetime_solution of the level below (itself started from the coarsest the same way)"""
    from dots_socp_amd.socp import solver_socp, solver_socp_spacetime_cascade

    geoms, grids = sphere_levels(kind), [3, 7, 15]
    kw = dict(tol=1e-3, nit=4000)
    sol, _ = solver_socp(3, geoms[0], **kw)
    sol, _ = solver_socp(7, geoms[1], init_solution=cascade.carry_spacetime_solution(sol, 3, 7, **level_map(geoms[1])), **kw)
    sol_h, hist_h = solver_socp(15, geoms[2], init_solution=cascade.carry_spacetime_solution(sol, 7, 15, **level_map(geoms[2])), **kw)
    sol_c, hist_c = solver_socp_spacetime_cascade(15, geoms, levels=grids, **kw)
    assert_same_run(sol_c, hist_c, sol_h, hist_h)
    rec = hist_c.solver_stats["spacetime_cascade"]["levels"]
    assert [r["n_time"] for r in rec] == grids and [r["n_vertices"] for r in rec] == [42, 162, 642]
    assert [r["transfer"] for r in rec] == [None] + list(kinds)
    assert rec[2]["iterations"] == int(hist_h.kkt_iteration[-1]) + 1
    assert rec[0]["prolong_ms"] is None and all(r["prolong_ms"] > 0 and r["prolong_bytes"] > 0 for r in rec[1:])
    assert "mesh_cascade" not in hist_c.solver_stats


def test_one_time_grid_is_the_mesh_cascade():
    from dots_socp_amd.socp import solver_socp_mesh_cascade, solver_socp_spacetime_cascade

    geoms = sphere_levels("nested")
    kw = dict(tol=1e-3, nit=4000)
    sol_m, hist_m = solver_socp_mesh_cascade(7, geoms, **kw)
    sol_c, hist_c = solver_socp_spacetime_cascade(7, geoms, levels=[7, 7, 7], **kw)
    assert_same_run(sol_c, hist_c, sol_m, hist_m)
    rec, rec_m = hist_c.solver_stats["spacetime_cascade"]["levels"], hist_m.solver_stats["mesh_cascade"]["levels"]
    assert [r["n_time"] for r in rec] == [7, 7, 7]
    for a, b in zip(rec, rec_m):
        assert all(a[k] == b[k] for k in ("n_vertices", "n_triangles", "iterations", "prolong_bytes", "cost", "kkt_max", "transfer"))


def test_finest_level_converges_and_the_plug_ins_agree():
    """Default levels (T = 31 on three meshes: 15, 15, 31 -- one step on one grid, one diagonal) at tol 1e-3: the finest level ends with
    all seven residuals below tol and every layer of mu carries the unit mass to 1e-3, as the existing cascades' tests ask; the plug-in
    with the read-out on the device returns what the one over the host does, bit for bit."""
    from dots_socp_amd.socp import solver_raw_spacetime_cascade, solver_socp_spacetime_cascade, solver_spacetime_cascade

    geoms = sphere_levels("nested")
    tol = 1e-3
    _, hist = solver_socp_spacetime_cascade(31, geoms, tol=tol, nit=4000)
    rec = hist.solver_stats["spacetime_cascade"]["levels"]
    assert [r["n_time"] for r in rec] == [15, 15, 31]
    last = np.asarray(hist.kkt_errors[-1], dtype=np.float64)
    print(f"iterations per level {[r['iterations'] for r in rec]}, kkt_max per level {[r['kkt_max'] for r in rec]}, last residuals {last}")
    assert last.shape == (7,) and np.all(np.isfinite(last)) and np.all(last < tol), last
    sol, hist_p = solver_raw_spacetime_cascade(31, geoms, tol=tol, nit=4000)
    assert sol["mu"].shape == (31, 642) and sol["E"].shape == (32, 1280, 3)
    assert abs(sol["mu"].sum(axis=1) - 1.0).max() < 1e-3 and evaluate.check_mass_conservation(sol["mu"]) < 1e-3
    assert evaluate.mass_conservation_from_layers(hist_p.solver_stats["readout"]["layer_mass"]) < 1e-3
    dev, _ = solver_spacetime_cascade(15, geoms, levels=[3, 7, 15], tol=tol, nit=4000, readout="device")
    host, _ = solver_spacetime_cascade(15, geoms, levels=[3, 7, 15], tol=tol, nit=4000, readout="host")
    assert dev["mu"].shape == (16, 642)
    for k in ("mu", "E"):
        assert np.array_equal(bits(dev[k]), bits(host[k])), k


def test_the_fine_factor_is_built_after_the_coarse_context_is_released(monkeypatch):
    from dots_socp_amd.device import DeviceProblem
    from dots_socp_amd.socp.solver_socp import AlmSolver

    coarse_geom, fine_geom = sphere_levels("nested")[:2]
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
        fine = AlmSolver(15, fine_geom, nit=50, tol=1e-12, init_from=coarse, init_parents=fine_geom["parents"], init_regrid=True,
                         release_init_from=True)
        assert len(seen) == 1
        coarse_open, (launches_before, state_bytes, filled), launches_after = seen[0]
        assert not coarse_open, "the coarse context was still open when the fine factor was built"
        # the fine context held its state, already the carried one, and no factor; the factor arrived with this call
        assert state_bytes > 0 and filled and launches_before == -1 and launches_after > 0
        assert coarse.dev.debug_counter(4) == -1 and coarse.dev.device_bytes() == -1      # (a closed handle)
        assert fine.prolong_ms > 0 and fine.n_time == 15 and fine.dev.T == 15
        fine.iterate()
    finally:
        coarse.close()
        if fine is not None:
            fine.close()

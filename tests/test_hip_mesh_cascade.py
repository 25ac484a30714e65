"""GPU tests of the coarse-to-fine cascade in space: the transfer of the state from a mesh to its nested refinement on the device
(dots_prolong_space) against its host specification (cascade.prolong_space) bit for bit at every pitch and under every pairing of
device numberings, the driver against the same cascade over the host, convergence against the cold solve, the order of release and
factorisation, and the error codes of the entry point."""
import ctypes as C

import numpy as np
import pytest

from carry_checks import STATE, bits, check_carry, with_bumps
from conftest import has_gpu
from dots_socp_amd import _lib, cascade, meshes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

CONVERGENCE_TOL = 1e-5


def on_sphere(p):
    return p / np.linalg.norm(p, axis=1, keepdims=True)


_pairs = {}


def pair(name):
    """(coarse geometry, its refinement with ``parents``): icosphere 1 -> 2 (42 -> 162 vertices), torus (8, 6) -> (16, 12), and the
    plane(4) patch -> its subdivision (a mesh with boundary)."""
    if name not in _pairs:
        if name == "icosphere":
            coarse, project = with_bumps(*meshes.icosphere(1)), on_sphere
        elif name == "torus":
            coarse, project = with_bumps(*meshes.torus(8, 6)), meshes.snap_projection(meshes.torus(16, 12)[0])
        else:
            coarse, project = with_bumps(*meshes.plane(4)), None
        _pairs[name] = tuple(meshes.refine_levels(coarse, 2, project=project))
    return _pairs[name]


def sphere_levels(n):
    """Icosphere 1 -> ... with the same three bumps on every level (the centres are vertices of the coarsest level)."""
    geom, _ = meshes.make_geometry(*meshes.icosphere(1))
    c = meshes.farthest_vertices(geom["vertices"], 0, 3)
    centre = geom["vertices"].mean(axis=0)
    radius = np.linalg.norm(geom["vertices"][0] - centre)
    dens = lambda v, a: (meshes.bump_density(v, a, [c[0]], 0.6, 0.2), meshes.bump_density(v, a, [c[1], c[2]], 0.6, 0.2))      # noqa: E731
    geom["mu0"], geom["mu1"] = dens(geom["vertices"], geom["area_vertices"])
    return meshes.refine_levels(geom, n, project=lambda p: centre + radius * on_sphere(p - centre), densities=dens)


@pytest.mark.parametrize("name", ["icosphere", "torus", "plane"])
@pytest.mark.parametrize("n_time", [1, 3, 6, 15, 31])
def test_prolongation_matches_the_host_specification(name, n_time):
    check_pair(name, n_time)


def test_prolongation_in_column_chunks():
    """T + 1 = 257 nodes: a pitch of 512, rows walked in two chunks of 256 columns."""
    check_pair("icosphere", 256, src_orders=(True,), dst_orders=("nd", False))


def check_pair(name, n_time, **orders):
    coarse, fine = pair(name)
    parents = fine["parents"]
    check_carry(coarse, fine, n_time, carry=lambda dst, src, factors: dst.prolong_space_from(src, parents, factors),
                host=lambda solution: cascade.prolong_space_solution(solution, parents),
                bytes_ok=lambda dst, pitch: dst.prolong_bytes > 0, **orders)


def test_cascade_equals_the_cascade_over_the_host():
    """Icosphere 1 -> 2 -> 3 at T = 7: the finest level of solver_socp_mesh_cascade against solver_socp warm-started with the host
    prolongation of the level-2 solution (itself warm-started from level 1 the same way)."""
    from dots_socp_amd.socp import solver_socp, solver_socp_mesh_cascade

    levels = sphere_levels(3)
    kw = dict(tol=1e-3, nit=4000)
    sol, _ = solver_socp(7, levels[0], **kw)
    sol, _ = solver_socp(7, levels[1], init_solution=cascade.prolong_space_solution(sol, levels[1]["parents"]), **kw)
    sol_h, hist_h = solver_socp(7, levels[2], init_solution=cascade.prolong_space_solution(sol, levels[2]["parents"]), **kw)
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
    assert rec[0]["prolong_ms"] is None and all(r["prolong_ms"] > 0 and r["prolong_bytes"] > 0 for r in rec[1:])


def test_every_level_converges_and_the_cost_is_the_cold_solve_s():
    """Icosphere 1 -> 2 -> 3 at T = 7, tol 1e-5: every level ends with all seven residuals below tol, and the finest level's cost is
    within 1e-6 relative (the project's parity budget) of the cold solve's at the same tol.  The tolerance is the one at which two
    converged runs of the oracle from different starts (cold; warm from the prolonged level-2 solution) agree to 1e-6 on this
    problem: 6.6e-10 relative at tol 1e-5 (5.8e-5 at 1e-3 and 1.5e-5 at 1e-4, which is why tol is not 1e-3)."""
    from dots_socp_amd.socp import solver_raw_mesh_cascade, solver_socp, solver_socp_mesh_cascade

    levels = sphere_levels(3)
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
    assert len(hist_p.solver_stats["mesh_cascade"]["levels"]) == 3


def test_the_fine_factor_is_built_after_the_coarse_context_is_released(monkeypatch):
    from dots_socp_amd.device import DeviceProblem
    from dots_socp_amd.socp.solver_socp import AlmSolver

    coarse_geom, fine_geom = sphere_levels(2)
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
        fine = AlmSolver(7, fine_geom, nit=50, tol=1e-12, init_from=coarse, init_parents=fine_geom["parents"], release_init_from=True)
        assert len(seen) == 1
        coarse_open, (launches_before, state_bytes, filled), launches_after = seen[0]
        assert not coarse_open, "the coarse context was still open when the fine factor was built"
        # the fine context held its state, already the prolonged one, and no factor; the factor arrived with this call
        assert state_bytes > 0 and filled and launches_before == -1 and launches_after > 0
        assert coarse.dev.debug_counter(4) == -1 and coarse.dev.device_bytes() == -1      # (a closed handle)
        assert fine.prolong_ms > 0
        fine.iterate()
    finally:
        coarse.close()
        if fine is not None:
            fine.close()


def raw_prolong_space(dst, src, maps, n_vertices=None, n_triangles=None, null_map=False, bad_entry=None):
    """The entry point itself with the row maps ``maps`` = (vmap, fmap), nothing checked on the way"""
    vmap, fmap = maps[0].copy(), maps[1].copy()
    if bad_entry is not None:
        vmap[-1, 1] = bad_entry
    d = _lib.ProlongSpaceDesc()
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731
    d.vmap, d.fmap = p(vmap), (None if null_map else p(fmap))
    d.n_vertices = vmap.shape[0] if n_vertices is None else n_vertices
    d.n_triangles = fmap.shape[0] if n_triangles is None else n_triangles
    for i in range(4):
        d.factor[i] = 1.0
    return dst.lib.dots_prolong_space(dst._h, src._h, C.byref(d))


def test_error_codes_leave_both_contexts_usable():
    from dots_socp_amd.device import DeviceProblem

    coarse, fine = pair("torus")
    other = pair("icosphere")[1]
    parents = real_parents = fine["parents"]
    mk = lambda T, g, **kw: DeviceProblem(T, g, lap_solver="modal_pcg", reorder=False, **kw)      # noqa: E731
    rng = np.random.default_rng(3)
    with mk(7, coarse) as src, mk(7, fine) as dst, mk(15, fine) as longer, mk(7, other) as alien, mk(7, fine, time_slab=(0, 2)) as slab:
        x = rng.standard_normal(src.shape("mu"))
        src.upload("mu", x)
        parents = cascade.space_row_maps(parents, src.V, src.F)      # (neither context is renumbered)
        assert raw_prolong_space(longer, src, parents) == _lib.ERR_ARGUMENT                   # another n_time
        assert raw_prolong_space(alien, src, parents) == _lib.ERR_ARGUMENT                    # parents of another mesh
        assert raw_prolong_space(dst, src, parents, n_vertices=dst.V - 1) == _lib.ERR_ARGUMENT
        assert raw_prolong_space(dst, src, parents, n_triangles=dst.F + 4) == _lib.ERR_ARGUMENT
        assert raw_prolong_space(dst, src, parents, null_map=True) == _lib.ERR_ARGUMENT
        assert raw_prolong_space(dst, src, parents, bad_entry=src.V) == _lib.ERR_ARGUMENT      # a row the source does not have
        assert raw_prolong_space(dst, dst, parents) == _lib.ERR_ARGUMENT
        assert raw_prolong_space(slab, src, parents) == _lib.ERR_STATE
        with pytest.raises(ValueError):
            longer.prolong_space_from(src, real_parents)
        with pytest.raises(ValueError):
            alien.prolong_space_from(src, real_parents)
        with pytest.raises(ValueError):
            dst.prolong_space_from(src, pair("icosphere")[1]["parents"])
        with pytest.raises(ValueError):
            slab.prolong_space_from(src, real_parents)
        # both contexts are as they were, and the call still works
        assert np.array_equal(src.download("mu"), x) and not np.any(dst.download("mu"))
        assert raw_prolong_space(dst, src, parents) == 0
        assert np.array_equal(bits(dst.download("mu")), bits(cascade.prolong_space(x, "mu", real_parents)))
        src.step(1)
        dst.step(1)

"""Host-side checks of the batched direct solve (no GPU): the library exports the entry points, the header documents them, and the
Python wrapper rejects a malformed batch before it touches a device."""
import os

import numpy as np
import pytest

from dots_socp_amd import _lib, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_batched_entry_points():
    lib = _lib.load(host_only=True)
    for name in ("dots_front_share", "dots_laplacian_solve_many"):
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 7      # additions only: the ABI version stays


def test_header_declares_the_batched_entry_points():
    with open(os.path.join(ROOT, "include", "dots_socp_hip.h")) as fh:
        text = fh.read()
    assert "int dots_front_share(dots_ctx *ctx, dots_ctx *owner);" in text
    assert "int dots_laplacian_solve_many(dots_ctx *const *ctxs, int n, const double *const *host_in, double *const *host_out);" in text


class _Shape:
    """stands in for a DeviceProblem: only the shape is asked for before the batch is validated"""
    lib = None

    def __init__(self, shape):
        self._shape = shape

    def shape(self, name):
        return self._shape


def test_wrapper_rejects_malformed_batches():
    with pytest.raises(ValueError):
        device.laplacian_solve_many([], [])
    with pytest.raises(ValueError):
        device.laplacian_solve_many([_Shape((4, 3))], [np.zeros((4, 3)), np.zeros((4, 3))])
    with pytest.raises(ValueError, match="expected shape"):
        device.laplacian_solve_many([_Shape((4, 3))], [np.zeros((3, 4))])


def test_batch_width_switch_is_known():
    assert "DOTS_FRONT_NR" in _lib.KNOWN_ENV
    for name in ("dots_step_many", "dots_bench_many"):
        assert name in _lib.EXPORTS


def _mesh():
    from dots_socp_amd import meshes

    geom, _ = meshes.example("torus", nu=12, nv=8)
    return geom


def test_solver_socp_many_checks_its_problems_before_any_device():
    from dots_socp_amd.socp import solver_socp_many

    geom = _mesh()
    V = np.asarray(geom["vertices"]).shape[0]
    mu = np.full(V, 1.0 / V)
    p = dict(mu0=mu, mu1=mu)
    with pytest.raises(ValueError, match="another mesh"):
        moved = np.asarray(geom["vertices"]) + 0.1
        solver_socp_many(5, geom, [p, dict(p, vertices=moved)])
    with pytest.raises(ValueError, match="eps"):
        solver_socp_many(5, geom, [p, dict(p, eps=1e-3)])
    for key in ("lap_solver", "reorder", "nd_leaf", "device"):
        with pytest.raises(ValueError):
            solver_socp_many(5, geom, [dict(p, **{key: 0})])
    for solver in ("modal_pcg", "spacetime_pcg"):
        with pytest.raises(ValueError, match="modal_direct"):
            solver_socp_many(5, geom, [p], lap_solver=solver)
    with pytest.raises(ValueError, match="unknown per-problem option"):
        solver_socp_many(5, geom, [dict(p, colour="red")])
    with pytest.raises(ValueError, match="unknown option"):
        solver_socp_many(5, geom, [p], colour="red")
    with pytest.raises(ValueError, match="one entry per vertex"):
        solver_socp_many(5, geom, [dict(p, mu0=mu[:-1])])
    with pytest.raises(ValueError):
        solver_socp_many(5, geom, [])


@pytest.mark.parametrize("reorder", ["nd", True, False])
def test_reused_plan_equals_build_plan(reorder):
    from dots_socp_amd import meshes
    from dots_socp_amd.geometry import build_plan, plan_with_densities

    geom = _mesh()
    v = np.asarray(geom["vertices"])
    av = meshes.vertex_areas(v.shape[0], geom["triangles"], meshes.triangle_areas(v, geom["triangles"]))
    mu0, mu1 = meshes.bump_density(v, av, [0]), meshes.bump_density(v, av, [v.shape[0] // 2])
    base = build_plan(7, geom, reorder=reorder)
    reused = plan_with_densities(base, mu0, mu1)
    fresh = build_plan(7, {**geom, "mu0": mu0, "mu1": mu1}, reorder=reorder)
    assert np.array_equal(reused.mu0, fresh.mu0) and np.array_equal(reused.mu1, fresh.mu1)
    if reorder:
        assert np.array_equal(reused.perm_vert, fresh.perm_vert) and np.array_equal(reused.perm_tri, fresh.perm_tri)
    for k in ("triangles", "lap_rowptr", "lap_col", "lap_val", "mass_vert", "hat_grad", "time_modes"):
        assert getattr(reused, k) is getattr(base, k)      # shared, not copied
        assert np.array_equal(getattr(reused, k), getattr(fresh, k)), k
    assert reused.dissection is base.dissection

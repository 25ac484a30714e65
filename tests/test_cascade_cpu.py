"""Host-side checks of the coarse-to-fine time cascade (no GPU): the library exports the transfer between two time grids, the
interpolation specified in dots_socp_amd/cascade.py has the properties a prolongation must have, the driver rejects malformed calls
before it touches a device, and the scheme itself -- run with the oracle and ``prolong_time`` -- pays."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, load_oracle
from dots_socp_amd import _lib, cascade, meshes

PAIRS = [(1, 4), (7, 15), (15, 31), (20, 50), (31, 63), (50, 20)]
NODE = ("phi", "B", "E")
STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")
V, F = 5, 4


def shape_of(name, n):
    return {"phi": (n + 1, V), "B": (n + 1, F, 3), "E": (n + 1, F, 3), "z_mid": (n, 2, 3, F, 3), "beta_mid": (n, 2, 3, F, 3)}.get(name, (n, V))


def times(name, n):
    return np.arange(n + 1) / n if name in NODE else (np.arange(n) + 0.5) / n


# ---------------------------------------------------------------------------- C ABI
def test_library_exports_the_prolongation():
    lib = _lib.load(host_only=True)
    assert "dots_prolong_time" in _lib.EXPORTS
    assert hasattr(lib, "dots_prolong_time")
    assert _lib.ABI_VERSION == 7      # an addition: the ABI version stays


def test_header_declares_the_prolongation(tmp_path):
    with open(os.path.join(ROOT, "include", "dots_socp_hip.h")) as fh:
        text = fh.read()
    assert "int dots_prolong_time(dots_ctx *dst, dots_ctx *src, const dots_prolong_desc *desc);" in text
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dots_socp_hip.h"\n'
                   'int main(void){printf("%zu %zu %zu\\n", sizeof(dots_prolong_desc), offsetof(dots_prolong_desc, factor),'
                   " offsetof(dots_prolong_desc, ms)); return 0;}\n")
    exe = tmp_path / "probe"
    assert os.system(f"gcc -I{ROOT}/include {src} -o {exe}") == 0
    out = [int(x) for x in os.popen(str(exe)).read().split()]
    assert out == [ctypes.sizeof(_lib.ProlongDesc), _lib.ProlongDesc.factor.offset, _lib.ProlongDesc.ms.offset]


# ---------------------------------------------------------------------------- the interpolation
@pytest.mark.parametrize("n_src,n_dst", PAIRS)
def test_time_weights_are_the_specified_tables(n_src, n_dst):
    for node in (True, False):
        j, w = cascade.time_weights(n_src, n_dst, node)
        assert j.dtype == np.int32 and w.dtype == np.float64
        n_pts = n_src + 1 if node else n_src
        assert j.shape == w.shape == ((n_dst + 1 if node else n_dst),)
        assert j.min() >= 0 and j.max() <= max(n_pts - 2, 0) and w.min() >= 0.0 and w.max() <= 1.0
        if n_pts > 1:      # the formula of the specification, literally
            ts = np.arange(n_src + 1) / n_src if node else (np.arange(n_src) + 0.5) / n_src
            td = np.arange(n_dst + 1) / n_dst if node else (np.arange(n_dst) + 0.5) / n_dst
            jj = np.clip(np.searchsorted(ts, td, "right") - 1, 0, len(ts) - 2)
            ww = np.clip((td - ts[jj]) / (ts[jj + 1] - ts[jj]), 0, 1)
            assert np.array_equal(j, jj) and np.array_equal(w, ww)
        else:
            assert not j.any() and not w.any()


@pytest.mark.parametrize("n", [1, 7, 20, 31])
def test_prolongation_to_the_same_grid_is_the_identity(n):
    rng = np.random.default_rng(n)
    for name in STATE:
        a = rng.standard_normal(shape_of(name, n))
        assert np.array_equal(cascade.prolong_time(a, name, n, n), a), name


@pytest.mark.parametrize("n_src,n_dst", PAIRS)
def test_shapes_constants_and_linear_fields(n_src, n_dst):
    rng = np.random.default_rng(n_src * 100 + n_dst)
    for name in STATE:
        shp = shape_of(name, n_src)
        out = cascade.prolong_time(rng.standard_normal(shp), name, n_src, n_dst)
        assert out.shape == shape_of(name, n_dst), name
        # constants exactly: (1 - w) * c + w * c with c a power of two is c * fl(fl(1 - w) + w), and fl(fl(1 - w) + w) = 1 for every w in
        # [0, 1] (w >= 1/2: 1 - w is exact; w < 1/2: 1 - w is off by at most 2^-54, which the sum rounds away).  Any other constant goes
        # through three roundings (two products, one sum): within 2 ulp.
        for c in (1.0, -0.25, 0.0):
            const = cascade.prolong_time(np.full(shp, c), name, n_src, n_dst)
            assert np.array_equal(const, np.full(shape_of(name, n_dst), c)), (name, c)
        const = cascade.prolong_time(np.full(shp, 0.3), name, n_src, n_dst)
        assert np.max(np.abs(const - 0.3)) <= 2 * np.spacing(0.3), name
        # a field linear in t (with a different slope and offset per spatial entry)
        slope, off = rng.standard_normal(shp[1:]), rng.standard_normal(shp[1:])
        ts, td = times(name, n_src), times(name, n_dst)
        ex = (None,) * (len(shp) - 1)
        lin = ts[(slice(None),) + ex] * slope[None] + off[None]
        got = cascade.prolong_time(lin, name, n_src, n_dst)
        want = td[(slice(None),) + ex] * slope[None] + off[None]
        inside = np.ones(td.size, dtype=bool) if name in NODE else (td >= ts[0]) & (td <= ts[-1])
        assert np.max(np.abs(got[inside] - want[inside]), initial=0.0) < 1e-14, name
        if name not in NODE and n_src > 1:      # constant beyond the first / last source centre
            assert np.array_equal(got[td < ts[0]], np.broadcast_to(lin[0], got[td < ts[0]].shape))
            assert np.array_equal(got[td > ts[-1]], np.broadcast_to(lin[-1], got[td > ts[-1]].shape))


def test_single_source_interval_is_constant_in_time():
    rng = np.random.default_rng(3)
    for name in ("A", "z_mid", "beta_end"):
        a = rng.standard_normal(shape_of(name, 1))
        out = cascade.prolong_time(a, name, 1, 4)
        assert np.array_equal(out, np.broadcast_to(a[0], out.shape))


def test_prolong_time_checks_its_input():
    with pytest.raises(ValueError):
        cascade.prolong_time(np.zeros((8, V)), "phi", 8, 16)      # phi has n + 1 nodes
    with pytest.raises(ValueError):
        cascade.prolong_time(np.zeros((8, V)), "rho", 8, 16)
    with pytest.raises(ValueError):
        cascade.time_weights(0, 4, True)


def test_default_levels():
    assert cascade.default_levels(1023) == [15, 31, 63, 127, 255, 511, 1023]
    assert cascade.default_levels(31) == [15, 31]
    assert cascade.default_levels(20) == [20]      # 21 nodes: an odd number is not halved
    assert cascade.default_levels(15) == [15]
    assert cascade.default_levels(47) == [23, 47]   # 48 -> 24 nodes -> 12 would fall below 16


def test_row_map_composes_two_numberings():
    rng = np.random.default_rng(5)
    pd, ps = rng.permutation(9), rng.permutation(9)
    m = cascade.row_map(pd, ps, 9)
    assert np.array_equal(ps[m], pd)      # source row m[i] holds the caller's entity that destination row i holds
    assert cascade.row_map(pd, pd.copy(), 9) is None and cascade.row_map(None, None, 9) is None
    assert np.array_equal(np.arange(9)[cascade.row_map(pd, None, 9)], pd)


@pytest.mark.parametrize("who", ["row_map", "space_row_maps", "transfer_row_maps"])
def test_inverse_numbering_rejects_a_permutation_of_the_wrong_size(who):
    """The one inverse the three row-map builders share, under the name of each"""
    perm = np.random.default_rng(6).permutation(9)
    inv = cascade.inverse_numbering(perm, 9, who)
    assert inv.dtype == np.int64 and np.array_equal(inv[perm], np.arange(9)) and np.array_equal(perm[inv], np.arange(9))
    assert np.array_equal(cascade.inverse_numbering(None, 9, who), np.arange(9))
    for n in (8, 10):
        with pytest.raises(ValueError, match=f"^{who}: a permutation of the wrong size$"):
            cascade.inverse_numbering(perm, n, who)
    with pytest.raises(ValueError, match=f"^{who}: a permutation of the wrong size$"):
        cascade.inverse_numbering(perm.reshape(3, 3), 9, who)


def test_row_map_rejects_a_source_numbering_of_the_wrong_size():
    with pytest.raises(ValueError, match="^row_map: a permutation of the wrong size$"):
        cascade.row_map(np.arange(9)[::-1], np.arange(8), 9)


# ---------------------------------------------------------------------------- the driver's argument checks
def test_cascade_checks_its_arguments_before_any_device(monkeypatch):
    import importlib

    mod = importlib.import_module("dots_socp_amd.socp.solver_socp")
    from dots_socp_amd.socp import solver_socp_cascade

    def no_device(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")

    monkeypatch.setattr(mod, "DeviceProblem", no_device)
    geom, _ = meshes.example("torus", nu=12, nv=8)
    with pytest.raises(ValueError, match="increase"):
        solver_socp_cascade(31, geom, levels=[15, 15, 31])
    with pytest.raises(ValueError, match="increase"):
        solver_socp_cascade(31, geom, levels=[31, 15])
    with pytest.raises(ValueError, match="last level"):
        solver_socp_cascade(31, geom, levels=[7, 15])
    with pytest.raises(ValueError, match="at most 1024"):
        solver_socp_cascade(2047, geom, levels=[15, 2047])
    with pytest.raises(ValueError, match="time slabs"):
        solver_socp_cascade(31, geom, time_slab=(0, 2))
    with pytest.raises(ValueError, match="modal_pcg"):
        solver_socp_cascade(511, geom, levels=[127, 255, 511], lap_solver="modal_pcg")
    with pytest.raises(ValueError, match="level_tol"):
        solver_socp_cascade(31, geom, level_tol=-1.0)
    with pytest.raises(ValueError, match="unknown option"):
        solver_socp_cascade(31, geom, colour="red")
    with pytest.raises(ValueError, match="Checkpoint"):
        solver_socp_cascade(31, geom, tol=1e-3, tol_checkpoints=[1e-4])


def test_init_from_excludes_init_solution(monkeypatch):
    import importlib

    mod = importlib.import_module("dots_socp_amd.socp.solver_socp")

    def no_device(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")

    monkeypatch.setattr(mod, "DeviceProblem", no_device)
    geom, _ = meshes.example("torus", nu=12, nv=8)

    class Coarse:
        finalized = True

    with pytest.raises(ValueError, match="mutually exclusive"):
        mod.AlmSolver(15, geom, init_from=Coarse(), init_solution={"phi": np.zeros((16, 96))})
    Coarse.finalized = False
    with pytest.raises(ValueError, match="finalised"):
        mod.AlmSolver(15, geom, init_from=Coarse())


def test_cascade_solvers_are_exported():
    from dots_socp_amd import socp

    for name in ("solver_socp_cascade", "solver_raw_cascade", "solver_cascade"):
        assert name in socp.__all__ and callable(getattr(socp, name))


@pytest.mark.parametrize("reorder", ["nd", True, False])
def test_level_plans_equal_build_plan(reorder):
    """One host plan per mesh: every level's plan is the one build_plan returns on its own; levels with one numbering share the mesh arrays."""
    from dots_socp_amd.geometry import build_level_plans, build_plan

    geom, _ = meshes.example("knot")
    levels = [15, 31, 63]
    plans = build_level_plans(levels, geom, reorder=reorder)
    for T, p in zip(levels, plans):
        q = build_plan(T, geom, reorder=reorder)
        assert p.n_time == T
        for k in ("triangles", "hat_grad", "area_tri", "mass_vert", "corner_ptr", "corner_idx", "lap_rowptr", "lap_col", "lap_val", "mu0", "mu1",
                  "time_modes", "time_eigs", "vertices"):
            assert np.array_equal(getattr(p, k), getattr(q, k)), (T, k)
        if reorder:
            assert np.array_equal(p.perm_vert, q.perm_vert) and np.array_equal(p.perm_tri, q.perm_tri)
        if reorder == "nd":
            assert np.array_equal(p.dissection.order, q.dissection.order) and np.array_equal(p.dissection.bands, q.dissection.bands)
            assert p.dissection.top_inverse == q.dissection.top_inverse
    for p in plans[1:]:
        same = p.perm_vert is None or np.array_equal(p.perm_vert, plans[0].perm_vert)
        assert (p.lap_val is plans[0].lap_val) == same      # shared exactly where the numbering is the same
    if reorder != "nd":
        assert all(p.lap_val is plans[0].lap_val for p in plans)


# ---------------------------------------------------------------------------- the scheme itself, on the CPU
def test_cascade_halves_the_finest_level_iterations_with_the_oracle():
    """Plane n = 20, congestion 0, tol 1e-3, levels [15, 31]: the finest level, warm-started from the interpolated solution of the
    coarse one, stops within half the iterations of the cold run (measured when the scheme was proposed: 51 against 361) with every
    KKT residual below tol."""
    O = load_oracle()
    geom, _ = meshes.example("plane", n=20)
    tol = 1e-3
    _, cold = O.solver_socp(31, geom, congestion=0.0, nit=4000, tol=tol)
    sol15, h15 = O.solver_socp(15, geom, congestion=0.0, nit=4000, tol=tol)
    init = cascade.prolong_solution(sol15, 15, 31)
    assert set(init) == set(STATE)
    _, warm = O.solver_socp(31, geom, congestion=0.0, nit=4000, tol=tol, init_solution=init)
    n_cold, n_coarse, n_warm = cold.last_record_it + 1, h15.last_record_it + 1, warm.last_record_it + 1
    print(f"iterations: cold {n_cold}, cascade {n_coarse} + {n_warm}")
    assert 2 * n_warm <= n_cold
    assert np.nanmax(warm.kkt_errors[-1]) < tol
    print("cost: cold", cold.history["Transportation cost"][-1], "cascade", warm.history["Transportation cost"][-1])

"""CPU side of the long time horizons (T + 1 in (256, 1024]): the oracle against the reference's recorded runs (tests/golden/long_*.npz),
the Python refusals that come before any library call, and the band cuts of the frontal plan at mode pitches 512 and 1024."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, load_oracle
from dots_socp_amd import meshes

O = load_oracle()
LONG = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN_DIR, "long_*.npz")))


def golden(name):
    return np.load(os.path.join(GOLDEN_DIR, name))


def test_fixtures_are_there():
    assert LONG == ["long_plane8_T1023_tol1e-3.npz", "long_plane8_T383_cong_tol1e-3.npz", "long_plane8_T383_tol1e-3.npz"]


@pytest.mark.parametrize("fname", LONG)
def test_oracle_reproduces_the_reference(fname):
    g = golden(fname)
    geom = dict(vertices=g["vertices"], triangles=g["triangles"], mu0=g["mu0"], mu1=g["mu1"])
    kw = {k[3:]: (g[k].tolist() if g[k].ndim else g[k].item()) for k in g.files if k.startswith("kw_")}
    sol, hist = O.solver_socp(int(g["n_time"]), geom, **kw)
    assert int(hist.kkt_iteration[-1]) == int(g["last_iteration"])
    got, want = np.asarray(hist.kkt_errors), g["hist_kkt_errors"]
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    m = ~np.isnan(want)
    assert np.allclose(got[m], want[m], rtol=1e-6, atol=1e-13)
    for key in ("Transportation cost", "Objective value"):
        assert np.allclose(hist.history[key], g["hist_" + key.replace(" ", "_")], rtol=1e-6, atol=0, equal_nan=True), key
    assert float(np.max(np.abs(sol["mu"] - g["sol_mu"])) / np.max(np.abs(g["sol_mu"]))) < 1e-5


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the HIP library fails the test: the refusals must come first."""
    from dots_socp_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", refuse)


@pytest.mark.parametrize("T,kw,match", [(300, dict(lap_solver="modal_pcg"), "modal_direct"), (511, dict(lap_solver="modal_pcg"), "256"),
                                        (1024, {}, "1024"), (1024, dict(lap_solver="spacetime_pcg"), "1024")])
def test_solver_refuses_before_the_library(no_library, T, kw, match):
    from dots_socp_amd.socp import solver_socp

    geom, _ = meshes.example("sphere", level=1)
    with pytest.raises(ValueError, match=match):
        solver_socp(T, geom, **kw)


@pytest.mark.parametrize("T", [256, 511, 1023])
def test_time_slabs_refuse_before_the_library(no_library, T):
    from dots_socp_amd.distributed import ShardedAlmSolver
    from dots_socp_amd.socp.solver_socp import check_time_nodes

    geom, _ = meshes.example("sphere", level=1)
    with pytest.raises(ValueError, match="256"):
        ShardedAlmSolver(T, geom, comm=object())
    with pytest.raises(ValueError, match="time slabs"):
        check_time_nodes(T, "modal_direct", time_slab=(0, 2))
    check_time_nodes(T, "modal_direct")      # one GPU: fine
    check_time_nodes(255, "modal_pcg", time_slab=(0, 2))


@pytest.mark.parametrize("mesh,kw", [("knot", {}), ("torus", dict(nu=400, nv=250))])
def test_band_cuts_at_long_horizons(mesh, kw):
    """plan_bands at pitches 512 and 1024: valid cuts (0 .. H, 1 to 4 heights per band), and no more merging than at a pitch of 128 -- the
    factor bytes grow with the pitch, so launches matter less, not more."""
    import scipy.sparse as sp

    from dots_socp_amd import frontal
    from dots_socp_amd.geometry import build_plan

    geom, _ = meshes.example(mesh, **kw)
    p = build_plan(1023, geom, reorder="nd")
    K = sp.csr_matrix((p.lap_val, p.lap_col, p.lap_rowptr), shape=(p.n_vertices, p.n_vertices))
    diss = p.dissection
    ff = frontal.factorize(K, p.mass_vert, p.time_eigs[:4], diss, pitch=8, numeric=False)
    H = int(diss.height.max()) + 1
    n128 = len(frontal.plan_bands(diss, ff.node_n, ff.node_b, 128, spec="auto", top_spec="auto")[0]) - 1
    for pitch in (512, 1024):
        cuts, top = frontal.plan_bands(diss, ff.node_n, ff.node_b, pitch, spec="auto", top_spec="auto")
        d = np.diff(cuts)
        assert cuts[0] == 0 and cuts[-1] == H and np.all(d >= 1) and np.all(d <= 4), (pitch, cuts)
        assert len(cuts) - 1 >= n128, (pitch, cuts, n128)
    # the plan the library is handed at those horizons cuts the same way
    assert [int(x) for x in diss.bands] == [int(x) for x in frontal.plan_bands(diss, ff.node_n, ff.node_b, 1024, spec="auto", top_spec="auto")[0]]

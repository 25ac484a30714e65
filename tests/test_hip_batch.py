"""GPU tests of the batched direct solve: several contexts on one surface share one factor (dots_front_share) and their
right-hand sides go through ONE sequence of multi-rhs sweep launches (dots_laplacian_solve_many).  Every problem's solution must
be bit for bit what the solve of that problem alone computes."""
import numpy as np
import pytest

from conftest import has_gpu
from dots_socp_amd import _lib, meshes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]


def make(geom, T, eps, plan=None, reorder="nd", **kw):
    from dots_socp_amd.device import DeviceProblem

    dev = DeviceProblem(T, geom, lap_solver="modal_pcg", reorder=reorder, plan=plan, **kw)
    dev.set_params(r=1.3, eps=eps)
    return dev


def family(geom, T, eps, n, **kw):
    """an owner with its factor and n - 1 contexts sharing it"""
    owner = make(geom, T, eps, **kw)
    owner.setup_frontal(eps=eps)
    devs = [owner]
    for _ in range(n - 1):
        d = make(geom, T, eps, plan=owner.plan)
        d.share_frontal(owner)
        devs.append(d)
    return devs


def check_batches(devs, seed=5):
    from dots_socp_amd.device import laplacian_solve_many

    rng = np.random.default_rng(seed)
    rhs = [rng.standard_normal(d.shape("phi")) for d in devs]
    alone = [laplacian_solve_many([d], [b])[0] for d, b in zip(devs, rhs)]
    for x in alone:
        assert np.all(np.isfinite(x))
    for n in (1, 2, 3, 5, 8):
        if n > len(devs):
            break
        got = laplacian_solve_many(devs[:n], rhs[:n])
        for k in range(n):
            assert np.array_equal(got[k], alone[k]), (n, k)
    # problems in another order, one repeated right-hand side: still each its own solution
    order = list(reversed(range(len(devs))))
    got = laplacian_solve_many([devs[k] for k in order], [rhs[0] if k == 1 else rhs[k] for k in order])
    for j, k in enumerate(order):
        want = laplacian_solve_many([devs[k]], [rhs[0]])[0] if k == 1 else alone[k]
        assert np.array_equal(got[j], want), k
    return alone, rhs


def close_all(devs):
    for d in devs:
        d.close()


@pytest.mark.parametrize("mesh,kw,T,eps", [("torus", dict(nu=40, nv=24), 5, 1e-3), ("sphere", dict(level=4), 31, 0.0),
                                           ("knot", dict(nu=240, nv=10), 7, 1e-2)])
def test_batched_sweeps_are_bit_identical(mesh, kw, T, eps):
    geom, _ = meshes.example(mesh, **kw)
    devs = family(geom, T, eps, 8)
    try:
        check_batches(devs)
    finally:
        close_all(devs)


@pytest.mark.parametrize("nr", ["2", "8"])
def test_batched_sweeps_other_widths_and_unmerged_bands(monkeypatch, nr):
    """one launch per tree height (DOTS_FRONT_BANDS=off: the leaf kernels and the un-merged bands) and 2 / 8 rhs per launch"""
    monkeypatch.setenv("DOTS_FRONT_BANDS", "off")
    monkeypatch.setenv("DOTS_FRONT_NR", nr)
    geom, _ = meshes.example("torus", nu=72, nv=40)
    devs = family(geom, 31, 1e-3, 8)
    try:
        assert devs[0].debug_counter(4) > 0      # the leaves run in the leaf kernels
        check_batches(devs, seed=7)
    finally:
        close_all(devs)


def test_batched_sweeps_on_high_degree_leaves(monkeypatch):
    """the mesh of test_hip_frontal's CSR fall-back (leaves of 48 vertices next to poles of degree 64): the leaf kernels walk the CSR"""
    nlat, nlon = 12, 64
    th = np.pi * np.arange(1, nlat + 1) / (nlat + 1)
    ph = 2.0 * np.pi * np.arange(nlon) / nlon
    rings = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(nlon))], axis=2).reshape(-1, 3)
    v = np.concatenate([rings, [[0.0, 0.0, 1.0]], [[0.0, 0.0, -1.0]]])
    north, south = nlat * nlon, nlat * nlon + 1
    t = []
    for j in range(nlon):
        k = (j + 1) % nlon
        t.append((north, j, k))
        t.append((south, (nlat - 1) * nlon + k, (nlat - 1) * nlon + j))
        for i in range(nlat - 1):
            a0, a1, b0, b1 = i * nlon + j, i * nlon + k, (i + 1) * nlon + j, (i + 1) * nlon + k
            t += [(a0, b0, a1), (a1, b0, b1)]
    t = np.asarray(t)
    mu0, mu1 = 1.0 + v[:, 2], 1.0 - v[:, 2]
    geom = dict(vertices=v, triangles=t, mu0=mu0 / mu0.sum(), mu1=mu1 / mu1.sum())
    monkeypatch.setenv("DOTS_FRONT_BANDS", "off")
    devs = family(geom, 15, 1e-2, 5, nd_leaf=48)
    try:
        assert devs[0].debug_counter(4) > 0 and devs[0].debug_counter(5) == 0
        check_batches(devs, seed=11)
    finally:
        close_all(devs)


def test_shared_factor_outlives_its_owner():
    """destroy the owner mid-run: the sharer keeps stepping on the factor and ends where a run with the owner alive ends"""
    from dots_socp_amd.device import laplacian_solve_many, step_many

    geom, _ = meshes.example("torus", nu=40, nv=24)
    finals = []
    for drop in (False, True):
        devs = family(geom, 5, 1e-3, 2)
        try:
            rng = np.random.default_rng(2)
            for name in ("A", "lambda_c", "mu", "B", "E"):
                devs[1].upload(name, rng.standard_normal(devs[1].shape(name)))
            devs[1].step(2)
            step_many(devs[1:])
            if drop:
                devs[0].close()      # the owner goes first: the sharer keeps the factor
            devs[1].step(2)
            step_many(devs[1:])
            b = rng.standard_normal(devs[1].shape("phi"))
            finals.append([devs[1].download(k) for k in ("phi", "A", "B", "mu", "E")] + laplacian_solve_many(devs[1:], [b]))
        finally:
            close_all(devs)
    for a, b in zip(*finals):
        assert np.array_equal(a, b)


def test_batched_solve_inverts_the_operator():
    """eps > 0: the batched solutions satisfy K x = b through DOTS_OP_LAPLACIAN_APPLY"""
    from dots_socp_amd.device import laplacian_solve_many

    geom, _ = meshes.example("torus", nu=40, nv=24)
    devs = family(geom, 5, 1e-3, 3)
    try:
        rng = np.random.default_rng(9)
        rhs = [rng.standard_normal(d.shape("phi")) for d in devs]
        for d, b, x in zip(devs, rhs, laplacian_solve_many(devs, rhs)):
            r = d.apply_operator("laplacian_apply", x) - b
            assert np.max(np.abs(r)) < 1e-10 * np.max(np.abs(b))
    finally:
        close_all(devs)


def test_sharing_and_batches_are_checked():
    from dots_socp_amd.device import laplacian_solve_many, step_many

    geom, _ = meshes.example("torus", nu=40, nv=24)
    owner = make(geom, 5, 1e-3)
    owner.setup_frontal(eps=1e-3)
    others = []
    try:
        other_eps = make(geom, 5, 2e-3, plan=None)
        others.append(other_eps)
        with pytest.raises(_lib.HipLibraryError) as e:
            other_eps.share_frontal(owner)
        assert e.value.status == _lib.ERR_ARGUMENT and "eps" in str(e.value)
        other_t = make(geom, 7, 1e-3)
        others.append(other_t)
        with pytest.raises(_lib.HipLibraryError) as e:
            other_t.share_frontal(owner)
        assert e.value.status == _lib.ERR_ARGUMENT
        pcg = make(geom, 5, 1e-3, plan=owner.plan)      # no factor: the modal PCG context
        others.append(pcg)
        b = np.zeros(owner.shape("phi"))
        with pytest.raises(_lib.HipLibraryError) as e:
            laplacian_solve_many([owner, pcg], [b, b])
        assert e.value.status == _lib.ERR_STATE
        with pytest.raises(_lib.HipLibraryError) as e:
            laplacian_solve_many([pcg], [b])
        assert e.value.status == _lib.ERR_STATE
        with pytest.raises(_lib.HipLibraryError) as e:
            step_many([owner, pcg])
        assert e.value.status == _lib.ERR_STATE
        from dots_socp_amd.device import DeviceProblem

        slab = DeviceProblem(5, geom, lap_solver="modal_pcg", time_slab=(0, 2))
        others.append(slab)
        with pytest.raises(_lib.HipLibraryError) as e:
            step_many([slab])
        assert e.value.status == _lib.ERR_STATE
        with pytest.raises(_lib.HipLibraryError) as e:
            slab.share_frontal(owner)
        assert e.value.status == _lib.ERR_STATE
        # a mesh with the same counts in another vertex numbering: refused
        moved = make(geom, 5, 1e-3, reorder=True)
        others.append(moved)
        with pytest.raises(_lib.HipLibraryError) as e:
            moved.share_frontal(owner)
        assert e.value.status == _lib.ERR_ARGUMENT
        # the penalty decision ahead is refused for a context stepped in a batch
        step_many([owner])
        with pytest.raises(_lib.HipLibraryError) as e:
            owner.penalty_ahead(1e-3, False, 0.1, 10.0, [(0.5, 2.0)])
        assert e.value.status == _lib.ERR_STATE
    finally:
        close_all([owner] + others)

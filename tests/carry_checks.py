"""What the GPU tests of the two carriers in space share (test_hip_mesh_cascade.py, test_hip_mesh_transfer.py): the geometries' densities,
the scaled random source, and the comparison of a device carry with its host specification, bit for bit, under every pairing of device
numberings."""
import numpy as np

from dots_socp_amd import meshes

STATE = ("phi", "A", "B", "lambda_c", "z_fst", "z_mid", "z_end", "mu", "E", "beta_fst", "beta_mid", "beta_end")


def with_bumps(v, t):
    geom, _ = meshes.make_geometry(v, t, normalize=False)
    c = meshes.farthest_vertices(geom["vertices"], 0, 3)
    geom["mu0"] = meshes.bump_density(geom["vertices"], geom["area_vertices"], [c[0]], 1.0, 0.4)
    geom["mu1"] = meshes.bump_density(geom["vertices"], geom["area_vertices"], [c[1], c[2]], 1.0, 0.4)
    return geom


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def scaled_source(geom, n_time, reorder, seed):
    """A finalised solver on the coarse mesh whose recovery factors all differ from 1 (a few iterations with penalty updates, a primal /
    dual rescaling, a z rescale), its twelve arrays then filled with random values: every entry of every array is exercised."""
    from dots_socp_amd.socp.solver_socp import AlmSolver

    alm = AlmSolver(n_time, geom, nit=40, tol=1e-12, check_kkt_step_by_step=True, reorder=reorder)
    for _ in range(6):
        alm.iterate()
    alm.adjust_penalty(1.3)
    alm.scale_prim_dual(scale_factor=(5.0, 0.7))
    alm.scale_variable_z(1.5)
    alm.iterate()
    alm.finalize(download=False)
    assert all(f != 1.0 for f in alm.recovery_factors())
    rng = np.random.default_rng(seed)
    for k in STATE:
        alm.dev.upload(k, rng.standard_normal(alm.dev.shape(k)))
    return alm


def check_carry(coarse, fine, n_time, carry, host, bytes_ok, src_orders=(True, False), dst_orders=("nd", False)):
    """``carry(dst, src_dev, factors)`` -> ms: the device carry under test; ``host(solution)``: its specification on the recovered
    solution; ``bytes_ok(dst, pitch)``: what ``dst.prolong_bytes`` must satisfy."""
    from dots_socp_amd.device import DeviceProblem

    for src_order in src_orders:
        alm = scaled_source(coarse, n_time, src_order, seed=n_time)
        try:
            assert (alm.dev.plan.perm_vert is not None) == bool(src_order)
            want = host({k: alm.recovered(k, alm.dev.download(k)) for k in STATE})
            for dst_order in dst_orders:
                with DeviceProblem(n_time, fine, lap_solver="modal_pcg", reorder=dst_order) as dst, \
                        DeviceProblem(n_time, fine, lap_solver="modal_pcg", reorder=dst_order) as ref:
                    ms = carry(dst, alm.dev, alm.recovery_factors())
                    pitch = max(8, 1 << int(np.ceil(np.log2(n_time + 1))))
                    assert ms >= 0.0 and bytes_ok(dst, pitch)
                    for k in STATE:
                        ref.upload(k, want[k])
                    for k in STATE:
                        got, up = dst.download(k), ref.download(k)
                        assert got.shape == want[k].shape
                        assert np.array_equal(bits(got), bits(up)), (k, src_order, dst_order, float(np.max(np.abs(got - up))))
                        assert np.array_equal(bits(got), bits(want[k])), (k, src_order, dst_order)
                    # the columns beyond the arrays' time points are as an upload leaves them: one step from either gives the same iterate
                    if n_time + 1 <= 256:      # (above, only a context with a factor steps)
                        for dev in (dst, ref):
                            dev.step(1)
                        for k in STATE:
                            assert np.array_equal(bits(dst.download(k)), bits(ref.download(k))), (k, "after a step", src_order, dst_order)
        finally:
            alm.close()

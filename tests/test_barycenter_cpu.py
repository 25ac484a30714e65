"""The barycentre without a GPU: the properties and refusals of the specification of the update (barycenter.update_host), the loop
(barycenter.barycenter_host) on the fp64 oracle against the exact midpoint of the plane's two Gaussians, the driver's checks before
any device is touched, and the new kernels' resources as the compiler reports them."""
import math
import os

import numpy as np
import pytest

import barycenter_checks as bc
from dots_socp_amd import _lib, barycenter

U = 2.0 ** -53


def inputs(V=37, K=3, seed=0):
    rng = np.random.default_rng(seed)
    nu = rng.uniform(0.1, 1.0, V)
    mass = 2.5
    return nu * (mass / math.fsum(nu)), 0.02 * rng.standard_normal((K, V)), rng.uniform(0.2, 1.0, K), 100.0, mass


def test_potentials_that_are_constants_leave_nu_where_it_is():
    """y = nu * exp(-eta * 0) = nu, S = fsum(nu), nu_new = nu * (mass / S): one multiplication and one division away."""
    nu, _, w, eta, mass = inputs()
    V = nu.shape[0]
    for potentials in (np.zeros((3, V)), np.array([[0.5] * V, [-2.0] * V, [1024.0] * V])):      # (constants whose mean is exact)
        new, s = barycenter.update_host(nu, potentials, w, eta, mass)
        assert np.all(np.abs(new - nu) <= 2.0 * U * nu)
        assert s["gmax"] == 0.0 and s["sum"] == math.fsum(nu) and s["change"] <= 2.0 * U * mass and s["min"] == np.min(new)


def test_the_sum_is_the_mass_and_a_constant_changes_nothing():
    nu, potentials, w, eta, mass = inputs()
    new, s = barycenter.update_host(nu, potentials, w, eta, mass)
    assert abs(math.fsum(new) - mass) <= 4.0 * np.spacing(mass)
    assert s["change"] > 0.1 * mass and s["gmax"] * eta > 0.5      # the update moves: the properties are not those of the identity
    assert s["change"] == math.fsum(np.abs(new - nu)) and s["min"] == np.min(new) > 0.0
    for k in range(potentials.shape[0]):
        shifted = potentials.copy()
        shifted[k] += 3.25
        again, _ = barycenter.update_host(nu, shifted, w, eta, mass)
        assert np.all(np.abs(again - new) <= 1e-12 * new)


def test_one_measure_without_a_step_is_the_identity():
    nu, potentials, _, _, mass = inputs(K=1)
    new, s = barycenter.update_host(nu, potentials, [1.0], 0.0, mass)
    assert np.all(np.abs(new - nu) <= 2.0 * U * nu) and s["sum"] == math.fsum(nu)


def test_update_host_follows_its_stated_order():
    """The scalar loop of the docstring on a small case, bit for bit."""
    nu, potentials, w, eta, mass = inputs(V=5, K=2, seed=3)
    V = 5
    m = [math.fsum(potentials[k]) / V for k in range(2)]
    g = [0.0] * V
    for v in range(V):
        for k in range(2):
            g[v] = g[v] + float(w[k]) * (-(float(potentials[k][v]) - m[k]))
    y = [float(nu[v]) * float(np.exp((-eta) * g[v])) for v in range(V)]
    S = math.fsum(y)
    want = [y[v] * (mass / S) for v in range(V)]
    new, s = barycenter.update_host(nu, potentials, w, eta, mass)
    assert list(new) == want and s["sum"] == S and s["gmax"] == max(abs(x) for x in g)


def test_update_host_refusals():
    nu, potentials, w, eta, mass = inputs()
    for bad in (0.0, -1e-3, np.nan):
        start = nu.copy()
        start[7] = bad
        with pytest.raises(ValueError, match="not positive"):
            barycenter.update_host(start, potentials, w, eta, mass)
    with pytest.raises(ValueError, match="potentials must have shape"):
        barycenter.update_host(nu, potentials[:, :-1], w, eta, mass)
    with pytest.raises(ValueError, match="potentials must have shape"):
        barycenter.update_host(nu, np.zeros((17, nu.shape[0])), np.ones(17), eta, mass)
    with pytest.raises(ValueError, match="weights must have shape"):
        barycenter.update_host(nu, potentials, w[:-1], eta, mass)
    with pytest.raises(ValueError, match="nu must have shape"):
        barycenter.update_host(nu.reshape(1, -1), potentials, w, eta, mass)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="weight that is not finite"):
            barycenter.update_host(nu, potentials, [w[0], bad, w[2]], eta, mass)
        with pytest.raises(ValueError, match="eta and mass"):
            barycenter.update_host(nu, potentials, w, bad, mass)


def test_the_loop_halves_eta_after_a_rise_and_stops_on_a_small_change():
    """A scripted solver: the costs rise at step 2, so eta is halved for the updates from step 2 on; nothing is redone."""
    V = 6
    measures = np.full((2, V), 1.0 / V)
    costs = iter([5.0, 5.0, 4.0, 4.0, 4.5, 4.5, 4.0, 4.0])
    calls = []

    def solve(nu, mu):
        calls.append(nu.copy())
        return next(costs), np.linspace(0.0, 0.01, V)
    r = barycenter.barycenter_host(solve, measures, None, np.ones(V), 4, 10.0)
    assert r["objective"] == [5.0, 4.0, 4.5, 4.0] and r["eta"] == [10.0, 10.0, 5.0, 5.0] and len(calls) == 8
    assert np.array_equal(r["costs"], [4.0, 4.0]) and len(r["change"]) == 4
    assert np.allclose(calls[0], 1.0 / V, rtol=1e-15) and np.array_equal(calls[0], calls[1])      # the default start; one nu per step
    stop = barycenter.barycenter_host(lambda nu, mu: (1.0, np.zeros(V)), measures, None, np.ones(V), 9, 10.0, tol_change=1e-9)
    assert len(stop["objective"]) == 1
    with pytest.raises(ValueError, match="not positive"):
        barycenter.barycenter_host(solve, measures, None, np.ones(V), 2, 10.0, init=np.array([1.0, 0.0, 1.0, 1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="one positive total mass"):
        barycenter.barycenter_host(solve, [measures[0], 2.0 * measures[1]], None, np.ones(V), 2, 10.0)


def test_the_driver_refuses_before_the_library(monkeypatch):
    from dots_socp_amd import socp

    def refuse(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", refuse)
    geom, measures = bc.plane_case()
    with pytest.raises(ValueError, match="measures must be"):
        socp.barycenter(7, geom, [measures[0][:-1]])
    with pytest.raises(ValueError, match="weights must be"):
        socp.barycenter(7, geom, measures, weights=[0.5, np.inf])
    with pytest.raises(ValueError, match="not positive"):
        socp.barycenter(7, geom, measures, init=np.zeros(measures[0].shape[0]))
    with pytest.raises(ValueError, match="steps"):
        socp.barycenter(7, geom, measures, steps=0)
    with pytest.raises(ValueError, match="unknown option"):
        socp.barycenter(7, geom, measures, preconditioner="jacobi")


@pytest.fixture(scope="module")
def plane_by_the_oracle():
    """The (0.5, 0.5) barycentre of the plane's two Gaussians by the loop on the fp64 oracle: 8 steps, about 20 s."""
    geom, measures = bc.plane_case()
    r = barycenter.barycenter_host(bc.oracle_solve(geom), measures, [0.5, 0.5], geom["area_vertices"], bc.PLANE_STEPS, bc.PLANE_ETA)
    return geom, r


def test_the_loop_on_the_oracle_reaches_the_exact_midpoint(plane_by_the_oracle):
    geom, r = plane_by_the_oracle
    distance = bc.rel_l1(r["nu"], bc.plane_exact(geom, 0.5))
    print("objective", r["objective"], "eta", r["eta"], "relative L1 distance to the exact midpoint", distance)
    objective = r["objective"]
    assert len(objective) == bc.PLANE_STEPS
    assert all(objective[s + 1] <= objective[s] + 2e-6 for s in range(1, len(objective) - 1))      # non-increasing from step 1 on
    assert abs(objective[-1] - 0.010304) <= 1e-5
    assert abs(objective[-1] - bc.ORACLE_HALF_OBJECTIVE) <= 2e-6
    assert distance <= bc.ORACLE_MARGIN * bc.ORACLE_HALF_L1
    assert abs(distance - bc.ORACLE_HALF_L1) <= 2e-4      # the recorded figure is this run's
    assert np.all(r["nu"] > 0.0) and abs(math.fsum(r["nu"]) - 1.0) <= 1e-13


def test_the_new_kernels_need_no_scratch(tmp_path):
    """k_bary_*: no private segment and no spills, from the code object's metadata (as test_kernel_resources_cpu.py reads it)."""
    import test_kernel_resources_cpu as kr

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the HIP library is not built")
    if not kr.READELF or not kr.OBJCOPY:
        pytest.skip("llvm-readelf / llvm-objcopy not found")
    records = [r for co in kr.code_objects(_lib.LIB_PATH, str(tmp_path)) for r in kr.kernel_records(co)]
    mine = {kr.short_name(r["name"]): r for r in records if kr.short_name(r["name"]).startswith("k_bary")}
    assert sorted(mine) == ["k_bary_finish", "k_bary_fold", "k_bary_means", "k_bary_update"]
    for name, r in mine.items():
        assert int(r["private_segment_fixed_size"]) == 0 and int(r["vgpr_spill_count"]) == 0 and int(r["sgpr_spill_count"]) == 0, (name, r)
        assert int(r["max_flat_workgroup_size"]) == 256 and int(r["group_segment_fixed_size"]) <= 128, (name, r)

"""The helpers of the one-step checks (tests/step_checks.py) against themselves, without a GPU: the planted state has the properties it
claims on the oracle's own projection, ``check_one_step`` passes oracle against oracle, and it FAILS for deliberate defects of the kind a
kernel variant could have -- so the inputs discriminate.  The scenario drivers of test_hip_step_variants.py also run here, on an oracle
that plays the device."""
import numpy as np
import pytest

import step_checks as sc

MESH_T = [(m, T) for m in sc.MESHES for T in sc.T_ALL]


@pytest.fixture(scope="module")
def geoms():
    return {m: sc.geometry(m) for m in sc.MESHES}


def test_fan_mesh(geoms):
    s = sc.make_oracle(1, geoms["fan"])
    assert (s.V, s.F) == (11, 9)
    assert sorted(sc.valence(s).tolist()) == [1, 1] + [2] * 8 + [9]
    g = geoms["fan"]
    assert g["mu0"].min() > 0 and g["mu1"].min() > 0 and abs(g["mu0"].sum() - g["mu1"].sum()) < 1e-15
    assert s.area_f.min() > 0


@pytest.mark.parametrize("mesh,T", MESH_T)
def test_edge_state_and_oracle_against_oracle(geoms, mesh, T):
    for div in (1.0, sc.FACTOR):
        s = sc.make_oracle(T, geoms[mesh], congestion=0.05)
        masks = sc.edge_state(s, seed=T, div=div)
        sc.assert_edge_properties(masks)
        # the planted columns are where they were put, the NaN ones at an even t and at the last interval
        p = masks["planted"]
        assert masks["nan"][p["nan0"]] and masks["nan"][p["nan1"]] and p["nan0"][0] % 2 == 0 and p["nan1"][0] == T - 1
        assert masks["on_upper"][p["up0"]] and masks["on_upper"][p["up1"]] and masks["on_lower"][p["lo0"]] and masks["on_lower"][p["lo1"]]
        before = sc.snapshot(s)
        if div != 1.0:
            before = sc.apply_penalty(s, before, div)
        after = sc.oracle_step(s, before)
        # the reference's own behaviour on the planted columns: exact boundaries, exact zeros, NaN
        t, v = p["up0"]
        assert after["z_fst"][t, v] > 0 and after["z_end"][t, v] == after["z_fst"][t, v]
        t, v = p["lo0"]
        assert after["z_fst"][t, v] == 0.0 and after["z_end"][t, v] == 0.0
        t, v = p["nan1"]
        assert np.isnan(after["z_fst"][t, v]) and np.isnan(after["A"][t, v])
        fig = sc.check_one_step(s, before, after)
        assert max(fig.values()) == 0.0


MUTATIONS = ("one_branch", "drops_nan", "odd_tail", "last_corner")


@pytest.mark.parametrize("mesh,T", MESH_T)
def test_check_one_step_fails_for_deliberate_defects(geoms, mesh, T):
    s = sc.make_oracle(T, geoms[mesh])
    sc.edge_state(s, seed=100 + T)
    before = sc.snapshot(s)
    for mutation in MUTATIONS:
        if mutation == "odd_tail" and T % 2 == 0:
            continue      # (no lane without a second interval)
        after = sc.oracle_step(s, before, mutation)
        with pytest.raises(AssertionError):
            sc.check_one_step(s, before, after)
    # the division applied to four of the five dual arrays only
    def pending(skip=()):
        s = sc.make_oracle(T, geoms[mesh])
        sc.edge_state(s, seed=100 + T, div=sc.FACTOR)
        return s, sc.apply_penalty(s, sc.snapshot(s), sc.FACTOR, skip=skip)

    s, before = pending()
    for forgotten in sc.DUAL:
        m, start = pending(skip=(forgotten,))
        with pytest.raises(AssertionError):
            sc.check_one_step(s, before, sc.oracle_step(m, start))
    # ... and a phi that is off by more than the solve's bound
    after = sc.oracle_step(s, before)
    after["phi"] = after["phi"] + 1e-7 * np.abs(after["phi"]).max() * np.cos(np.arange(after["phi"].size)).reshape(after["phi"].shape)
    with pytest.raises(AssertionError):
        sc.check_one_step(s, before, after)


def test_compare_entries_is_entry_by_entry():
    want = np.array([1.0, 1e-9, np.nan, -2.0])
    sc.compare_entries("x", want.copy(), want)
    sc.compare_entries("x", want + np.array([1e-13, 1e-13, 0.0, 1e-13]), want)      # small entries: against the array's rms
    for bad in (np.array([1.0, 1e-9, 0.0, -2.0]), np.array([np.nan, 1e-9, np.nan, -2.0]), np.array([1.0, 1e-9, np.nan, -2.0 - 1e-11])):
        with pytest.raises(AssertionError):
            sc.compare_entries("x", bad, want)


@pytest.mark.parametrize("name,mesh,T,congestion", [c for c in sc.cases() if c[3] == 0.05])
def test_scenarios_on_the_oracle(geoms, name, mesh, T, congestion):
    """The drivers of test_hip_step_variants.py with an oracle in the device's place: their bookkeeping (which state is `before`, where the
    penalty update goes, what is skipped) is right, and the conditions they put on their inputs hold at every mesh and T."""
    s = sc.make_oracle(T, geoms[mesh], congestion)
    dev = sc.OracleDevice(T, geoms[mesh], congestion)
    sc.scenario(name)(dev, s, T, seed=T, expect=lambda dev, **bits: None)

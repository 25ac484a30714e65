"""The checks of the time-slab iteration (tests/slab_checks.py), checked themselves on the CPU: the scenarios and partitions of
test_hip_slab_steps.py through ``SlabDevice`` over LOCAL ranks of the numpy stand-in (tests/fake_device.py), which know their own slab
and what they received and nothing else; and one deliberate defect after the other, each of which a check must catch."""
import numpy as np
import pytest

import slab_checks as sl
import step_checks as sc
from fake_device import DEFECTS, FakeDeviceProblem

MESHES = ("ops_ico1", "fan")      # closed, valence 5; a boundary and valences 1, 2 and 9
ALL = list(sl.PARTITIONS)


@pytest.fixture(scope="module")
def geoms():
    return {m: sc.geometry(m) for m in MESHES}


def fake_group(T, geom, n_ranks, defect=None):
    group = sl.SlabGroup(T, geom, n_ranks, rank_class=FakeDeviceProblem, buffers=sl.NumpyBuffers(), local=True)
    for d in group.devs:
        d.defect = defect
    return group


def test_partition_table_is_what_the_driver_cuts():
    from dots_socp_amd.distributed import slab_partition

    for (T, n_ranks), (parts, pitch) in sl.PARTITIONS.items():
        stride, cut = slab_partition(T + 1, n_ranks)
        assert [c for _, c in cut] == [nl for nl, _ in parts]
        assert [max(0, min(c, T - b)) for b, c in cut] == [ni for _, ni in parts]
        assert max(4, 1 << (stride - 1).bit_length()) == pitch
        assert sum(nl for nl, _ in parts) == T + 1 and sum(ni for _, ni in parts) == T
        assert T + 1 <= 256
    pitches = {pitch for _, pitch in sl.PARTITIONS.values()}
    assert pitches == {4, 8, 16, 32, 64, 128, 256}
    assert sl.PARTITIONS[sl.SMALL_PITCH][1] == 4 and sl.PARTITIONS[sl.LARGE_PITCH][1] >= 64


def test_stand_in_cuts_the_same_slabs(geoms):
    for (T, n_ranks), (parts, pitch) in sl.PARTITIONS.items():
        if T > 64:
            continue
        group = fake_group(T, geoms["fan"], n_ranks)
        assert [(d.nl, d.ni) for d in group.devs] == list(parts) and {d.pitch for d in group.devs} == {pitch}


@pytest.mark.parametrize("partition", ALL, ids=sl.partition_id)
@pytest.mark.parametrize("mesh", MESHES)
def test_planted_states_meet_the_conditions_on_the_input(geoms, mesh, partition):
    """On the oracle alone: the share of every branch, every branch on every interval next to a slab boundary, the special columns where
    they were asked for -- in the four variants the scenarios plant."""
    T = partition[0]
    s = sl.make_oracle(T, geoms[mesh], 0.05)
    cells, boundary = sl.slab_cells(partition), sl.boundary_intervals(partition)
    starts = sl.first_nodes(partition)
    if len(starts) > 1:
        assert starts[1] - 1 in cells.values() and (starts[1] in cells.values() or starts[1] == T)
        n0 = 0
        for nl, _ in sl.PARTITIONS[partition][0]:
            if nl == 1 and n0 > 0:
                assert n0 - 1 in boundary
            n0 += nl
        lone = [n0 for n0, (nl, _) in zip(starts, sl.PARTITIONS[partition][0]) if nl == 1 and n0 > 0]
        assert not lone or lone[-1] - 1 in cells.values()
    for zero_preimage in (True, False):
        for div in (1.0, sc.FACTOR):
            masks = sc.edge_state(s, sl.seed_for(mesh, partition), zero_preimage=zero_preimage, div=div, cells=cells)
            sc.assert_edge_properties(masks, zero_preimage=zero_preimage, cells=cells, boundary=boundary)


def test_branches_on_every_interval_of_ico1(geoms):
    """What the choice seed = T rests on: at least 5 columns of every branch in EVERY interval of ops_ico1."""
    for T in (1, 5, 31, 127, 255):
        s = sl.make_oracle(T, geoms["ops_ico1"], 0.05)
        masks = sc.edge_state(s, T)
        for branch in ("one", "zero", "mid"):
            assert masks[branch].sum(axis=1).min() >= (5 if T > 1 else 3), (T, branch)


def test_default_cells_are_the_old_places(geoms):
    s = sl.make_oracle(7, geoms["fan"], 0.0)
    a = sc.edge_state(s, 7)
    state = sc.snapshot(s)
    b = sc.edge_state(s, 7, cells=sc.default_cells(7))
    assert a["planted"] == b["planted"] and all(np.array_equal(state[k], getattr(s, k)) for k in sc.STATE)
    assert {k: t for k, (t, _) in a["planted"].items()} == {"nan0": 0, "nan1": 6, "up0": 0, "up1": 6, "lo0": 3, "lo1": 6}


def scenario_cases():
    out = []
    for name in sc.SCENARIOS_ALL_T:
        for p in ALL:
            for mesh in MESHES:
                out.append((name, mesh, p, 0.05, 0.0, False))
    for name in ("skip_z_mid", "pending_after_carry", "timed", "timed_carry", "palm"):
        for i, p in enumerate((sl.SMALL_PITCH, sl.LARGE_PITCH)):
            for j, mesh in enumerate(MESHES):
                out.append((name, mesh, p, 0.0 if (i + j) % 2 else 0.05, 0.0, bool(j)))
    for name in ("plain", "carry"):
        for i, p in enumerate((sl.SMALL_PITCH, sl.LARGE_PITCH)):
            out.append((name, MESHES[i], p, 0.05, 1e-2, bool(i)))
    return out


@pytest.mark.parametrize("name,mesh,partition,congestion,eps,split", scenario_cases(),
                         ids=lambda v: sl.partition_id(v) if isinstance(v, tuple) else None)
def test_scenarios_on_local_ranks(geoms, name, mesh, partition, congestion, eps, split):
    T, n_ranks = partition
    s = sl.make_oracle(T, geoms[mesh], congestion, eps)
    sl.run_scenario(fake_group(T, geoms[mesh], n_ranks), name, s, partition, sl.seed_for(mesh, partition), split=split)


@pytest.mark.parametrize("partition", ALL, ids=sl.partition_id)
def test_kkt_objective_orders_and_layout_on_local_ranks(geoms, partition):
    T, n_ranks = partition
    mesh = MESHES[ALL.index(partition) % 2]
    geom, seed = geoms[mesh], sl.seed_for(mesh, partition)
    s = sl.make_oracle(T, geom, 0.05)
    sl.check_kkt_and_objective(fake_group(T, geom, n_ranks), s, partition, seed)
    sl.check_stage_orders(fake_group(T, geom, n_ranks), fake_group(T, geom, n_ranks), s, partition, seed)
    sl.check_layout(fake_group(T, geom, n_ranks), fake_group(T, geom, n_ranks), s, partition, seed)


# ---- deliberate defects: every one must fail a check ------------------------------------------------------------------------------------
STEP_DEFECTS = ("recv_nsq_zero", "recv_x_zero", "stale_tail", "stale_phi_hi", "to_slab_shift")
DEFECT_PARTITIONS = [(1, 2), (5, 6), (4, 8), (6, 3), (8, 2), (31, 3), (64, 5)]


def defective_scenario(geoms, defect, name, partition, mesh="ops_ico1"):
    T, n_ranks = partition
    s = sl.make_oracle(T, geoms[mesh], 0.05)
    group = fake_group(T, geoms[mesh], n_ranks, defect=defect)
    dev = sl.SlabDevice(group, partition, defect=defect)
    dev.set_params(**sc.device_params(s))
    sc.scenario(name)(dev, s, T, seed=sl.seed_for(mesh, partition), expect=lambda *a, **k: None)


@pytest.mark.parametrize("defect", STEP_DEFECTS)
def test_check_one_step_catches_a_defective_exchange(geoms, defect):
    """recv_nsq taken as zero (the cone norm of a slab's last interval loses a half), recv_x taken as zero (the right-hand side of a slab's
    first node), the tail of x_send left from the step before (the multiplier of the interval across the boundary), phi_hi not refreshed,
    the s = 1 half of a corner array one node late in to_slab: ``check_one_step`` fails on EVERY partition with a slab boundary (the last
    one: on every partition with a slab of more than one node) -- and passes without the defect (test_scenarios_on_local_ranks).

    What the max-norm figure of test_hip_sharded.test_slab_iterations_equal_the_single_context would have let through:
    test_what_the_max_norm_figure_lets_through below."""
    assert set(STEP_DEFECTS) - {"to_slab_shift"} <= set(DEFECTS)
    for partition in DEFECT_PARTITIONS:
        parts = sl.PARTITIONS[partition][0]
        reaches = max(nl for nl, _ in parts) > 1 if defect == "to_slab_shift" else len(sl.first_nodes(partition)) > 1
        for name in ("plain", "carry"):
            if reaches:
                with pytest.raises(AssertionError):
                    defective_scenario(geoms, defect, name, partition)
            else:
                defective_scenario(geoms, defect, name, partition)


def test_compare_kkt_catches_missing_halos(geoms):
    """mu_lo and B_hi left out of conditions 2, 4 and 5: each of the three fails ``compare_kkt`` on every partition with a slab boundary;
    the step itself is untouched."""
    for partition in DEFECT_PARTITIONS:
        T, n_ranks = partition
        s = sl.make_oracle(T, geoms["ops_ico1"], 0.05)
        dev = sl.SlabDevice(fake_group(T, geoms["ops_ico1"], n_ranks, defect="kkt_halos_missing"), partition)
        before = sl.plant(dev, s, T)
        dev.step_flags()
        dev.step(1, wait=False)
        after = dev.download_all()
        sc.check_one_step(s, before, after)
        got = dev.kkt(range(7))
        sc.compare_kkt(s, after, got, conditions=(0, 1, 3, 6))
        for i in (2, 4, 5):
            with pytest.raises(AssertionError):
                sc.compare_kkt(s, after, got, conditions=(i,))


def test_palm_catches_phi_uploaded_without_the_next_node(geoms):
    """A slab's steps 2+3, step 0 of is_palm and its KKT sums read phi at the NEXT slab's first node, which only its own inverse transform
    writes -- unless the upload brings it along (DeviceProblem.to_slab(..., with_next_node=True) cuts phi with that row).  Uploaded without it, the palm scenario
    fails ``check_one_step`` on every partition with a slab boundary; no other scenario reads the node before a solve has written it."""
    for partition in DEFECT_PARTITIONS:
        for name in ("plain", "carry", "palm"):
            if name == "palm" and len(sl.first_nodes(partition)) > 1:
                with pytest.raises(AssertionError):
                    defective_scenario(geoms, "phi_without_next_node", name, partition)
            else:
                defective_scenario(geoms, "phi_without_next_node", name, partition)


def test_what_the_max_norm_figure_lets_through():
    """The only entry-wise slab check there was, test_hip_sharded.test_slab_iterations_equal_the_single_context: ops_torus8x6, T = 5, white
    noise, two iterations without a flag, max|got - want| <= 1e-12 max|want| per array, KKT residuals at 1e-10.  Played here with a LOCAL
    stand-in with and without each defect (the figure is the difference between the two runs, so the stand-in's own solve stays out of it).
    Measured: each of the first five defects moves some array by 0.5 to 11 times its largest entry on 2, 3 and 4 ranks, and the missing
    KKT halos move a residual by 2 % or more: in this gross form that test would have caught them -- except the shifted s = 1 half on 6
    ranks (one node per slab: nothing to shift).  It lets through phi uploaded without the next slab's first node, with a figure of exactly
    0 on every rank count: without DOTS_STEP_PALM the first solve overwrites the node before anything reads it.  And being a max-norm, it
    cannot see an error confined to entries far below the largest one; the planted columns exactly on the cone's boundaries are such entries."""
    import os

    from conftest import GOLDEN_DIR

    g = np.load(os.path.join(GOLDEN_DIR, "ops_torus8x6.npz"))
    geom, T = dict(vertices=g["vertices"], triangles=g["triangles"], mu0=g["mu0"], mu1=g["mu1"]), int(g["n_time"])
    assert T == 5
    s = sc.O.OracleSolver(T, geom)
    mass = s.mass_v[None, :]

    def run(n_ranks, defect):
        rng = np.random.default_rng(3)
        state = {k: rng.standard_normal(getattr(s, k).shape) for k in sc.O.OracleSolver.STATE}
        group = fake_group(T, geom, n_ranks, defect=defect)
        dev = sl.SlabDevice(group, defect=defect)
        dev.set_params(r=1.3, scale_z=2.0, const_d=2.0, congestion=0.07)
        for k, v in state.items():
            dev.upload(k, v)
        for _ in range(2):
            group.iterate()
        out = dev.download_all()
        out["phi"] = out["phi"] - np.sum(out["phi"] * mass) / (np.sum(mass) * (T + 1))
        return out, group.kkt(list(range(7)))

    for n_ranks in (2, 3, 6):
        want, want_kkt = run(n_ranks, None)
        for defect in STEP_DEFECTS + ("kkt_halos_missing", "phi_without_next_node"):
            got, got_kkt = run(n_ranks, defect)
            arrays = max(float(np.max(np.abs(got[k] - want[k])) / np.max(np.abs(want[k]))) for k in sc.STATE)
            kkt = max(abs(got_kkt[i][0] - want_kkt[i][0]) / abs(want_kkt[i][0]) for i in range(7))
            if defect == "phi_without_next_node" or (defect == "to_slab_shift" and n_ranks == 6):
                assert arrays == 0.0 and kkt == 0.0, (defect, n_ranks, arrays, kkt)
            elif defect == "kkt_halos_missing":
                assert arrays == 0.0 and kkt > 1e-2, (defect, n_ranks, arrays, kkt)
            else:
                assert arrays > 0.5, (defect, n_ranks, arrays)

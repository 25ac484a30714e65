"""The TIME-SLAB iteration (dots_slab_stage 0 / 1 or 6, 5 / 2 / 3 / 4) against the fp64 oracle, entry by entry, on planted states.

The multi-GPU path is a second implementation of the ALM iteration: k_rhs<CARRIED> with X_lo, the stand-alone k_soc_projection with the
recv_nsq halo, k_slab_pack_iteration<CARRIED> / k_slab_pack_kkt / k_slab_append_multiplier, steps 2+3 with phi_hi, the KKT bodies with
mu_lo and B_hi, the gathered time transforms, the slab layouts of k_convert and a time pitch of its own.  Here n slabs live in one process
on one GPU (tests/slab_checks.py: SlabGroup, the exchanges are plain copies) and run the scenarios of tests/step_checks.py through
``SlabDevice``: the state after each step against the oracle (step_checks.check_one_step: phi within 1e-9, the other eleven arrays within
1e-12 entry by entry, NaN where and only where the oracle has NaN), the launcher's record (dots_debug_counter 12) of every rank that holds
nodes against LITERAL expectations, both stage orders bit for bit, the seven KKT residuals and the objective across the slab boundaries,
and the host layouts.  The planted states put a zero pre-image and a column on each boundary of the cone on the last interval of the first
slab, the first interval of the second and the interval that ends at a single-node slab (slab_checks.slab_cells); every partition of
slab_checks.PARTITIONS runs (slab pitches 4 to 256, single-node and empty ranks, one rank alone).

What the launchers take on a slab (kernels_alm.hip: launch_rhs, launch_soc_projection, launch_q_lambda_mult; dots_api.hip: slab_stage):
k_rhs, never a mode kernel; the projection riding in it (stage 1) or alone (stages 6, 5); k_q_lambda_mult_carry with Z = 1 when
DOTS_STEP_CARRY was asked and a factor is installed at a pitch of at most 128 -- z_mid is never deferred on a slab -- else
k_q_lambda_mult_triangle2; DOTS_STEP_KKT_SUMS is ignored; dots_adjust_penalty divides at once, so no launch ever carries a DIV argument.

Found by the ``palm`` scenario: a slab reads phi at the next slab's first node (phi_hi), which only its own inverse transform wrote; after an
upload step 0 of DOTS_STEP_PALM (and a KKT evaluation) read the value of the last solve -- zero on a fresh context.  dots_upload now
takes that node as one more row of phi (DeviceProblem.to_slab(..., with_next_node=True) cuts it so); tests/test_slab_checks_cpu.py plays the upload without it.
T = 63 on 4 and on 5 ranks (both slab pitch 16) agree bit for bit after two carried steps; nothing of the issue's list was left out.

MEASURED on an MI355X (worst figure per array over all cases of a partition, test_slab_step_against_oracle and
test_kkt_and_objective_across_slab_boundaries; bounds 1e-9 for phi, 1e-12 for the rest; T6x3 and T127x2 include the Jacobi PCG, whose
phi is as good as cg_tol = 1e-13 makes it).  The whole module takes 10 s.
    partition cases      phi        A        B lambda_c    z_fst    z_mid    z_end       mu        E beta_fst beta_mid beta_end
    T1x2         13  2.8e-15  3.0e-16  1.6e-15  2.5e-16  2.4e-16  6.8e-16  1.3e-16  4.2e-16  3.6e-15  7.4e-16  2.7e-15  5.6e-16
    T5x6         13  1.7e-15  3.9e-16  2.0e-15  1.1e-15  2.5e-16  6.3e-16  3.1e-16  1.5e-15  3.6e-15  5.0e-16  3.2e-15  1.2e-15
    T4x8         13  2.8e-15  4.9e-16  1.3e-15  3.9e-16  2.5e-16  8.3e-16  4.1e-16  1.3e-15  2.7e-15  4.9e-16  4.1e-15  1.1e-15
    T6x3         41  5.0e-13  3.9e-16  1.8e-15  1.1e-15  5.0e-16  1.4e-15  6.4e-16  1.4e-15  3.1e-15  1.0e-15  4.7e-15  2.6e-15
    T8x2         13  3.7e-15  3.5e-16  1.6e-15  5.0e-16  3.7e-16  7.7e-16  2.9e-16  6.0e-16  3.5e-15  6.4e-16  4.1e-15  6.5e-16
    T31x3        13  1.1e-13  4.2e-16  1.4e-15  1.0e-15  2.8e-16  9.0e-16  4.5e-16  1.2e-15  3.1e-15  6.8e-16  4.2e-15  1.2e-15
    T31x1        13  8.3e-14  4.3e-16  1.6e-15  9.4e-16  2.9e-16  9.2e-16  4.2e-16  1.1e-15  3.2e-15  8.3e-16  5.2e-15  1.2e-15
    T63x2        13  3.8e-13  4.4e-16  1.5e-15  1.8e-15  3.1e-16  8.7e-16  3.4e-16  1.2e-15  4.1e-15  7.8e-16  5.3e-15  1.3e-15
    T64x5        13  5.0e-13  4.6e-16  1.6e-15  7.1e-16  3.7e-16  8.6e-16  3.7e-16  8.3e-16  3.4e-15  8.0e-16  6.3e-15  1.2e-15
    T127x2       41  5.2e-11  5.5e-16  1.6e-15  2.1e-15  5.7e-16  1.9e-15  4.9e-16  1.7e-15  4.6e-15  5.7e-15  5.3e-15  6.8e-15
    T255x2       13  1.6e-12  5.2e-16  1.6e-15  1.8e-15  3.7e-16  1.1e-15  4.1e-16  1.1e-15  3.8e-15  8.6e-16  4.8e-15  1.8e-15
    T255x1       13  1.5e-12  4.6e-16  1.6e-15  1.8e-15  3.7e-16  1.0e-15  4.4e-16  1.2e-15  3.5e-15  7.9e-16  5.3e-15  1.8e-15
"""
import numpy as np
import pytest

import slab_checks as sl
import step_checks as sc

pytestmark = pytest.mark.gpu
MESHES = ("ops_ico1", "fan")      # closed, valence 5 (V = 12); a boundary and valences 1, 2 and 9 (V = 11)
ALL = list(sl.PARTITIONS)

# dots_debug_counter 12 (csrc/step_choice.h: STEP_PATH_*), written out
RHS, RHS_CARRIED, SOC_RIDER, SOC_ALONE, QL_TRIANGLE2, QL_CARRY, QL_BMNT = 1, 16, 64, 128, 512, 1024, 1 << 15
Z1, Z2 = 1 << 11, 2 << 11


def slab_launches(name, split, carries):
    """The record after every step of a scenario.  ``carries``: direct solver at a slab pitch of at most 128."""
    soc = SOC_ALONE if split else SOC_RIDER
    plain = RHS | soc | QL_TRIANGLE2 | Z1
    carry = RHS | soc | QL_CARRY | Z1 if carries else plain
    carried = carry | RHS_CARRIED if carries else plain
    return {
        "plain": [plain],
        "carry": [carry, carried],
        "pending_division": [carry],                                # (divided at once: no DIV; DOTS_STEP_CARRY was asked)
        "skip_z_mid": [RHS | soc | QL_TRIANGLE2 | Z2, plain],
        "pending_after_carry": [carry, carry],                      # (the parameters changed in between: the carried sums are dropped)
        "timed": [plain],
        "timed_carry": [carry, carried],
        "palm": [plain],
    }[name]


@pytest.fixture(scope="module")
def geoms():
    return {m: sc.geometry(m) for m in MESHES}


def device_group(T, geom, n_ranks, direct=True, eps=0.0, buffers_last=False):
    """``buffers_last``: the exchange buffers are set after the factor is installed (ShardedAlmSolver's order), not before."""
    group = sl.SlabGroup(T, geom, n_ranks, defer_buffers=buffers_last)
    for d in group.devs:
        if direct and d.nl:
            assert d.setup_frontal(eps=eps, leaf=4)["levels"] >= 1      # (the factor is that of K + (sigma + eps) M)
        elif not direct:
            d.set_params(cg_tol=1e-13)                              # Jacobi PCG
    if buffers_last:
        group.set_buffers()
    return group


def cases():
    """(scenario, mesh, partition, congestion, eps, split, direct): plain, carry and pending_division on every partition, both meshes and
    congestions (the stage order alternates); the rest, eps = 1e-2 and the Jacobi PCG on one small-pitch and one pitch-64 partition."""
    out, i = [], 0
    for name in sc.SCENARIOS_ALL_T:
        for p in ALL:
            for mesh in MESHES:
                for congestion in (0.0, 0.05):
                    out.append((name, mesh, p, congestion, 0.0, bool(i % 2), True))
                    i += 1
                i += 1
    few = (sl.SMALL_PITCH, sl.LARGE_PITCH)
    for name in ("skip_z_mid", "pending_after_carry", "timed", "timed_carry", "palm"):
        for p in few:
            for mesh in MESHES:
                for congestion in (0.0, 0.05):
                    out.append((name, mesh, p, congestion, 0.0, bool(i % 2), True))
                    i += 1
                i += 1
    for p in few:
        for mesh in MESHES:
            for name in ("plain", "carry"):
                out.append((name, mesh, p, 0.05, 1e-2, bool(i % 2), True))
                i += 1
            for congestion in (0.0, 0.05):
                out.append(("plain", mesh, p, congestion, 0.0, bool(i % 2), False))
                i += 1
    return out


def case_id(v):
    return sl.partition_id(v) if isinstance(v, tuple) else None


def record_figures(monkeypatch, record_property):
    """Every check_one_step of the test leaves its worst figure per array in the test's properties."""
    worst = {}
    inner = sc.check_one_step

    def recording(*a, **kw):
        figures = inner(*a, **kw)
        for k, v in figures.items():
            worst[k] = max(worst.get(k, 0.0), v)
            record_property("worst_" + k, worst[k])
        return figures

    monkeypatch.setattr(sc, "check_one_step", recording)
    return worst


@pytest.mark.parametrize("name,mesh,partition,congestion,eps,split,direct", cases(), ids=case_id)
def test_slab_step_against_oracle(geoms, monkeypatch, record_property, name, mesh, partition, congestion, eps, split, direct):
    from dots_socp_amd import _lib

    P = _lib.STEP_PATH
    assert (P["rhs"], P["rhs_carried"], P["soc_rider"], P["soc_alone"], P["ql_triangle2"], P["ql_carry"], P["ql_bmnt"], _lib.STEP_PATH_QL_Z_SHIFT) == \
           (RHS, RHS_CARRIED, SOC_RIDER, SOC_ALONE, QL_TRIANGLE2, QL_CARRY, QL_BMNT, 11)
    T, n_ranks = partition
    record_figures(monkeypatch, record_property)
    s = sl.make_oracle(T, geoms[mesh], congestion, eps)
    group = device_group(T, geoms[mesh], n_ranks, direct, eps)
    holders = [d for d in group.devs if d.nl]
    assert [(d.nl, d.ni) for d in group.devs] == list(sl.PARTITIONS[partition][0])
    want = slab_launches(name, split, carries=direct and sl.PARTITIONS[partition][1] <= sl.CARRY_MAX_PITCH)
    steps = []

    def expect(dev, **_single_context_bits):
        for d in holders:
            got = d.debug_counter(_lib.STEP_PATH_COUNTER)
            if want[len(steps)] & QL_CARRY:      # BMNT follows the rule of dots_front_setup (dots_debug_counter 6), whatever it decided here
                assert bool(got & QL_BMNT) == bool(d.debug_counter(6))
            assert got & ~QL_BMNT == want[len(steps)], (len(steps), d.slab, hex(got), hex(want[len(steps)]))
        steps.append(1)

    try:
        assert all(d.debug_counter(_lib.STEP_PATH_COUNTER) == 0 for d in group.devs)      # nothing enqueued yet
        dev = sl.run_scenario(group, name, s, partition, sl.seed_for(mesh, partition), split=split, expect=expect)
        assert len(steps) == len(want)
        dev.upload("mu", dev.download("mu"))                                                # a change of state ends the record
        assert all(c == 0 for c in dev.debug_counter(_lib.STEP_PATH_COUNTER))
    finally:
        group.close()


@pytest.mark.parametrize("partition", ALL, ids=sl.partition_id)
def test_stage_orders_are_bit_identical(geoms, partition):
    T, n_ranks = partition
    mesh = MESHES[ALL.index(partition) % 2]
    s = sl.make_oracle(T, geoms[mesh], 0.05)
    a, b = device_group(T, geoms[mesh], n_ranks), device_group(T, geoms[mesh], n_ranks)
    try:
        sl.check_stage_orders(a, b, s, partition, sl.seed_for(mesh, partition))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("partition", ALL, ids=sl.partition_id)
def test_kkt_and_objective_across_slab_boundaries(geoms, monkeypatch, record_property, partition):
    T, n_ranks = partition
    mesh = MESHES[(ALL.index(partition) + 1) % 2]
    record_figures(monkeypatch, record_property)
    s = sl.make_oracle(T, geoms[mesh], 0.05)
    group = device_group(T, geoms[mesh], n_ranks)
    try:
        sl.check_kkt_and_objective(group, s, partition, sl.seed_for(mesh, partition))
    finally:
        group.close()


@pytest.mark.parametrize("partition", ALL, ids=sl.partition_id)
def test_slab_layouts(geoms, partition):
    T, n_ranks = partition
    mesh = MESHES[ALL.index(partition) % 2]
    s = sl.make_oracle(T, geoms[mesh], 0.05)
    a, b = device_group(T, geoms[mesh], n_ranks), device_group(T, geoms[mesh], n_ranks)
    try:
        sl.check_layout(a, b, s, partition, sl.seed_for(mesh, partition))
    finally:
        a.close()
        b.close()


def test_rank_counts_of_equal_slab_pitch_are_bit_identical(geoms):
    """T = 63 on 4 ranks (16 nodes each) and on 5 (13, 13, 13, 13, 12): both slab pitch 16, direct solver, two carried steps."""
    T, mesh = 63, "fan"
    s = sl.make_oracle(T, geoms[mesh], 0.05)
    out = []
    for n_ranks in (4, 5):
        group = device_group(T, geoms[mesh], n_ranks)
        try:
            assert max(4, 1 << (group.devs[0].slab[2] - 1).bit_length()) == 16
            dev = sl.SlabDevice(group)
            sl.plant(dev, s, T)
            dev.step_flags(carry=True)
            dev.step(2, wait=False)
            assert all(d.debug_counter(12) & RHS_CARRIED for d in group.devs if d.nl)
            out.append(dev.download_all())
        finally:
            group.close()
    for k in sc.STATE:
        assert np.array_equal(out[0][k], out[1][k]), k


def test_factor_and_buffers_in_either_order_are_bit_identical(geoms):
    """The factor installed before dots_slab_set_buffers (the driver's order) and after it (this module's): direct solver, two carried
    steps on T6x3.  The installation allocates the carried gathers (cn_sq, cn_g, cn_lo, cn_e) and the buffers set the halo pointers; the
    PCG's and the transforms' views of a slab are derived from the context's one Dev when a launch needs them, so neither call can leave
    a view behind the other.  After each step all twelve arrays of every rank carry the same bits and every rank took the same launches."""
    from dots_socp_amd import _lib

    partition, mesh = sl.SMALL_PITCH, "fan"
    assert sl.partition_id(partition) == "T6x3"
    T, n_ranks = partition
    seen = []
    for buffers_last in (True, False):
        s = sl.make_oracle(T, geoms[mesh])
        group = device_group(T, geoms[mesh], n_ranks, buffers_last=buffers_last)
        holders = [d for d in group.devs if d.nl]
        steps = []

        def expect(dev, **_single_context_bits):
            steps.append(([d.debug_counter(_lib.STEP_PATH_COUNTER) for d in holders], [{k: d.download(k) for k in sc.STATE} for d in holders]))

        try:
            sl.run_scenario(group, "carry", s, partition, sl.seed_for(mesh, partition), expect=expect)
        finally:
            group.close()
        assert len(steps) == 2 and all(p & QL_CARRY for p in steps[0][0]) and all(p & RHS_CARRIED for p in steps[1][0])
        seen.append(steps)
    for (paths_a, ranks_a), (paths_b, ranks_b) in zip(*seen):
        assert paths_a == paths_b
        assert len(ranks_a) == len(ranks_b) == 3
        for a, b in zip(ranks_a, ranks_b):
            for k in sc.STATE:
                assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k

"""The 22 KKT sums, the 3 objective sums and dots_norm_square, slot by slot and route by route, against the long-double reference of
tests/kkt_checks.py.

These sums decide when a solve stops, when the penalty moves and how the state is rescaled; the other tests compare only the seven
combined ratios res / (c + nsum), on white noise, where an error in one slot can hide behind the constant or a norm sum.  Here every
slot of dots_kkt_sums, dots_objective_sums and dots_norm_square (all twelve arrays, parts 1 and 2 of phi) is compared on its own with
``kkt_checks.reference``, within MARGIN = 16 times max(|plain fp64 - reference|, the reference's running error bound); a slot whose
reference is exactly 0 must be exactly 0.0.  Nothing in a tolerance comes from the device.

STATES.  ``white``: the recipe of random_state.  ``converged``: the oracle's own iterate after 10, 60 and 300 iterations from its start (10 and 300 above T = 64),
then scale_prim_dual(3, 0.625), uploaded with the oracle's r, scale_z, const_d, norm_d, norm_boundary, congestion and the prim, dual and
boundary scales (3, 0.625 and 1.6): at k = 300 the residual slots of conditions 0, 1, 3 are below 1e-12 of their norm slots (differences of
nearly equal numbers).  ``probe``: all arrays zero except on one small support, const_d = 0: a slot is the contribution of the support
and every slot it cannot reach must be 0.0 -- time node / interval 0, 1, T - 1, T alone, the pair of an even lane and of the last lane,
a boundary vertex, the vertex of largest odd valence, the first and last vertex of the first and of the last vertex tile and the first
and last row of the last triangle-row tile, in the DEVICE numbering of the plan.

ROUTES.
(a), (e) test_standalone_sums_slot_by_slot: dots_kkt_sums with one node per lane (DOTS_KKT_TWO=0) and with two, dots_objective_sums,
    dots_norm_square; all 22 slots for the mask of all seven conditions, each condition alone holds the same bits in the slots it
    needs, a second call repeats the bits.  fan (V = 11, open, valences 9, 2, 1) and ops_ico1 (V = 42) at T = 1, 2, 6, 7, 8, 15, 20, 31, 63,
    64, 255, 300, 1023 (every pitch from 8 to 1024); meshes.plane(20) (V = 504, F = 920, open; at pitch 32: 16 vertex tiles with a
    ragged last one, 87 triangle-row tiles, so the XCD remap is not the identity and one workgroup slot is idle) at every T up to
    pitch 128, reorder=True and "nd"; congestion 0 and 0.05.  No counter tells the one-node from the two-node bodies: the
    environment switch read at dots_create is what selects them.
(b) test_sums_left_by_steps_2_and_3: see its docstring (DOTS_STEP_KKT_SUMS with and without DOTS_STEP_CARRY, a pending penalty
    division, DOTS_STEP_SKIP_Z_MID; the norms of z_mid and beta_mid after a carried and after a lazily divided step).
(c) test_reduction_routes_hold_the_same_bits: dots_kkt_sums_device and the mailbox's fallback hold the bits of (a), at pitch 8 and 128.
(d) test_slab_shares_slot_by_slot: time slabs on one GPU, T = 6 and 7 on 3 ranks, T = 63 on 2: every slab's share against
    ``reference(..., slab)``, the slot-wise total against the reference of the whole problem.

LEFT OUT, AND WHY.  The route of fetch_sums without a mailbox: the library has no switch that takes the mailbox away (every context
allocates one).  DOTS_STEP_SKIP_Z_MID switches DOTS_STEP_KKT_SUMS off (dots_step_flags), so there are no fused sums after such a step:
the slots of conditions 0, 2, 3, 6 are then read through the stand-alone kernels and condition 1 is refused (asserted).  Above pitch
128 steps 2+3 leave no sums either (no carry mapping): T = 255 and 300 in (b) check the stand-alone kernels on the state a step left.
THINNED (run time).  The converged iterates run at every T on the two small meshes: k = 10, 60, 300 up to T = 64, k = 10 and 300
at T = 255, 300 and 1023, at both congestions (300 oracle iterations take 5 s on ops_ico1 at T = 255 and 20 s at
T = 1023: a sparse solve per time mode and iteration); on the plane at T = 7 (both congestions) and T = 31 (0.05).  The probes run at
congestion 0.05 only (a support does not depend on it): all of them at every T on the two small meshes; on the plane only the vertex,
row and last-lane probes (a time support there costs a long-double pass over 10^6 entries), at every T with reorder=True and at
T = 7, 31, 64 with "nd".  No shape and no route was thinned.

MUTATIONS (tests/test_kkt_checks_cpu.py plays them through ``kkt_checks.plain`` and asserts which states reject each; fan at T = 7
and ops_ico1 at T = 63):
    last_interval, pair_reads_t1, odd_corner, mu0_interval, ragged_tile, neighbour_area, rmid_last_half, dphi_rounded, objective_node,
    norm_extra_column: rejected on white noise, on the converged iterates and by at least one probe;
    mu1_sign: white noise and the converged iterates (and the probes that hold node T);
    cong_prim_scale: the converged iterates only (the scales are 1 elsewhere) -- the one defect of the twelve that the existing figure
    (compare_kkt at 1e-11 on white noise) lets through.

MEASURED on an MI355X, 2026-10-20: worst |got - reference| / tolerance per route and kind of state (1 would fail).  No slot missed its
bound and no defect was found: the library is unchanged.  The tolerances are dominated by the reduction's N 2^-53 share of the bound
(N up to 10^6 entries), the device's pairwise sums stay a factor of 100 and more below it; the probes and the converged states are
what makes the check sharp (a defect confined to a support shows at full relative size, as the CPU file demonstrates).  The whole
module takes 85 s, most of it the oracle's iterations and the long-double passes on the host.
    stand-alone, one node per lane     white 0.005   converged 0.009   probe 0.006
    stand-alone, two nodes per lane    white 0.005   converged 0.009   probe 0.006
    after a step, carry = 0            plain 0.001   pending division 0.001   skip_z_mid 0.001
    after a step, carry = 1            plain 0.001   pending division 0.001   skip_z_mid 0.001
    time slabs (shares and totals)     white 0.007
    device buffer, mailbox fallback    bit for bit
"""
import functools

import numpy as np
import pytest

import kkt_checks as kc
import slab_checks as sl
import step_checks as sc

pytestmark = pytest.mark.gpu

T_ALL = (1, 2, 6, 7, 8, 15, 20, 31, 63, 64, 255, 300, 1023)      # pitches 8 8 8 8 16 16 32 32 64 128 256 512 1024
T_PLANE = tuple(t for t in T_ALL if kc.pitch_of(t) <= 128)
T_PLANE_PROBES = {True: T_PLANE, "nd": (7, 31, 64)}
CONGESTIONS = (0.0, 0.05)
STEP_CONDITIONS = (0, 1, 2, 3, 6)                                 # what steps 2+3 leave sums for (plus Dual(alpha)'s vertex pass)
# dots_debug_counter 12 (include/dots_socp_hip.h), written out
DIV, Z_MODE, Z_REBUILD_ONLY, FUSED_KKT, QL_DIV = 32, 3 << 11, 2 << 11, 8192, 16384
FACTOR = 1.7

WORST = {}      # (route, kind of state) -> worst |got - ref| / tolerance seen by this process


def note(route, kind, q):
    WORST[(route, kind)] = max(WORST.get((route, kind), 0.0), float(q))


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    print("\nworst |got - ref| / tolerance per route and state:")
    for (route, kind), q in sorted(WORST.items()):
        print(f"    {route:<28s} {kind:<10s} {q:.3f}")


@functools.lru_cache(maxsize=None)
def geometry(mesh):
    return kc.plane_geometry(20) if mesh == "plane20" else sc.geometry(mesh)


@functools.lru_cache(maxsize=4)
def oracle(mesh, T):
    return sc.make_oracle(T, geometry(mesh), 0.0)


class Expected:
    """state, parameters, reference values and tolerances of one (case, state): formed once, shared by the routes and never written."""

    def __init__(self, kind, name, s, state, params, slab=None):
        self.kind, self.name, self.s, self.state, self.params = kind, name, s, state, params
        ref, pl = kc.reference(s, state, params, slab=slab), kc.plain(s, state, params, slab=slab)
        self.names, self.ref, self.tol = kc.tolerances(ref, pl)
        for a in (self.ref, self.tol):
            a.setflags(write=False)


def converged_ks(mesh, T, congestion):
    """The iteration counts of the converged iterates of a case (none: no converged state).  300 oracle iterations cost 0.05 s on the
    fan at T = 7, 5 s on ops_ico1 at T = 255 and 20 s there at T = 1023 (a sparse solve per time mode and iteration)."""
    if mesh == "plane20":
        return kc.CONVERGED_K if (T == 7 or (T == 31 and congestion)) else ()
    return kc.CONVERGED_K if T <= 64 else (10, 300)


def case_states(mesh, T, congestion, numbering, probes):
    """The states of one case, lazily: white noise, the converged iterates, the probes asked for."""
    geom, s = geometry(mesh), oracle(mesh, T)
    yield Expected("white", "white", s, kc.white(s, 1000 + T), dict(kc.params_of(s, geom), congestion=congestion))
    ks = converged_ks(mesh, T, congestion)
    for k, (sk, st, p) in zip(ks, kc.converged(T, geom, congestion, ks) if ks else ()):
        yield Expected("converged", f"converged{k}", sk, st, p)
    if congestion == CONGESTIONS[-1]:      # (a probe's support does not depend on the congestion: one of the two)
        for name, support in kc.probe_supports(s, numbering).items():
            if probes(name):
                yield Expected("probe", name, s, kc.probe(s, support), dict(kc.probe_params(s, geom), congestion=congestion))


def probe_filter(mesh, reorder, T):
    """Every probe on the small meshes; on the plane the vertex, row and last-lane probes at the T of ``T_PLANE_PROBES``."""
    if mesh != "plane20":
        return lambda name: True
    return lambda name: T in T_PLANE_PROBES[reorder] and name.startswith(("boundary", "odd", "device", "lastpair"))


def load_state(dev, e):
    for k in sc.STATE:
        dev.upload(k, e.state[k])
    dev.set_params(**kc.device_params(e.s, e.params))


def read_all(dev):
    """Everything ``kkt_checks.flat`` lists, from the stand-alone entry points."""
    sums = dev.kkt_sums(range(7))
    assert sums.shape == (24,) and not sums[kc.N_SUMS:].any()
    return sums, kc.device_vector(sums, dev.objective_sums(), {k: dev.norm_square(*k) for k in kc.NORMS})


def make_device(mesh, T, reorder=True, direct=False):
    from dots_socp_amd.device import DeviceProblem

    dev = DeviceProblem(T, geometry(mesh), lap_solver="modal_pcg", reorder=reorder)
    if direct:
        dev.setup_frontal(leaf=4)
    return dev


def standalone_cases():
    out = [(mesh, True, T, c) for mesh in ("fan", "ops_ico1") for T in T_ALL for c in CONGESTIONS]
    return out + [("plane20", reorder, T, c) for reorder in (True, "nd") for T in T_PLANE for c in CONGESTIONS]


# ---- (a) + (e): the stand-alone kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,reorder,T,congestion", standalone_cases())
def test_standalone_sums_slot_by_slot(mesh, reorder, T, congestion, monkeypatch, record_property):
    """dots_kkt_sums with one node per lane (DOTS_KKT_TWO=0) and with two, dots_objective_sums and dots_norm_square of all twelve arrays
    and of both parts of phi, on white noise, converged iterates and the probes: every slot within its tolerance and exactly 0.0 where
    the reference is; every condition alone gives the bits of the full mask in the slots it needs; a second call repeats the bits."""
    devs = {}
    for two in ("0", "1"):
        monkeypatch.setenv("DOTS_KKT_TWO", two)
        devs[two] = make_device(mesh, T, reorder)
    nb = kc.Numbering.of_plan(devs["0"].plan)
    worst = {}
    try:
        for e in case_states(mesh, T, congestion, nb, probe_filter(mesh, reorder, T)):
            for two, dev in devs.items():
                load_state(dev, e)
                sums, got = read_all(dev)
                what = f"{mesh} reorder={reorder} T={T} cong={congestion} {e.name} two={two}"
                q = kc.assert_within(got, e.names, e.ref, e.tol, what)
                key = (f"stand-alone two={two}", e.kind)
                worst[key] = max(worst.get(key, 0.0), q)
                assert np.array_equal(dev.kkt_sums(range(7)), sums), what
                for i in range(7):
                    one = dev.kkt_sums([i])
                    for k in kc.SLOTS:
                        if i in kc.NEEDS[k]:
                            assert one[kc.IX[k]] == sums[kc.IX[k]], (what, i, k)
    finally:
        for dev in devs.values():
            dev.close()
    for key, q in worst.items():
        note(*key, q)
        record_property(f"{key[0]} {key[1]}", q)
    print(f"{mesh} reorder={reorder} T={T} cong={congestion}: " + ", ".join(f"{k[0]} {k[1]} {q:.3f}" for k, q in sorted(worst.items())))


# ---- (b): the sums steps 2+3 leave ------------------------------------------------------------------------------------------------------
def step_cases():
    out = [(mesh, T, carry) for mesh in ("fan", "ops_ico1") for T in (7, 31, 64, 255) for carry in (False, True)]
    return out + [("plane20", 31, True), ("ops_ico1", 300, False)]


def slots_of(conditions):
    return [kc.IX[k] for k in kc.SLOTS if set(kc.NEEDS[k]) & set(conditions)]


def compare_step_slots(dev, params, s, got, norms, conditions=STEP_CONDITIONS):
    """``got`` (the sums read before any download) against the reference on the state the context holds now.  Without condition 1
    nothing reads z_mid: it is not downloaded (zeros stand in for it)."""
    after = {k: dev.download(k) for k in sc.STATE if k != "z_mid" or 1 in conditions}
    after.setdefault("z_mid", np.zeros(s.z_mid.shape))
    ref, pl = kc.reference(s, after, params), kc.plain(s, after, params)
    names, r, tol = kc.tolerances(ref, pl)
    idx = slots_of(conditions)
    q = kc.assert_within(got[idx], [names[i] for i in idx], r[idx], tol[idx], "sums after a step")
    for k, v in norms.items():
        i = names.index(f"norm.{k[0]}.{k[1]}")
        q = max(q, kc.assert_within(np.array([v]), [names[i]], r[i:i + 1], tol[i:i + 1], "norm after the step"))
    return q


@pytest.mark.parametrize("mesh,T,carry", step_cases())
def test_sums_left_by_steps_2_and_3(mesh, T, carry, record_property):
    """DOTS_STEP_KKT_SUMS with the direct solver: after a step (plain, then with a penalty division pending) the slots of conditions
    0, 1, 2, 3, 6, read BEFORE any download, against the reference on the state downloaded afterwards; the norms of z_mid and beta_mid
    likewise (after the carried step, and after the lazily divided one).  Counter 12 says that the step formed the sums (8192: at a
    pitch of at most 128, where the carry mapping exists; above it the flag is a hint and the stand-alone kernels read the state the
    step left) and divided as it read (32, 16384).  DOTS_STEP_SKIP_Z_MID switches the fused sums off (dots_step_flags): after such a
    step (bits 11-12 = 2, no 8192) condition 1 is refused and the slots of conditions 0, 2, 3, 6 come from the stand-alone kernels.
    No counter tells whether dots_kkt_sums reduced the fused sums or read the state again (kkt_takes_fused), nor whether Dual(alpha)
    took k_kkt_dual_alpha_carried: the flags of the step and the absence of any call in between are what select them."""
    from dots_socp_amd import _lib

    geom, s = geometry(mesh), oracle(mesh, T)
    corner = (("z_mid", 0), ("beta_mid", 0))
    fuses = kc.pitch_of(T) <= sl.CARRY_MAX_PITCH
    worst = {}
    for congestion in CONGESTIONS:
        state, params = kc.white(s, 2000 + T), dict(kc.params_of(s, geom), congestion=congestion)
        dev = make_device(mesh, T, direct=True)
        try:
            for k in sc.STATE:
                dev.upload(k, state[k])
            dev.set_params(**kc.device_params(s, params))
            # 1. a plain step
            dev.step_flags(carry=carry, kkt_sums=True)
            dev.step(1, wait=False)
            assert bool(dev.debug_counter(12) & FUSED_KKT) == fuses
            got = dev.kkt_sums(STEP_CONDITIONS)
            norms = {k: dev.norm_square(*k) for k in corner}
            worst["plain"] = max(worst.get("plain", 0.0), compare_step_slots(dev, params, s, got, norms))
            # 2. a penalty division left pending
            p2 = dict(params, r=params["r"] * FACTOR)
            dev.adjust_penalty(FACTOR)
            dev.set_params(r=p2["r"])
            dev.step_flags(carry=carry, kkt_sums=True)
            dev.step(1, wait=False)
            path = dev.debug_counter(12)
            assert bool(path & FUSED_KKT) == fuses
            if fuses:
                assert path & DIV and path & QL_DIV, hex(path)
            got = dev.kkt_sums(STEP_CONDITIONS)
            norms = {k: dev.norm_square(*k) for k in corner}
            worst["pending division"] = max(worst.get("pending division", 0.0), compare_step_slots(dev, p2, s, got, norms))
            # 3. skip_z_mid
            if T in (7, 64):
                dev.step_flags(carry=carry, kkt_sums=True, skip_z_mid=True)
                dev.step(1, wait=False)
                path = dev.debug_counter(12)
                assert not path & FUSED_KKT and path & Z_MODE == Z_REBUILD_ONLY, hex(path)
                with pytest.raises(_lib.HipLibraryError, match="kkt: z_mid was not materialised") as refusal:
                    dev.kkt_sums([1])
                assert refusal.value.status == _lib.ERR_STATE
                got = dev.kkt_sums((0, 2, 3, 6))
                norms = {corner[1]: dev.norm_square(*corner[1])}
                worst["skip_z_mid"] = max(worst.get("skip_z_mid", 0.0), compare_step_slots(dev, p2, s, got, norms, conditions=(0, 2, 3, 6)))
        finally:
            dev.close()
    for k, q in worst.items():
        note(f"steps 2+3 carry={int(carry)} {k}", "white", q)
        record_property(k, q)
    print(f"{mesh} T={T} carry={carry}: " + ", ".join(f"{k} {q:.3f}" for k, q in worst.items()))


# ---- (c): the reduction routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,T", [("fan", 7), ("ops_ico1", 64)])
def test_reduction_routes_hold_the_same_bits(mesh, T, monkeypatch):
    """dots_kkt_sums_device into a torch buffer, and the mailbox's fallback (every publish goes astray, the spin cut short: the sums are
    copied from the device scalars and dots_debug_counter 0 counts it), hold the bits of dots_kkt_sums -- which
    test_standalone_sums_slot_by_slot compares with the reference at this shape.  The library has no switch that takes the mailbox away,
    so the route of fetch_sums without one is not reached here."""
    import torch

    geom, s = geometry(mesh), oracle(mesh, T)
    e = Expected("white", "white", s, kc.white(s, 1000 + T), dict(kc.params_of(s, geom), congestion=0.05))
    dev = make_device(mesh, T)
    load_state(dev, e)
    sums, got = read_all(dev)
    kc.assert_within(got, e.names, e.ref, e.tol, "mailbox")
    assert dev.debug_counter(0) == 0
    buf = torch.full((24,), np.nan, dtype=torch.float64, device="cuda")
    masks = [list(range(7)), [4, 5], [2], [0, 1, 3, 6]]
    for conditions in masks:
        dev.kkt_sums_device(conditions, buf.data_ptr())
        dev.sync()
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy()[:kc.N_SUMS], dev.kkt_sums(conditions)[:kc.N_SUMS]), conditions
    dev.close()
    monkeypatch.setenv("DOTS_MAIL_TEST_DROP", "1")
    monkeypatch.setenv("DOTS_MAIL_SPINS", "100")
    dropped = make_device(mesh, T)
    monkeypatch.delenv("DOTS_MAIL_TEST_DROP")
    monkeypatch.delenv("DOTS_MAIL_SPINS")
    load_state(dropped, e)
    before = dropped.debug_counter(0)
    assert np.array_equal(dropped.kkt_sums(range(7)), sums)
    assert np.array_equal(dropped.kkt_sums([4, 5])[:kc.N_SUMS], np.where([bool(set(kc.NEEDS[k]) & {4, 5}) for k in kc.SLOTS], sums[:kc.N_SUMS], 0.0))
    assert dropped.debug_counter(0) == before + 2
    _, again = read_all(dropped)
    assert np.array_equal(again, got)
    assert dropped.debug_counter(0) == before + 2 + 1 + 1 + len(kc.NORMS)
    dropped.close()


# ---- (d): time slabs on one GPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("partition", [(6, 3), (7, 3), (63, 2)], ids=sl.partition_id)
@pytest.mark.parametrize("mesh", ["fan", "ops_ico1"])
def test_slab_shares_slot_by_slot(mesh, partition, record_property):
    """n time slabs in one process (slab_checks.SlabGroup): after the KKT halo exchange every slab's own share of every sum against
    ``reference(..., slab)``, and the slot-wise total against the reference of the whole problem; the objective's sums and the norms
    likewise (a slab's part 1 of phi reads the next slab's first node, which the upload brings)."""
    T, n_ranks = partition
    geom, s = geometry(mesh), oracle(mesh, T)
    worst = 0.0
    group = sl.SlabGroup(T, geom, n_ranks)
    try:
        dev = sl.SlabDevice(group)
        for congestion in CONGESTIONS:
            whole = Expected("white", "white", s, kc.white(s, 3000 + T), dict(kc.params_of(s, geom), congestion=congestion))
            dev.set_params(**kc.device_params(s, whole.params))
            for k in sc.STATE:
                dev.upload(k, whole.state[k])
            group.each(lambda d: d.slab_stage(4))
            group.neighbours(("send_mu", "recv_mu"), ("send_b", "recv_b"))
            total = np.zeros(len(whole.names))
            for d in group.devs:
                sums, got = read_all(d)
                share = Expected("white", "share", s, whole.state, whole.params, slab=(d.node0, d.nl))
                worst = max(worst, kc.assert_within(got, share.names, share.ref, share.tol, f"{mesh} {partition} rank {d.slab[0]}"))
                total += got
            worst = max(worst, kc.assert_within(total, whole.names, whole.ref, whole.tol, f"{mesh} {partition} total"))
    finally:
        group.close()
    note("time slabs", "white", worst)
    record_property("time slabs white", worst)
    print(f"{mesh} {sl.partition_id(partition)}: {worst:.3f}")

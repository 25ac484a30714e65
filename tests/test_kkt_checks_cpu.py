"""tests/kkt_checks.py on the CPU: the slot order against the header, ``combine`` against the oracle, the conditions on the inputs, ``plain``
within the tolerances (the bound is not empty), the deliberate defects (every one rejected slot by slot; which of them the existing
figure lets through is recorded), the geometry tables the bound counts, and the slab shares.

CAUGHT BY (test_every_mutation_is_rejected asserts this table; fan at T = 7 and ops_ico1 at T = 63, congestion 0.05):
    last_interval       white, converged, time probes of the last interval
    pair_reads_t1       white, converged, the probe of node 2 alone (B there is the node t + 2 of interval 1)
    odd_corner          white, converged, the probe of the odd-valence vertex's corners through E: the time probes
    mu1_sign            white, converged (and the probes that hold node T)
    mu0_interval        white, converged, the probe of interval 0
    ragged_tile         white, converged, the probe of the last device vertex (the fan: that vertex alone; ops_ico1: the 10 vertices
                        of the ragged third tile)
    neighbour_area      white, converged, the probe of the last device row (component 2 of the last device triangle: one row)
    rmid_last_half      white, converged, the probe of node T
    cong_prim_scale     converged (the three scales differ from 1 there; on white and the probes prim_scale = dual_scale = 1: void)
    dphi_rounded        white, converged, the time probes (30 bits kept: 1e-9 of V_RESMU2 on white noise, the whole slot where
                        dphi - A - lambda_c cancels)
    objective_node      white, converged, the probe of node T
    norm_extra_column   white, converged, the probe of interval T - 1
LET THROUGH by the existing figure (step_checks.compare_kkt at KKT_TOL = 1e-11 on white noise, the objective at 1e-12 and the norms at
1e-13, as test_kkt_objective_norms_a10_a11_a12 asks): cong_prim_scale alone (void at unit scales, and no existing test evaluates the
residuals at other scales); the other eleven are confined to few entries but not small, and white noise at 1e-11 rejects them too.
Recorded by test_every_mutation_is_rejected, not asserted.

THE INPUTS.  On white noise both branches of fmax(0, aux + rho) occur on more than 10 % of the entries.  On a converged state rho > 0 on
every entry (the end masses are positive) and aux -> 0, so only the branch aux + rho > 0 occurs: the branch that clips to 0 is covered by
white noise and by the probes (rho < 0 on about half of a support).
"""
import numpy as np
import pytest

import kkt_checks as kc
import slab_checks as sl
import step_checks as sc

LD = kc.LD
CASES = [("fan", 1, 0.0), ("fan", 7, 0.05), ("ops_ico1", 6, 0.0), ("ops_ico1", 63, 0.05)]
MUTATION_CASES = [("fan", 7, 0.05), ("ops_ico1", 63, 0.05)]
# state kinds that must reject each mutation on every case of MUTATION_CASES ("probe": at least one probe)
CAUGHT_BY = {
    "last_interval": ("white", "converged", "probe"), "pair_reads_t1": ("white", "converged", "probe"),
    "odd_corner": ("white", "converged", "probe"), "mu1_sign": ("white", "converged"), "mu0_interval": ("white", "converged", "probe"),
    "ragged_tile": ("white", "converged", "probe"), "neighbour_area": ("white", "converged", "probe"),
    "rmid_last_half": ("white", "converged", "probe"), "cong_prim_scale": ("converged",), "dphi_rounded": ("white", "converged", "probe"),
    "objective_node": ("white", "converged", "probe"), "norm_extra_column": ("white", "converged", "probe"),
}


@pytest.fixture(scope="module")
def geoms():
    return {"fan": sc.geometry("fan"), "ops_ico1": sc.geometry("ops_ico1"), "plane20": kc.plane_geometry(20)}


def numbering(T, geom):
    from dots_socp_amd.geometry import build_plan

    return kc.Numbering.of_plan(build_plan(T, geom, reorder=True))


def states(T, geom, congestion, ks=kc.CONVERGED_K):
    """(kind, name, s, state, params) of one case: white noise, the converged iterates, every probe."""
    s = sc.make_oracle(T, geom, congestion)
    out = [("white", "white", s, kc.white(s, T), kc.params_of(s, geom))]
    for k, (sk, st, p) in zip(ks, kc.converged(T, geom, congestion, ks)):
        out.append(("converged", f"converged{k}", sk, st, p))
    nb = numbering(T, geom)
    for name, support in kc.probe_supports(s, nb).items():
        out.append(("probe", name, s, kc.probe(s, support), kc.probe_params(s, geom)))
    return out, nb


def test_slot_names_follow_the_header():
    from dots_socp_amd import _lib

    names, n_vsums = kc.header_slots()
    assert tuple(names) == kc.SLOTS
    assert n_vsums == 13 and all(n.startswith("V_") for n in names[:13]) and all(n.startswith("F_") for n in names[13:])
    assert kc.N_SUMS == 22 and kc.N_SUMS <= _lib.KKT_N_SUMS
    assert set(kc.NEEDS) == set(kc.SLOTS) and all(0 <= c < 7 for v in kc.NEEDS.values() for c in v)
    assert {c for v in kc.NEEDS.values() for c in v} == set(range(7))


@pytest.mark.parametrize("mesh,T,congestion", CASES)
def test_combine_agrees_with_the_oracle(geoms, mesh, T, congestion):
    """The new reference is tied to OracleSolver.kkt_functions (which the golden vectors tie to the reference solver): 1e-12 on white
    noise; the boundary term and the objective's sums likewise."""
    geom = geoms[mesh]
    s = sc.make_oracle(T, geom, congestion)
    st, p = kc.white(s, 3), kc.params_of(s, geom)
    ref = kc.reference(s, st, p)
    want = kc.oracle_kkt(s, st)
    got = kc.combine(np.asarray(ref["kkt"], dtype=np.float64), s)
    for i in range(7):
        for g, w in zip(got[i], want[i]):
            assert (g is None) == (w is None)
            if w is not None:
                assert abs(g - w) <= 1e-12 * abs(w), (i, g, w)
    assert np.allclose(-p["boundary_scale"] * p["mu0"] / (p["r"] * s.h), s.bnd[0], rtol=1e-15, atol=0.0)
    assert np.allclose(p["boundary_scale"] * p["mu1"] / (p["r"] * s.h), s.bnd[-1], rtol=1e-15, atol=0.0)
    obj = np.asarray(ref["objective"], dtype=np.float64)
    cost, lagr = s.objective()
    mine = p["prim_scale"] * p["dual_scale"] * p["boundary_scale"] * (obj[1] - obj[0])
    assert abs(mine - cost) <= 1e-12 * abs(cost)
    if congestion:
        cong = s.congestion * s.prim_scale / s.dual_scale
        assert abs(mine - p["prim_scale"] ** 2 * obj[2] / T / (2 * cong) - lagr) <= 1e-12 * abs(lagr)
    norms = {k: float(v) for k, v in ref["norms"].items()}
    od = sc.OracleDevice(T, geom, congestion)
    sc.load(od.s, st)
    for (name, part) in kc.NORMS:
        want = od.norm_square(name, part)
        assert abs(norms[(name, part)] - want) <= 1e-12 * want, (name, part)


def test_combine_agrees_with_the_oracle_at_scales_other_than_one(geoms):
    """... and on an iterate after scale_prim_dual (prim, dual and boundary scale differ from 1)."""
    for s, st, p in kc.converged(7, geoms["fan"], 0.05, ks=(10,)):
        assert p["prim_scale"] != 1.0 and p["dual_scale"] != 1.0 and p["boundary_scale"] != 1.0
        got = kc.combine(np.asarray(kc.reference(s, st, p)["kkt"], dtype=np.float64), s)
        want = kc.oracle_kkt(s, st)
        for i in range(7):
            for g, w in zip(got[i], want[i]):
                if w is not None:      # (Dual(beta) is rounding noise here, 5e-16 of its norm sum: an absolute floor for it)
                    assert abs(g - w) <= 1e-10 * abs(w) + 1e-15, (i, g, w)
        assert np.allclose(-p["boundary_scale"] * p["mu0"] / (p["r"] * s.h), s.bnd[0], rtol=4e-16, atol=0.0)


@pytest.mark.parametrize("mesh", ["fan", "ops_ico1", "plane20"])
def test_the_tables_differ_by_the_roundings_the_bound_counts(geoms, mesh):
    """The library's host assembly (device numbering) against the oracle's tables: within TAB_AREA, TAB_AREA + valence + 1 and TAB_HAT
    roundings -- what ``reference`` adds to its counts for every table entry an expression reads."""
    from dots_socp_amd.geometry import build_plan

    geom = geoms[mesh]
    s = sc.make_oracle(3, geom)
    for reorder in (True, "nd"):
        plan = build_plan(3, geom, reorder=reorder)
        pv, pf = plan.perm_vert, plan.perm_tri
        assert np.all(np.abs(plan.area_tri - s.area_f[pf]) <= kc.TAB_AREA * kc.U * s.area_f[pf])
        val = np.bincount(s.tri.reshape(-1), minlength=s.V)
        assert np.all(np.abs(plan.mass_vert - s.mass_v[pv]) <= (kc.TAB_AREA + val[pv] + 1) * kc.U * s.mass_v[pv])
        inv = np.empty_like(pv)
        inv[pv] = np.arange(s.V)
        assert np.array_equal(plan.triangles, inv[s.tri[pf]])      # corners keep their index
        hat = s.hat[pf]
        scale = np.abs(hat).max(axis=2, keepdims=True)
        assert np.all(np.abs(plan.hat_grad - hat) <= kc.TAB_HAT * kc.U * scale)


@pytest.mark.parametrize("mesh,T,congestion", CASES)
def test_conditions_on_the_inputs(geoms, mesh, T, congestion):
    geom = geoms[mesh]
    s = sc.make_oracle(T, geom, congestion)
    st, p = kc.white(s, T), kc.params_of(s, geom)

    def branch(s, st, p):
        """aux + rho > 0 per entry, from the oracle's own arithmetic (kkt_comp_rho_fq)."""
        sc.load(s, st)
        rho = (p["dual_scale"] * p["r"]) * s.mu
        sq = np.sum(np.square(kc.O.decouple(p["prim_scale"] * s.B)), axis=(1, 4)).reshape(-1)
        aux = p["prim_scale"] * s.A + 0.25 * s.c2v_area_T.dot(sq).reshape(s.T, s.V) / s.w_v
        return aux + rho > 0.0

    pos = branch(s, st, p)
    assert 0.1 <= pos.mean() <= 0.9, pos.mean()
    deep = kc.converged(T, geom, congestion)
    q = {n: float(v) for n, v in zip(kc.SLOTS, kc.reference(*deep[-1])["kkt"])}
    # the deepest iterate: residual slot over the matching norm slot below 1e-6 (squares: 1e-12) for conditions 0, 1 and 3
    assert q["V_RESMU2"] <= 1e-12 * q["V_DPHI2"] and q["F_RESE2"] <= 1e-12 * q["F_DX2"]
    assert q["V_RFST2"] + q["V_REND2"] + q["F_RMID2"] <= 1e-12 * (q["V_A2"] + q["F_B2"] + deep[-1][2]["const_d"] ** 2)
    assert q["V_MUAUX1_2"] <= 1e-12 * q["V_MU2"] and q["F_EAUX2_2"] <= 1e-12 * q["F_E2"]
    # ... and only one branch of the fmax there (module docstring): white noise and the probes cover the other
    assert branch(*deep[-1]).mean() > 0.9
    nb = numbering(T, geom)
    sup = kc.probe_supports(s, nb)
    neg = [(kc.probe(s, v)["mu"] < 0).sum() for v in sup.values()]
    assert max(neg) > 0


@pytest.mark.parametrize("mesh,T,congestion", CASES)
def test_plain_is_within_the_tolerance_everywhere(geoms, mesh, T, congestion):
    """The bound is not empty: the straightforward fp64 evaluation passes on every state; what the support of a probe cannot reach is
    exactly zero in both."""
    all_states, _ = states(T, geoms[mesh], congestion)
    for kind, name, s, st, p in all_states:
        ref, pl = kc.reference(s, st, p), kc.plain(s, st, p)
        names, r, tol = kc.tolerances(ref, pl)
        got = np.asarray(kc.flat(pl)[1], dtype=np.float64)
        assert kc.assert_within(got, names, r, tol, f"{mesh} T={T} {name}") <= 1.0 / kc.MARGIN
        assert np.all((r == 0) == (got == 0.0)), name
        if kind == "probe":      # (at T = 1 a time support reaches every slot)
            assert (r != 0).any() and ((r == 0).any() or T == 1), name


def rejected(s, st, p, mutation, nb):
    ref, pl = kc.reference(s, st, p), kc.plain(s, st, p)
    names, r, tol = kc.tolerances(ref, pl)
    got = np.asarray(kc.flat(kc.plain(s, st, p, mutation=mutation, numbering=nb))[1], dtype=np.float64)
    q = kc.ratios(got, r, tol)
    return bool((~(q <= 1.0)).any())


def old_figure_lets_through(s, st, p, mutation, nb):
    """compare_kkt's figure (the seven residuals at KKT_TOL), the objective at 1e-12 and the norms at 1e-13, mutated against plain."""
    a, b = kc.plain(s, st, p), kc.plain(s, st, p, mutation=mutation, numbering=nb)
    ka, kb = kc.combine(a["kkt"], s), kc.combine(b["kkt"], s)
    ok = all(abs(y - x) <= sc.KKT_TOL * abs(x) for u, v in zip(ka, kb) for x, y in zip(u, v) if x is not None)
    oa, ob = (p["prim_scale"] * p["dual_scale"] * p["boundary_scale"] * (o["objective"][1] - o["objective"][0]) for o in (a, b))
    ok = ok and abs(ob - oa) <= 1e-12 * abs(oa)
    return ok and all(abs(b["norms"][k] - a["norms"][k]) <= 1e-13 * a["norms"][k] for k in kc.NORMS)


def test_every_mutation_is_rejected(geoms, record_property):
    assert set(CAUGHT_BY) == set(kc.MUTATIONS) == set(kc.MUTATION_DOC)
    let_through = {}
    for mesh, T, congestion in MUTATION_CASES:
        all_states, nb = states(T, geoms[mesh], congestion, ks=(10, 300))
        for mutation in kc.MUTATIONS:
            caught = {}
            for kind, name, s, st, p in all_states:
                if rejected(s, st, p, mutation, nb):
                    caught.setdefault(kind, []).append(name)
            for kind in CAUGHT_BY[mutation]:
                assert kind in caught, (mesh, T, mutation, kind, caught)
            white = all_states[0]
            let_through[(mesh, T, mutation)] = old_figure_lets_through(white[2], white[3], white[4], mutation, nb)
            print(f"{mesh} T={T} {mutation}: rejected by {sorted(caught)} ({sum(map(len, caught.values()))} states);"
                  f" the existing figure {'lets it through' if let_through[(mesh, T, mutation)] else 'rejects it'}")
    record_property("let_through_by_the_existing_figure", sorted({m for (_, _, m), v in let_through.items() if v}))


# the slot order of fake_device.FakeDeviceProblem._local_kkt_sums (entries 17 and 20, rho^2 and m^2, have no slot of their own)
FAKE_ORDER = ("V_DPHI2", "F_DX2", "V_A2", "F_B2", "V_LAM2", "V_RESMU2", "F_RESE2", "V_RFST2", "V_REND2", "F_RMID2", "V_DUALAUX2", "V_MU2", "F_E2",
              "V_AUX1_2", "F_AUX2_2", "V_MUAUX1_2", "F_EAUX2_2", None, "V_COMP_AUX2", "V_COMP_RES2", None, "F_AUX5_2", "F_AUX5M_2", "V_CONG_RES2")


@pytest.mark.parametrize("partition", [(6, 3), (5, 6), (8, 2), (4, 8)], ids=sl.partition_id)
@pytest.mark.parametrize("mesh", ["fan", "ops_ico1"])
def test_slab_shares_add_up_to_the_whole(geoms, mesh, partition):
    """Per slot: the shares ``reference(..., slab)`` of a partition add up to the whole; the local ranks of fake_device, which form their
    shares from the halos they RECEIVED and in another slot order, agree with their share; halos handed in replace the neighbours' entries."""
    from fake_device import FakeDeviceProblem

    T, n_ranks = partition
    geom = geoms[mesh]
    s = sc.make_oracle(T, geom, 0.05)
    st, p = kc.white(s, 11), kc.params_of(s, geom)
    whole, pl = kc.reference(s, st, p), kc.plain(s, st, p)
    names, r, tol = kc.tolerances(whole, pl)
    group = sl.SlabGroup(T, geom, n_ranks, rank_class=FakeDeviceProblem, buffers=sl.NumpyBuffers(), local=True)
    dev = sl.SlabDevice(group, partition)
    dev.set_params(**sc.device_params(s))
    for k in sc.STATE:
        dev.upload(k, st[k])
    group.each(lambda d: d.slab_stage(4))
    group.neighbours(("send_mu", "recv_mu"), ("send_b", "recv_b"))
    total = np.zeros(len(names), dtype=LD)
    for d in group.devs:
        share = kc.reference(s, st, p, slab=(d.node0, d.nl))
        total += kc.flat(share)[1]
        fake = d.kkt_sums(range(7))
        for j, name in enumerate(FAKE_ORDER):
            if name is not None:
                i = kc.IX[name]
                assert abs(LD(fake[j]) - share["kkt"][i]) <= max(tol[i], LD(0)), (d.rank, name, fake[j], float(share["kkt"][i]))
        if d.nl and d.node0 > 0:      # halos handed in: the same share from a state that does not hold the neighbours' entries
            cut = {k: np.array(v, copy=True) for k, v in st.items()}
            cut["mu"][d.node0 - 1] = np.nan
            halos = dict(mu_lo=st["mu"][d.node0 - 1])
            if d.node0 + d.nl <= T:
                cut["B"][d.node0 + d.nl], cut["phi"][d.node0 + d.nl] = np.nan, np.nan
                halos.update(B_hi=st["B"][d.node0 + d.nl], phi_hi=st["phi"][d.node0 + d.nl])
            with np.errstate(invalid="ignore"):
                again = kc.reference(s, cut, p, slab=(d.node0, d.nl), halos=halos)
            assert np.array_equal(kc.flat(again)[1], kc.flat(share)[1])
    assert np.all(np.abs(total - r) <= 2.0 ** -60 * n_ranks * np.abs(r))

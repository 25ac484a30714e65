"""tests/sequence_checks.py without a GPU: the committed sequences replay clean with the oracle's stand-in on both sides, they reach
every (situation, operation) pair of ``REQUIRED`` within the cap, and ``replay`` catches a numpy imitation of the library's deferrals
(``LazyFake``) as soon as one of them is planted wrong -- so that test_hip_sequences.py cannot pass by checking nothing."""
import numpy as np
import pytest

import sequence_checks as sq
import step_checks as sc

O = sc.O
CASES = (("fan", 7), ("ops_ico1", 6))      # pitch 8 on the odd-valence fan and ragged: the smallest of test_hip_sequences.py's cases
DEFECTS = ("download_skips_division", "carried_survive_upload", "z_mid_from_new_beta_mid", "readout_mu_undivided", "ahead_survives_set_params",
           "cold_restart_keeps_division", "fused_survive_q_lambda")


class LazyFake(sc.OracleDevice):
    """The deferrals of dots_api.hip imitated in numpy on the stand-in, each one switchable to a planted defect (``DEFECTS``):

    * a penalty division is left pending (the five dual arrays stay undivided) until something reads or writes them; the first step
      after a restart does not look for one (a restart drops it: this shortcut is what gives a division that a cold restart KEEPS
      something to divide -- applied at once it would meet arrays that are zero, and nothing could tell);
    * a ``carry`` step keeps copies of B, E and beta_mid, and the next step forms its right-hand side and the cone norms from the
      copies; a ``kkt_sums`` step keeps the residuals 0-3 and 6, and a read within them returns what was kept;
    * after a ``carry`` or ``kkt_sums`` step z_mid is not stored: it is rebuilt on demand from the OLD B and beta_mid;
    * the first KKT read after an ``rhs_ahead`` step forms the next right-hand side, which the next step takes.

    Every call that changes the state or the parameters drops what was carried, kept or formed ahead."""

    def __init__(self, T, geom, congestion, defects=()):
        super().__init__(T, geom, congestion, strict=False)
        assert set(defects) <= set(DEFECTS), defects
        self.defects = set(defects)
        self.pending = self.carried = self.fused = self.deferred = self.ahead = None
        self.carry = self.ksum = self.want_ahead = self.ahead_armed = self.fresh = False

    # ---- the deferred work
    def _flush(self, skip=()):
        if self.pending is not None:
            f, self.pending = self.pending, None
            for k in sc.DUAL:
                if k not in skip:
                    setattr(self.s, k, getattr(self.s, k) / f)

    def _materialise(self):
        if self.deferred is not None:
            s = self.s
            (B_old, bm_old, lam, sz), self.deferred = self.deferred, None
            if "z_mid_from_new_beta_mid" in self.defects:
                bm_old = s.beta_mid
            lam_corner = s.v2c_T.dot(lam.reshape(-1)).reshape(s.T, 3, s.F) / s.D[None]
            s.z_mid = lam_corner[:, None, :, :, None] * (s.D[None, None, :, :, None] * (O.decouple(B_old, sz) - bm_old))

    def _changed(self, keep=()):
        for k in ("carried", "fused", "ahead"):
            if k not in keep:
                setattr(self, k, None)
        self.ahead_armed = False

    def _rhs(self):
        s = self.s
        B, E = (self.carried[0], self.carried[1]) if self.carried is not None else (s.B, s.E)
        return O.div_time(s.h, (s.A + s.lambda_c - s.mu) * s.w_v) + O.div_space(s.Dv, (B - E) * s.w_f) - s.bnd - s.eps * s.w_v * s.phi

    # ---- the calls
    def step_flags(self, palm=False, skip_z_mid=False, rhs_ahead=False, carry=False, kkt_sums=False, timed=False):
        super().step_flags(palm=palm, skip_z_mid=skip_z_mid, rhs_ahead=rhs_ahead)
        self.carry, self.ksum, self.want_ahead = carry and not palm, kkt_sums and not skip_z_mid, rhs_ahead

    def step(self, n=1, wait=True):
        s = self.s
        for _ in range(n):
            if self.palm and self.stale:
                raise sc.refused(-5, "dots_step")
            if not self.fresh:
                self._flush()
            self.fresh = False
            if self.palm:
                self._materialise()
                sc.palm_step0(s)
                self._changed()
            self.deferred = None      # (nobody asked for the last z_mid)
            s.phi[:] = s.lap_inv(self.ahead if self.ahead is not None else self._rhs())
            # the oracle's projection, the norms gathered from what was carried
            B_g, bm_g = (self.carried[0], self.carried[2]) if self.carried is not None else (s.B, s.beta_mid)
            w_fst = s.d - s.sz * s.A - s.beta_fst
            w_mid = s.D[None, None, :, :, None] * (O.decouple(s.B, s.sz) - s.beta_mid)
            w_end = s.d + s.sz * s.A - s.beta_end
            per_corner = ((s.D[None, None, :, :, None] * (O.decouple(B_g, s.sz) - bm_g)) ** 2).sum(axis=(1, 4))
            nrm = np.sqrt(s.c2v_one_T.dot(per_corner.reshape(-1)).reshape(s.T, s.V) + w_end ** 2)
            with np.errstate(divide="ignore", invalid="ignore"):
                lam = np.clip(0.5 * (1.0 + w_fst / nrm), 0.0, 1.0)
            lam_corner = s.v2c_T.dot(lam.reshape(-1)).reshape(s.T, 3, s.F) / s.D[None]
            s.z_fst[:] = np.where(lam >= 1.0, w_fst, lam * nrm)
            s.z_mid[:] = lam_corner[:, None, :, :, None] * w_mid
            s.z_end[:] = lam * w_end
            old = (s.B.copy(), s.beta_mid.copy(), lam, s.sz)
            s.step_q_lambda()
            s.step_multipliers()
            self._changed()
            self.stale = self.skip
            if self.carry:
                self.carried = (s.B.copy(), s.E.copy(), s.beta_mid.copy())
            if self.ksum:
                self.fused = sc.OracleDevice.kkt(self, sorted(sq.FUSED))
            if self.skip or ((self.carry or self.ksum) and not self.palm):
                s.z_mid = np.full_like(s.z_mid, np.nan)      # not stored
                if not self.skip:
                    self.deferred = old
            self.ahead_armed = self.want_ahead and not self.palm

    def kkt(self, conditions):
        conditions = list(conditions)
        if 1 in conditions and self.stale:
            raise sc.refused(-5, "dots_kkt")
        self._flush()
        if self.fused is not None and set(conditions) <= sq.FUSED:
            out = {i: list(self.fused[i]) for i in conditions}
        else:
            if 1 in conditions:
                self._materialise()
            out = super().kkt(conditions)
        if self.ahead_armed:
            self.ahead_armed, self.ahead = False, self._rhs()
        return out

    def download(self, name):
        if name == "z_mid" and self.stale:
            raise sc.refused(-5, "download z_mid")
        if not (name == "beta_mid" and "download_skips_division" in self.defects):
            self._flush()
        if name == "z_mid":
            self._materialise()
        return super().download(name)

    def download_all(self):
        if self.stale:
            raise sc.refused(-5, "download z_mid")
        self._flush()
        self._materialise()
        return super().download_all()

    def upload(self, name, a):
        self._flush()
        if name != "z_mid":
            self._materialise()
        self.deferred = None
        super().upload(name, a)
        self._changed(keep=("carried",) if name == "beta_mid" and "carried_survive_upload" in self.defects else ())

    def set_params(self, **kw):
        super().set_params(**kw)
        self._changed(keep=("ahead",) if set(kw) == {"r"} and "ahead_survives_set_params" in self.defects else ())

    def adjust_penalty(self, f):
        self._flush()
        self.s.r *= f
        self.s.bnd /= f
        self.pending, self.fresh = f, False
        self._changed()

    def _then_changed(self, call, *a, keep=()):
        self._flush()
        self._materialise()
        try:
            return call(*a)
        finally:
            self._changed(keep=keep)

    def scale_z(self, *a):
        self._then_changed(super().scale_z, *a)

    def scale_arrays(self, *a):
        self._then_changed(super().scale_arrays, *a)

    def run_phase(self, phase):
        self._then_changed(super().run_phase, phase, keep=("fused",) if phase == "q_lambda" and "fused_survive_q_lambda" in self.defects else ())

    def restart(self, mu0, mu1, mode="cold", factors=None):
        if mode == "warm":
            if self.stale:
                raise sc.refused(-5, "dots_restart")
            self._flush()
            self._materialise()
        elif "cold_restart_keeps_division" not in self.defects:
            self.pending = None
        self.deferred = None
        super().restart(mu0, mu1, mode, factors)
        self._changed()
        self.carry = self.ksum = self.want_ahead = False
        self.fresh = True

    def objective(self):
        self._flush()
        return super().objective()

    def norm_square(self, name, part=0):
        self._flush()
        if name == "z_mid" and not self.stale:
            self._materialise()
        self._changed()      # (the library treats it as a call that changes the state)
        return super().norm_square(name, part)

    def apply_operator(self, *a):
        self._flush()
        self._changed()
        return super().apply_operator(*a)

    def readout(self, *a):
        self._flush(skip=("mu",) if "readout_mu_undivided" in self.defects else ())
        return super().readout(*a)

    def sensitivity(self, *a, **kw):
        self._flush()
        return super().sensitivity(*a, **kw)

    def flow_trace(self, *a, **kw):
        self._flush()
        return super().flow_trace(*a, **kw)


@pytest.fixture(scope="module")
def geoms():
    return {m: sc.geometry(m) for m, _ in CASES}


def run(seq, seed, geom, T, lazy_of, report=None):
    c = sq.congestion_of(seed)
    lazy, eager, oracle = lazy_of(T, geom, c), sc.OracleDevice(T, geom, c, strict=False), sc.make_oracle(T, geom, c)
    sq.start((lazy, eager), oracle, geom, seed)
    sq.replay(seq, lazy, eager, oracle, report=report)


def fails(seed, geom, T, lazy_of):
    def predicate(seq):
        try:
            run(seq, seed, geom, T, lazy_of)
        except AssertionError:
            return True
        return False
    return predicate


def test_the_table_is_full_within_the_cap():
    assert sq.LENGTH <= 16 and len(sq.SEEDS) <= 32
    seqs = [sq.make_sequence(seed, sq.LENGTH) for seed in sq.SEEDS]
    assert all(len(s) <= sq.LENGTH and sq.legal(s) for s in seqs)
    missing = sq.REQUIRED - sq.coverage(seqs)
    assert not missing, sorted(missing)
    # every reader and every state-changing call under each single situation, and the combinations the issue names
    for sit in sq.SINGLE:
        for kind in sq.READERS + sq.CHANGERS:
            if sit == sq.SKIP and kind in sq.ONLY_REFUSED:      # while z_mid is unspecified these can only be refused
                assert (sit, "refuse_" + kind) in sq.REQUIRED
            else:
                assert (sit, kind) in sq.REQUIRED
    assert {k for s, k in sq.REQUIRED if s == sq.MULTI} >= {"readout", "sensitivity", "flow_map", "restart_warm", "restart_cold", "download_z_mid",
                                                            "kkt_all", "confirm", "drop"}
    # the seed count: at most one sequence more than the operations of the episodes that fill the table need at this length
    assert len(sq.SEEDS) <= -(-sum(len(s) for s in seqs) // sq.LENGTH) + 1
    # the sequences are plain data, the same on every call, and name every operation, flag and refusal of the issue
    assert seqs == [sq.make_sequence(seed, sq.LENGTH) for seed in sq.SEEDS]
    flat = [op for s in seqs for op in s]
    assert {f for n, a in flat if n == "step" for f in a["flags"]} == set(sq.FLAGS)
    assert {tuple(a["mask"]) for n, a in flat if n == "kkt"} >= set(sq.MASKS)
    assert {(a["name"], a["part"]) for n, a in flat if n == "norm_square"} == set(sq.NORMS)
    assert {a["name"] for n, a in flat if n == "download"} == set(sc.STATE)
    assert {a["phase"] for n, a in flat if n == "run_phase"} == set(sq.PHASES)
    assert {a["what"] for n, a in flat if n == "refuse"} == set(sq.REFUSALS)
    assert {a["centred"] for n, a in flat if n == "readout"} == {False, True} and {a["wait"] for n, a in flat if n == "step"} == {False, True}
    assert {a["op"] for n, a in flat if n == "apply_operator"} == set(sq.OPERATORS)
    assert any(x[0] == y[0] == "adjust_penalty" for s in seqs for x, y in zip(s, s[1:]))      # two penalty updates in a row
    steps = sum(n == "step" for n, _ in flat)
    assert 0.3 * len(flat) <= steps <= 0.6 * len(flat), (steps, len(flat))
    # beyond the planned sequences the generator goes on at random, within the rules
    extra = sq.make_sequence(1000, 12)
    assert len(extra) == 12 and sq.legal(extra) and extra == sq.make_sequence(1000, 12)


def test_situations_are_told_from_the_sequence():
    seq = [sq.step("carry", "kkt_sums", "rhs_ahead"), ("kkt", {"mask": [0, 2, 3]}), ("objective", {}), ("penalty_ahead", {}),
           ("kkt", {"mask": [0, 1, 2, 3]}), ("adjust_penalty", {"f": 1.7, "how": "confirm"}), ("set_r", {"f": 1.4}), ("readout", {}),
           sq.step("skip_z_mid"), ("adjust_penalty", {"f": 1.7, "how": "given"}), ("download", {"name": "mu"}), ("download", {"name": "mu"})]
    got = [sorted(s - {sq.MULTI}) for s in sq.situations(seq)]
    assert got == [[], ["carry", "kkt_sums"], ["ahead"], ["ahead"], ["ahead"], ["ahead", "armed"], ["div"], ["div"], [], ["skip"], ["div", "skip"], ["skip"]]
    assert [sq.MULTI in s for s in sq.situations(seq)] == [len(g) >= 2 for g in got]
    assert not sq.legal([sq.step("skip_z_mid"), ("kkt", {"mask": [1]})]) and sq.legal([sq.step("skip_z_mid"), ("refuse", {"what": "kkt_1"})])
    assert not sq.legal([("refuse", {"what": "kkt_1"})]) and sq.legal([("refuse", {"what": "flags_palm_skip"})])
    # SKIP lasts while z_mid is unspecified and no longer; norm_square and apply_operator end AHEAD, ARMED and the fused reads
    seq = [sq.step("skip_z_mid", "rhs_ahead"), ("kkt", {"mask": [0]}), ("objective", {}), ("norm_square", {"name": "mu", "part": 0}),
           ("objective", {}), ("upload", {"name": "z_mid"}), ("objective", {})]
    assert [sorted(s - {sq.MULTI}) for s in sq.situations(seq)] == [[], ["skip"], ["ahead", "skip"], ["ahead", "skip"], ["skip"], ["skip"], []]
    seq = [sq.step("kkt_sums"), ("objective", {}), ("kkt", {"mask": [0]}), ("apply_operator", {"op": "decouple"}), ("kkt", {"mask": [0]})]
    assert sq.fused_reads(seq) == [False, False, True, False, False]
    seq = [("scale_z", {"f": 0.8}), ("kkt", {"mask": [3]}), ("adjust_penalty", {"f": 1.3, "how": "given"}), ("kkt", {"mask": [0, 3]}),
           ("kkt", {"mask": [0]}), sq.step(), ("kkt", {"mask": [3]})]
    assert sq.cancelling_reads(seq) == [False, True, False, True, False, False, True]
    assert sq.cancelling_reads([("restart", {"mode": "cold"}), sq.step(), ("kkt", {"mask": [3]}), ("upload", {"name": "mu"}), ("kkt", {"mask": [3]})]) \
        == [False, False, True, False, False]
    assert sq.stale_at_end([sq.step("skip_z_mid"), ("objective", {})]) and not sq.stale_at_end([sq.step("skip_z_mid"), ("upload", {"name": "z_mid"})])


@pytest.mark.parametrize("mesh,T", CASES)
def test_committed_seeds_replay_clean_on_the_oracle(geoms, mesh, T):
    """Self-consistency: the stand-in plays both contexts; the model, the bookkeeping of ``replay`` and every bound hold."""
    for seed in sq.SEEDS:
        run(sq.make_sequence(seed), seed, geoms[mesh], T, lambda *a: sc.OracleDevice(*a, strict=False))
    for name, (seed, seq) in sq.REGRESSIONS.items():
        run(seq, seed, geoms[mesh], T, lambda *a: sc.OracleDevice(*a, strict=False))


def test_the_imitation_replays_clean(geoms):
    mesh, T = CASES[0]
    for seed in sq.SEEDS:
        run(sq.make_sequence(seed), seed, geoms[mesh], T, LazyFake)


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_is_caught_and_shrunk(geoms, defect):
    mesh, T = CASES[0]
    lazy_of = lambda *a: LazyFake(*a, defects=(defect,))      # noqa: E731
    caught = [seed for seed in sq.SEEDS if fails(seed, geoms[mesh], T, lazy_of)(sq.make_sequence(seed))]
    assert caught, defect
    seed = caught[0]
    pred = fails(seed, geoms[mesh], T, lazy_of)
    small = sq.shrink(sq.make_sequence(seed), pred)
    print(f"{defect}: caught by seeds {caught}; seed {seed} shrinks to {len(small)} operations:")
    for op in small:
        print("   ", op)
    assert pred(small) and len(small) <= 6
    for i in range(len(small)):      # minimal: no single operation can go
        cand = small[:i] + small[i + 1:]
        assert not (sq.legal(cand) and pred(cand)), (defect, i)
    assert not fails(seed, geoms[mesh], T, LazyFake)(small)      # the same sequence passes with every switch off

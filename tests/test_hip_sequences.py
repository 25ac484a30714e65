"""GPU: the bookkeeping of dots_api.hip under call sequences (tests/sequence_checks.py).

Every entry point decides what of a context's deferred work -- a pending penalty division, carried gathers, fused KKT sums, an
unspecified or deferred z_mid, a right-hand side ahead, an armed penalty decision -- it flushes, keeps or drops, and the header promises
that results never depend on it.  The committed sequences (``sequence_checks.SEEDS``; test_sequence_checks_cpu.py shows that they put
every reader and every state-changing call into every one of these situations) are replayed on a context with the library's defaults
and the hints the sequence names (``lazy``), on a context created under DOTS_LAZY_DIV=0 and DOTS_ZMID_DEFER=0 that gets no hint at all
(``eager``), and on the fp64 oracle:

* everything a sequence reads comes out of ``lazy`` and ``eager`` with the same bits (KKT values equal; within 1e-12 where the read
  may take the sums a kkt_sums step left), and so do the twelve arrays at its end;
* ``eager`` follows the oracle operation by operation: steps as test_hip_step_variants.py checks them (phi 1e-9, every other entry
  1e-12), the residuals within 1e-11, objective and norms within the bounds of test_kkt_objective_norms_a10_a11_a12, the outputs of
  dots_readout, dots_sensitivity and the tracer equal to their host specifications bit for bit;
* the refusals the header documents come with their status, and the sequence goes on from an untouched state.

One test per (mesh, T) -- pitch 8 ragged, pitch 8 full on the odd-valence fan, pitch 32, pitch 128 on the matrix cores -- loops over the
seeds on one pair of contexts and then asserts, on the step paths ``lazy`` recorded (dots_debug_counter 12) and on counters 2 and 3,
that the hints were taken: a sequence whose flags were silently ignored would compare an eager context with itself.

Every tolerance is one of step_checks.py, or the cited tests' own, with two remarks:

* a read between a kkt_sums step and the next call that changes the state may take the fused sums also when another read came first
  (the header keeps them over reads): ``sequence_checks.fused_reads`` gives such a read the 1e-12 as well;
* Dual(beta) read after scale_z, which SETS mu and E to what makes it vanish (``sequence_checks.cancelling_reads``; the iteration keeps it so from
  there on, and from the zero state of a cold restart), is rounding alone: 1.6e-16 on the device against 1.6e-16 in the oracle, a
  relative 9e-3 apart, and no relative bound holds for it.  That one condition
  of those reads gets, on top of step_checks.KKT_TOL * |want|, mode_checks.MARGIN times a figure measured on the oracle side for the
  very state: what the oracle's own closure moves by when its terms are added and scaled in another order
  (``sequence_checks.dual_beta_reordered``).  Every other read goes through step_checks.compare_kkt as it stands.
  MEASURED on an MI355X over the four cases (28 such reads, two values each): device against oracle 8.0e-20 to 2.9e-17 apart, the
  oracle-side figure 2.9e-18 to 4.4e-17, the largest share of the bound taken 0.13.

The committed sequences are constructed, not sampled (sequence_checks.make_sequence).  MEASURED on an MI355X: the 25 of them (391
operations) take 0.4 to 1.6 s per (mesh, T).  No defect found in the library; ``REGRESSIONS`` is empty."""
import pytest

import sequence_checks as sq
import step_checks as sc
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

CASES = (("ops_ico1", 6), ("fan", 7), ("ops_refplane4", 31), ("ops_ico1", 64))
EAGER_ENV = {"DOTS_LAZY_DIV": "0", "DOTS_ZMID_DEFER": "0"}      # both read by dots_create


def contexts(T, geom, monkeypatch):
    from dots_socp_amd.device import DeviceProblem

    out = []
    try:
        for env in ({}, EAGER_ENV):
            for k in EAGER_ENV:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            out.append(DeviceProblem(T, geom, lap_solver="modal_pcg"))
            assert out[-1].setup_frontal(leaf=4)["levels"] >= 1
    except BaseException:
        for dev in out:
            dev.close()
        raise
    finally:
        for k in EAGER_ENV:
            monkeypatch.delenv(k, raising=False)
    return out


def report_failure(seq, seed, T, geom, monkeypatch, err):
    """The seed and the sequence, then what is left of it after shrinking on fresh contexts (a failing assertion is not a fault)."""
    print(f"seed {seed} fails: {err}")
    for op in seq:
        print("   ", op)

    def make_players():
        lazy, eager = contexts(T, geom, monkeypatch)
        return lazy, eager, sc.make_oracle(T, geom, sq.congestion_of(seed)), geom, seed, lambda: (lazy.close(), eager.close())

    small = sq.shrink(seq, sq.fails_on(make_players))
    print(f"shrunk to {len(small)} operations:")
    for op in small:
        print("   ", op)


@pytest.mark.parametrize("mesh,T", CASES)
def test_sequences_against_the_oracle_and_the_eager_twin(mesh, T, monkeypatch):
    from dots_socp_amd import _lib

    geom = sc.geometry(mesh)
    lazy, eager = contexts(T, geom, monkeypatch)
    paths = []
    try:
        runs = [(seed, sq.make_sequence(seed)) for seed in sq.SEEDS] + [tuple(v) for v in sq.REGRESSIONS.values()]
        for seed, seq in runs:
            oracle = sc.make_oracle(T, geom, sq.congestion_of(seed))
            sq.start((lazy, eager), oracle, geom, seed)
            try:
                sq.replay(seq, lazy, eager, oracle, on_step=lambda dev: paths.append(dev.debug_counter(_lib.STEP_PATH_COUNTER)))
            except AssertionError as err:      # (a difference, or a status on a legal call: never an error of the runtime itself)
                lazy.close()
                eager.close()
                report_failure(seq, seed, T, geom, monkeypatch, err)
                raise
        started, confirmed = lazy.debug_counter(2), lazy.debug_counter(3)
    finally:
        lazy.close()
        eager.close()
    # the hints were taken: every deferral occurred on `lazy` (the bit names of test_hip_step_variants.expect)
    P, union = _lib.STEP_PATH, 0
    for p in paths:
        union |= p
    taken = {"carried": union & P["rhs_carried"], "div": union & P["rhs_div"], "ql_div": union & P["ql_div"], "defer": union & P["ql_defer"],
             "kkt": union & P["ql_kkt"], "rider": union & P["soc_rider"], "Z = 2": any((p >> _lib.STEP_PATH_QL_Z_SHIFT) & 3 == 2 for p in paths)}
    assert all(taken.values()), {k: bool(v) for k, v in taken.items()}
    assert started > 0 and confirmed > 0, (started, confirmed)      # penalty decisions started ahead of the host, and confirmed

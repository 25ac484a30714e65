"""The kernel variants of the direct solver's iteration against the fp64 oracle, one step at a time, on planted states.

``dots_step`` picks its right-hand-side / projection launch (k_rhs_modes2 / k_rhs_modes_mfma <CARRIED, DIV>, the projection riding along or
alone) and its steps-2+3 launch (k_q_lambda_mult_triangle2<Z>, k_q_lambda_mult_carry<Z, K, DIV, BMNT>) from the step flags, a pending penalty
division and what the last step left.  Every scenario of tests/step_checks.py sets one such combination up, asserts on the launcher's
record (dots_debug_counter 12) that the intended kernels ran -- a launcher that falls back to another variant fails here -- and compares
the state after the step with the oracle entry by entry (step_checks.check_one_step: phi within 1e-9, everything else within 1e-12, NaN
where and only where the reference has NaN).  The states take every branch of the cone projection, sit exactly on both of its boundaries and
hold a zero pre-image (step_checks.edge_state); the meshes have valences 1 to 9, the time pitches run from 8 to 128."""
import pytest

import step_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geoms():
    return {m: sc.geometry(m) for m in sc.MESHES}


def expect_launches(T):
    from dots_socp_amd import _lib

    P = _lib.STEP_PATH

    def expect(dev, carried=False, div=False, rider=True, ql="ql_triangle2", z=1, kkt=False, ql_div=False, defer=False):
        want = P["rhs_mfma"] if T + 1 >= 64 else P["rhs_modes2"]      # pitch 64 and 128: the transform on the matrix cores
        want |= (P["rhs_carried"] if carried else 0) | (P["rhs_div"] if div else 0) | (P["soc_rider"] if rider else P["soc_alone"])
        want |= P[ql] | (z << _lib.STEP_PATH_QL_Z_SHIFT) | (P["ql_kkt"] if kkt else 0) | (P["ql_div"] if ql_div else 0) | (P["ql_defer"] if defer else 0)
        got = dev.debug_counter(_lib.STEP_PATH_COUNTER)
        if ql == "ql_carry":      # BMNT follows the rule of dots_front_setup (dots_debug_counter 6), whatever it decided here
            assert bool(got & P["ql_bmnt"]) == bool(dev.debug_counter(6))
        assert got & ~P["ql_bmnt"] == want, (hex(got), hex(want))

    return expect


@pytest.mark.parametrize("name,mesh,T,congestion", sc.cases())
def test_step_variant_against_oracle(geoms, name, mesh, T, congestion):
    from dots_socp_amd import _lib
    from dots_socp_amd.device import DeviceProblem

    s = sc.make_oracle(T, geoms[mesh], congestion)
    with DeviceProblem(T, geoms[mesh], lap_solver="modal_pcg") as dev:
        assert dev.setup_frontal(leaf=4)["levels"] >= 1
        dev.set_params(**sc.device_params(s))
        assert dev.debug_counter(_lib.STEP_PATH_COUNTER) == 0      # nothing enqueued yet
        sc.scenario(name)(dev, s, T, seed=T, expect=expect_launches(T))
        dev.upload("mu", dev.download("mu"))                        # a change of state ends the record
        assert dev.debug_counter(_lib.STEP_PATH_COUNTER) == 0


def test_step_path_without_the_direct_solver(geoms):
    """The record names the other launchers' choices too: a PCG context takes k_rhs and the stand-alone projection."""
    from dots_socp_amd import _lib
    from dots_socp_amd.device import DeviceProblem

    P = _lib.STEP_PATH
    with DeviceProblem(6, geoms["ops_ico1"], lap_solver="modal_pcg") as dev:
        dev.set_params(cg_tol=1e-10)
        dev.step(1)
        assert dev.debug_counter(_lib.STEP_PATH_COUNTER) == P["rhs"] | P["soc_alone"] | P["ql_triangle2"] | (1 << _lib.STEP_PATH_QL_Z_SHIFT)
        dev.run_phase("q_lambda_mult")                              # a single phase: its own launch only
        assert dev.debug_counter(_lib.STEP_PATH_COUNTER) == P["ql_triangle2"]

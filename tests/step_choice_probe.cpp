// Runs rhs_choice and ql_choice of csrc/step_choice.h over every combination of their facts: one line per combination
// (tests/test_step_choice_cpu.py compiles, runs and checks it).  A stand-alone host program: the header knows nothing of HIP.
#include <cstdio>

#include "../dots_socp_amd/csrc/step_choice.h"

using namespace dots;

int main() {
    printf("bits rhs=%d rhs_modes=%d rhs_modes2=%d rhs_mfma=%d rhs_carried=%d rhs_div=%d soc_rider=%d soc_alone=%d ql_triangle=%d ql_triangle2=%d ql_carry=%d "
           "ql_z_shift=%d ql_kkt=%d ql_div=%d ql_bmnt=%d ql_defer=%d deep_rhs=%d deep_inverse=%d\n",
           STEP_PATH_RHS, STEP_PATH_RHS_MODES, STEP_PATH_RHS_MODES2, STEP_PATH_RHS_MFMA, STEP_PATH_RHS_CARRIED, STEP_PATH_RHS_DIV, STEP_PATH_SOC_RIDER,
           STEP_PATH_SOC_ALONE, STEP_PATH_QL_TRIANGLE, STEP_PATH_QL_TRIANGLE2, STEP_PATH_QL_CARRY, STEP_PATH_QL_Z_SHIFT, STEP_PATH_QL_KKT, STEP_PATH_QL_DIV,
           STEP_PATH_QL_BMNT, STEP_PATH_QL_DEFER, DEEP_PATH_RHS, DEEP_PATH_INVERSE);
    const char *const rhs_kernel[] = {"mfma", "modes2_deep", "modes2", "modes", "plain"};
    const char *const rhs_variant[] = {"carried", "dividing", "neither"};
    // facts in the order of RhsFacts: writes_modes, mfma_ok, tp4, carried, deep_wins, with_soc, pending
    for (int m = 0; m < 1 << 7; ++m) {
        const auto bit = [m](int i) { return ((m >> (6 - i)) & 1) != 0; };
        const RhsFacts f{bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6)};
        const RhsChoice o = rhs_choice(f);
        printf("rhs %d%d%d%d%d%d%d %s %s path=%d deep=%d divides=%d refused=%d\n", f.writes_modes, f.mfma_ok, f.tp4, f.carried, f.deep_wins, f.with_soc, f.pending,
               rhs_kernel[o.kernel], rhs_variant[o.variant], o.path, o.deep, (int)o.divides, (int)o.refused);
    }
    const char *const ql_kernel[] = {"carry", "triangle2", "triangle"};
    // facts in the order of QlFacts, zmid_mode as its digit: carry_possible, step_carry, step_kkt, zmid_mode, fused_present, fused_fit, slab, step_palm,
    // can_defer, tp4, bm_nt, pending
    for (int m = 0; m < 1 << 11; ++m)
        for (int z = 0; z < 3; ++z) {
            const auto bit = [m](int i) { return ((m >> (10 - i)) & 1) != 0; };
            const QlFacts f{bit(0), bit(1), bit(2), z, bit(3), bit(4), bit(5), bit(6), bit(7), bit(8), bit(9), bit(10)};
            const QlChoice o = ql_choice(f);
            printf("ql %d%d%d%d%d%d%d%d%d%d%d%d %s Z=%d emit=%d defer=%d path=%d divides=%d refused=%d\n", f.carry_possible, f.step_carry, f.step_kkt, f.zmid_mode,
                   f.fused_present, f.fused_fit, f.slab, f.step_palm, f.can_defer, f.tp4, f.bm_nt, f.pending, ql_kernel[o.kernel], o.Z, o.emit, (int)o.defer, o.path,
                   (int)o.divides, (int)o.refused);
        }
    return 0;
}

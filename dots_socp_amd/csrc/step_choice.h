// Which kernel a step launch takes, decided once: launch_rhs and launch_q_lambda_mult (kernels_alm.hip) collect the facts, call the
// function and execute what it returns; rhs_divides and ql_divides collect the same facts and read `divides`.  Host code that knows
// nothing of HIP and takes no context, so that a stand-alone program can run every combination of the facts (tests/step_choice_probe.cpp).
#pragma once

namespace dots {

// Launches the last iteration took (Carried::step_path, dots_debug_counter 12), recorded where launch_rhs, launch_soc_projection and
// launch_q_lambda_mult choose: a test of one kernel variant asserts that the step ran it.  Host bookkeeping only.
enum {
    STEP_PATH_RHS = 1,              // k_rhs
    STEP_PATH_RHS_MODES = 2,        // k_rhs_modes
    STEP_PATH_RHS_MODES2 = 4,       // k_rhs_modes2
    STEP_PATH_RHS_MFMA = 8,         // k_rhs_modes_mfma
    STEP_PATH_RHS_CARRIED = 16,     // ... its CARRIED argument
    STEP_PATH_RHS_DIV = 32,         // ... its DIV argument
    STEP_PATH_SOC_RIDER = 64,       // the cone projection rode in the right-hand-side launch
    STEP_PATH_SOC_ALONE = 128,      // ... or ran as k_soc_projection
    STEP_PATH_QL_TRIANGLE = 256,    // k_q_lambda_mult_triangle
    STEP_PATH_QL_TRIANGLE2 = 512,   // k_q_lambda_mult_triangle2
    STEP_PATH_QL_CARRY = 1024,      // k_q_lambda_mult_carry
    STEP_PATH_QL_Z_SHIFT = 11,      // the Z mode of steps 2+3 (0 read z_mid, 1 rebuild and store, 2 rebuild only), bits 11-12
    STEP_PATH_QL_KKT = 1 << 13,     // K: the fused KKT sums
    STEP_PATH_QL_DIV = 1 << 14,     // DIV: a pending penalty division applied
    STEP_PATH_QL_BMNT = 1 << 15,    // BMNT: beta_mid streamed around the caches
    STEP_PATH_QL_DEFER = 1 << 16,   // z_mid deferred (Carried::zmid)
    STEP_PATH_RHS_MASK = 0xff, STEP_PATH_QL_MASK = 0x1ff00,
    // Carried::deep_path, dots_debug_counter 15: which form of the launches around the direct solve ran last
    DEEP_PATH_RHS = 1,              // k_rhs_modes2_deep took the right-hand side (and the projection riders)
    DEEP_PATH_INVERSE = 2           // k_time_modes_tile_fast took the inverse time transform
};

// ---- the right-hand side of step 1 (with or without the riding cone projection) ----
enum RhsKernel : int { RHS_MFMA = 0, RHS_MODES2_DEEP, RHS_MODES2, RHS_MODES, RHS_PLAIN };      // k_rhs_modes_mfma, k_rhs_modes2_deep, k_rhs_modes2, k_rhs_modes, k_rhs
// the mode kernels' variants: CARRIED (the corners' shares come from the last steps-2+3 launch), DIVIDING (a penalty update is pending: the dual
// arrays are divided as they are read), or neither.  The values are the launch's template ladder.
enum RhsVariant : int { RHS_CARRIED = 0, RHS_DIVIDING = 1, RHS_NEITHER = 2 };
struct RhsFacts {
    bool writes_modes;      // rhs_writes_modes: the direct solver on one GPU
    bool mfma_ok;           // time_modes_mfma_ok: T + 1 >= 64
    bool tp4;               // pitch >= 4: two time columns per lane
    bool carried;           // Carried::carry_valid
    bool deep_wins;         // deep_launch_wins for this launch's grid
    bool with_soc;          // the cone projection rides in the launch
    bool pending;           // a penalty division is to be applied as the launch reads
};
struct RhsChoice {
    RhsKernel kernel;
    RhsVariant variant;
    int path, deep;         // STEP_PATH_*, DEEP_PATH_*
    bool divides;           // the launch (kernel and variant) has a dividing instantiation
    bool refused;           // a division is pending and the launch cannot apply it: nothing may be launched
};
inline RhsChoice rhs_choice(const RhsFacts &f) {
    RhsChoice o{};
    o.kernel = !f.writes_modes ? RHS_PLAIN
             : f.mfma_ok ? RHS_MFMA
             : (f.carried && f.deep_wins) ? RHS_MODES2_DEEP      // the carried walks with every row in flight (pitch 8, 16, 32)
             : f.tp4 ? RHS_MODES2 : RHS_MODES;
    const bool takes_carried = o.kernel != RHS_MODES && f.carried;
    o.divides = (o.kernel == RHS_MFMA || o.kernel == RHS_MODES2) && !f.carried;
    o.refused = f.pending && !o.divides;
    o.variant = takes_carried ? RHS_CARRIED : (f.pending && o.divides) ? RHS_DIVIDING : RHS_NEITHER;
    const int kernel_bit[] = {STEP_PATH_RHS_MFMA, STEP_PATH_RHS_MODES2, STEP_PATH_RHS_MODES2, STEP_PATH_RHS_MODES, STEP_PATH_RHS};
    o.path = kernel_bit[o.kernel] | (o.variant == RHS_CARRIED ? STEP_PATH_RHS_CARRIED : 0) | (o.variant == RHS_DIVIDING ? STEP_PATH_RHS_DIV : 0) |
             (f.with_soc ? STEP_PATH_SOC_RIDER : 0);
    o.deep = o.kernel == RHS_MODES2_DEEP ? DEEP_PATH_RHS : 0;
    return o;
}

// ---- steps 2+3 ----
enum QlKernel : int { QL_CARRY = 0, QL_TRIANGLE2, QL_TRIANGLE };      // k_q_lambda_mult_carry, k_q_lambda_mult_triangle2, k_q_lambda_mult_triangle
struct QlFacts {
    bool carry_possible;    // carry_possible: the direct solver's iteration with the gathers allocated, pitch 4 .. 128
    bool step_carry;        // DOTS_STEP_CARRY
    bool step_kkt;          // DOTS_STEP_KKT_SUMS
    int zmid_mode;          // 0: read z_mid; 1: rebuild it from the multiplier and store it; 2: rebuild, do not store
    bool fused_present;     // the buffers of the fused KKT sums exist
    bool fused_fit;         // ... and hold the launch's workgroups
    bool slab;              // a time slab
    bool step_palm;         // DOTS_STEP_PALM
    bool can_defer;         // DOTS_ZMID_DEFER and the alternate B buffer exists
    bool tp4;               // pitch >= 4: two nodes per lane
    bool bm_nt;             // FrontSchedule::bm_nt
    bool pending;           // a penalty division is to be applied as the launch reads
};
struct QlChoice {
    QlKernel kernel;
    int Z;                  // the kernel's Z mode
    int emit;               // carry kernel: 1 the next iteration's gathers, 2 the fused KKT sums (its K argument)
    bool defer;             // z_mid on demand: the new B / beta_mid go to the alternate buffers (Ctx::swap_deferred_zmid)
    int path;               // STEP_PATH_QL_*
    bool divides;           // the kernel has a dividing instantiation (the carry kernel alone)
    bool refused;           // a division is pending and the kernel cannot apply it: nothing may be launched
};
inline QlChoice ql_choice(const QlFacts &f) {
    QlChoice o{};
    // DOTS_STEP_KKT_SUMS: the launch also leaves the sums of the KKT conditions it can form from its registers and the per-corner gather of
    // Dual(alpha); it takes the carry mapping (whole triangles per workgroup) whether or not the next iteration's gathers are wanted (emit)
    const bool kkt = f.step_kkt && f.zmid_mode == 1 && f.fused_present && f.carry_possible && !f.slab;
    const bool carry = f.carry_possible && f.step_carry && f.zmid_mode >= 1;
    o.kernel = (carry || kkt) ? QL_CARRY : f.tp4 ? QL_TRIANGLE2 : QL_TRIANGLE;
    o.divides = o.kernel == QL_CARRY;
    o.refused = f.pending && !o.divides;
    if (o.kernel != QL_CARRY) {
        o.Z = f.zmid_mode;
        o.path = (o.kernel == QL_TRIANGLE2 ? STEP_PATH_QL_TRIANGLE2 : STEP_PATH_QL_TRIANGLE) | (o.Z << STEP_PATH_QL_Z_SHIFT);
        return o;
    }
    const bool k = kkt && f.fused_fit;      // (only with zmid_mode 1: the fused sums go with a stored or deferred z_mid)
    o.emit = (carry ? 1 : 0) | (k ? 2 : 0);
    o.defer = f.zmid_mode == 1 && f.can_defer && !f.slab && !f.step_palm;
    o.Z = (f.zmid_mode == 2 || o.defer) ? 2 : 1;
    o.path = STEP_PATH_QL_CARRY | (o.Z << STEP_PATH_QL_Z_SHIFT) | (k ? STEP_PATH_QL_KKT : 0) | (f.pending ? STEP_PATH_QL_DIV : 0) |
             (f.bm_nt ? STEP_PATH_QL_BMNT : 0) | (o.defer ? STEP_PATH_QL_DEFER : 0);
    return o;
}

}  // namespace dots

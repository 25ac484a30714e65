// What a call does to the work a context carries from one call to the next: the rules as one table, and the two operations every
// entry point of dots_api.hip opens with.  Host code that knows nothing of HIP: the runtime is reached through `Runtime`, so that a
// stand-alone program can run every row against every kind of carried work (tests/admission_probe.cpp).
#pragma once

#include <string>

#include "../../include/dots_socp_hip.h"

namespace dots {

void set_error(const std::string &msg);      // dots_last_error's text: the library's, or the probe's

enum ZMid : int {
    ZMID_STORED = 0,       // z_mid's storage holds the z_mid of the current iterate
    ZMID_DEFERRED,         // it holds the OLD beta_mid and B_alt the OLD B (Ctx::B_alt): rebuilt before anything reads z_mid
    ZMID_UNSPECIFIED       // it does not belong to the current iterate (DOTS_STEP_SKIP_Z_MID, or nobody asked for a deferred one)
};

// The deferred work of a context.  Results never depend on any of it (include/dots_socp_hip.h).
struct Carried {
    double pending_div = 0.0;     // a penalty division not yet applied to the five dual arrays (0: none)
    int carry_valid = 0;          // the per-corner gathers steps 2+3 left (cn_sq, cn_g) belong to the current iterate
    int kkt_fused_valid = 0;      // the KKT partial sums steps 2+3 left belong to the current iterate and parameters
    int step_path = 0;            // STEP_PATH_* of the last iteration's launches (a right-hand side starts a new record)
    int deep_path = 0;            // DEEP_PATH_* of the last right-hand side and inverse transform
    int rhs_ahead_armed = 0;      // DOTS_STEP_RHS_AHEAD: the next KKT launch is followed by the next iteration's right-hand side
    int rhs_ahead = 0;            // ... which is on the stream and still valid; 2: with the cone projection, whose results wait in the
                                  // alternate buffers; 3 / 4: started by the penalty decision ahead of the host with the division `ahead_dv`
                                  // applied as it read and the penalty `ahead_r`: 2 once dots_adjust_penalty (3 -> 4) and dots_set_params
                                  // (4 -> 2) confirm both
    double ahead_div = 0.0;       // rhs_ahead == 2: the division the launch ahead applied as it read (steps 2+3 of the step that takes it apply the same)
    int penalty_armed = 0;        // dots_penalty_ahead: the next evaluation of conditions 0-3 takes the penalty decision itself
    ZMid zmid = ZMID_STORED;
    int kkt_halo_fresh = 0;       // time slab: mu_lo / B_hi belong to the current iterate
    int needs_restart = 0;        // dots_move_vertices changed the surface under the iterate: dots_restart before the next step

    // ---- the drops, each written once ----
    // a call that changes the state or the parameters: the launch ahead, the armed decisions and what steps 2+3 left belong to what was
    void drop_for_change() { rhs_ahead = rhs_ahead_armed = penalty_armed = carry_valid = kkt_fused_valid = step_path = deep_path = 0; }
    void drop_for_step0() { carry_valid = kkt_fused_valid = step_path = deep_path = 0; }      // step 0 of PALM moves A, B and lambda_c
    void drop_for_steps23() { carry_valid = kkt_fused_valid = 0; }                             // a new steps 2+3 launch replaces both
    // steps 2+3 ran, or are about to (a launch that defers says so itself, before or after this)
    void stepped(bool skip_zmid) {
        if (skip_zmid) zmid = ZMID_UNSPECIFIED;
        else if (zmid == ZMID_UNSPECIFIED) zmid = ZMID_STORED;
    }
};

enum Access : unsigned {
    DROPS = 1,       // changes the state or the parameters (or counts as such): Carried::drop_for_change
    DUALS = 2,       // reads or writes the dual arrays: a pending division is carried out first
    STATE = 4,       // really changes the arrays: the KKT halos of a slab go stale (state_changed, where the call has succeeded so far)
    SURFACE = 8      // steps or measures the iterate on its surface: refused while needs_restart is set
};
enum Need : int { NEVER = 0, ALWAYS, BY_ARGUMENT };

struct Row {
    const char *name;        // as the error texts have it
    unsigned access;
    Need reads;              // z_mid is read from memory: one left to be rebuilt is rebuilt first
    Need refuses;            // ... and an unspecified one is refused, with the text `stale`
    const char *stale;
};

// One value per exported function that takes a context (a second one where two contexts of a call are treated differently).
// dots_get_params, dots_array_count, dots_device_bytes, dots_slab_elems, dots_debug_counter and dots_destroy are not admitted: they
// read host fields only (or end the context) and have no row.
enum Entry : int {
    E_SET_PARAMS, E_RESTART,
    E_PENALTY_AHEAD, E_SYNC, E_STREAM_WAIT, E_STEP_FLAGS, E_STEP_TIMES, E_GEOMETRY_COPY, E_FRONT_SHARE_OWNER,
    E_STEP, E_STEP_MANY,
    E_SLAB_STAGE, E_KKT_COMBINE, E_OBJECTIVE_COMBINE, E_READOUT, E_SENSITIVITY, E_FLOW_MAP, E_FLOW_PUSH, E_FLOW_TRACE, E_FLOW_SLIDE,
    E_DOWNLOAD,
    E_KKT, E_KKT_SUMS, E_KKT_SUMS_DEVICE, E_OBJECTIVE, E_OBJECTIVE_SUMS,
    E_PROLONG_TIME_SRC, E_PROLONG_SPACE_SRC, E_TRANSFER_SPACE_SRC, E_CARRY_SPACETIME_SRC,
    E_PROLONG_TIME, E_PROLONG_SPACE, E_TRANSFER_SPACE, E_CARRY_SPACETIME,
    E_UPLOAD, E_ADJUST_PENALTY, E_SCALE_Z, E_SCALE_ARRAYS, E_MOVE_VERTICES, E_MOVE_VERTICES_MANY,
    E_RUN_PHASE, E_NORM_SQUARE,
    E_APPLY_OPERATOR, E_SLAB_SET_BUFFERS, E_MG_SETUP, E_MG_ENABLE, E_MG_APPLY, E_FRONT_SETUP, E_FRONT_SHARE, E_FRONT_ENABLE, E_PCG_WINDOWS,
    E_FRONT_LAUNCHES, E_FRONT_INFO, E_FRONT_PITCH, E_BENCH_KERNEL, E_LAPLACIAN_SOLVE_MANY, E_BENCH_MANY,
    N_ENTRIES
};

#define DOTS_STALE(who) who ": z_mid was not materialised by the last step (dots_step_flags)"
#define DOTS_STALE_SOURCE(who) who ": the source's z_mid was not materialised by its last step (dots_step_flags)"
constexpr Row ADMISSION[N_ENTRIES] = {
    {"set_params", DROPS, NEVER, NEVER, nullptr},
    // (warm: the division is carried out, then z_mid refused or rebuilt; the refusal comes before anything is dropped)
    {"restart", DROPS | STATE, BY_ARGUMENT, BY_ARGUMENT, DOTS_STALE("restart") ": no warm start from this iterate"},
    {"penalty_ahead", 0, NEVER, NEVER, nullptr},
    {"sync", 0, NEVER, NEVER, nullptr},
    {"stream_wait", 0, NEVER, NEVER, nullptr},
    {"step_flags", 0, NEVER, NEVER, nullptr},
    {"step_times", 0, NEVER, NEVER, nullptr},
    {"geometry_copy", 0, NEVER, NEVER, nullptr},
    {"front_share", 0, NEVER, NEVER, nullptr},      // the owner
    // (an iteration consumes the carried work and a pending division itself; the argument is DOTS_STEP_PALM, whose step 0 reads z_mid)
    {"step", SURFACE, BY_ARGUMENT, BY_ARGUMENT, "step: DOTS_STEP_PALM needs z_mid of the previous iteration in memory"},
    {"step_many", SURFACE, BY_ARGUMENT, BY_ARGUMENT, "step: DOTS_STEP_PALM needs z_mid of the previous iteration in memory"},
    // (the stages say themselves what they invalidate: carried sums live from stage 3 to the next stages 0 and 1)
    {"slab_stage", DUALS, NEVER, NEVER, nullptr},
    {"kkt_combine", DUALS, NEVER, NEVER, nullptr},
    {"objective_combine", DUALS, NEVER, NEVER, nullptr},
    {"readout", DUALS, NEVER, NEVER, nullptr},
    {"sensitivity", DUALS, NEVER, NEVER, nullptr},
    {"flow_map", DUALS, NEVER, NEVER, nullptr},
    {"flow_push", DUALS, NEVER, NEVER, nullptr},
    {"flow_trace", DUALS, NEVER, NEVER, nullptr},
    {"flow_slide", DUALS, NEVER, NEVER, nullptr},
    {"download", DUALS, BY_ARGUMENT, BY_ARGUMENT, DOTS_STALE("download")},      // id == DOTS_Z_MID
    // (refused when Prim(q, z) is in the mask; rebuilt when the sums steps 2+3 left are not taken for it: kkt_prelude)
    {"kkt", DUALS | SURFACE, BY_ARGUMENT, BY_ARGUMENT, DOTS_STALE("kkt")},
    {"kkt_sums", DUALS | SURFACE, BY_ARGUMENT, BY_ARGUMENT, DOTS_STALE("kkt")},
    {"kkt_sums_device", DUALS | SURFACE, BY_ARGUMENT, BY_ARGUMENT, DOTS_STALE("kkt")},
    {"objective", DUALS | SURFACE, NEVER, NEVER, nullptr},
    {"objective_sums", DUALS | SURFACE, NEVER, NEVER, nullptr},
    {"prolong_time", DUALS, ALWAYS, ALWAYS, DOTS_STALE_SOURCE("prolong_time")},      // the source of a carrier
    {"prolong_space", DUALS, ALWAYS, ALWAYS, DOTS_STALE_SOURCE("prolong_space")},
    {"transfer_space", DUALS, ALWAYS, ALWAYS, DOTS_STALE_SOURCE("transfer_space")},
    {"carry_spacetime", DUALS, ALWAYS, ALWAYS, DOTS_STALE_SOURCE("carry_spacetime")},
    {"prolong_time", DROPS | STATE, NEVER, NEVER, nullptr},      // its destination (a pending division is discarded: every array is replaced)
    {"prolong_space", DROPS | STATE, NEVER, NEVER, nullptr},
    {"transfer_space", DROPS | STATE, NEVER, NEVER, nullptr},
    {"carry_spacetime", DROPS | STATE, NEVER, NEVER, nullptr},
    {"upload", DROPS | DUALS | STATE, BY_ARGUMENT, NEVER, nullptr},      // id != DOTS_Z_MID
    {"adjust_penalty", DROPS | DUALS | STATE, NEVER, NEVER, nullptr},
    {"scale_z", DROPS | DUALS | STATE, ALWAYS, NEVER, nullptr},
    {"scale_arrays", DROPS | DUALS | STATE, ALWAYS, NEVER, nullptr},
    {"move_vertices", DROPS | DUALS | STATE, ALWAYS, NEVER, nullptr},      // (z_mid is rebuilt from tables that are about to change)
    {"move_vertices_many", DROPS | DUALS | STATE, ALWAYS, NEVER, nullptr},
    {"run_phase", DROPS | DUALS | SURFACE, ALWAYS, BY_ARGUMENT, DOTS_STALE("phase q_lambda")},      // phase == DOTS_PHASE_Q_LAMBDA
    {"norm_square", DROPS | DUALS, BY_ARGUMENT, BY_ARGUMENT, DOTS_STALE("norm_square")},            // id == DOTS_Z_MID
    {"apply_operator", DROPS | DUALS, NEVER, NEVER, nullptr},
    {"slab_set_buffers", DROPS | DUALS, NEVER, NEVER, nullptr},
    {"mg_setup", DROPS | DUALS, NEVER, NEVER, nullptr},
    {"mg_enable", DROPS | DUALS, NEVER, NEVER, nullptr},
    {"mg_apply", DROPS | DUALS, NEVER, NEVER, nullptr},
    {"front_setup", DROPS | DUALS, NEVER, NEVER, nullptr},
    {"front_share", DROPS | DUALS, NEVER, NEVER, nullptr},      // the sharer
    {"front_enable", DROPS | DUALS, NEVER, NEVER, nullptr},
    {"pcg_windows", DROPS | DUALS, NEVER, NEVER, nullptr},
    {"front_launches", DROPS | DUALS, NEVER, NEVER, nullptr},      // (the three queries count as calls that change something)
    {"front_info", DROPS | DUALS, NEVER, NEVER, nullptr},
    {"front_pitch", DROPS | DUALS, NEVER, NEVER, nullptr},
    {"bench_kernel", DROPS | DUALS, BY_ARGUMENT, NEVER, nullptr},      // the kernels that read z_mid
    {"laplacian_solve_many", DROPS | DUALS, NEVER, NEVER, nullptr},
    {"bench_many", DROPS | DUALS, NEVER, NEVER, nullptr},
};
#undef DOTS_STALE
#undef DOTS_STALE_SOURCE

// What needs the runtime, on the context `ctx` the Carried belongs to; each returns a dots_status
struct Runtime {
    int (*select_device)(void *ctx);              // hipSetDevice
    int (*divide)(void *ctx, double factor);      // the stand-alone pass over the five dual arrays
    int (*rebuild_zmid)(void *ctx);               // z_mid from the old B / beta_mid a deferred step kept
};

// A pending penalty division carried out now
inline int flush_division(Carried &k, const Runtime &rt, void *ctx) {
    if (k.pending_div == 0.0) return 0;
    const double f = k.pending_div;
    k.pending_div = 0.0;
    return rt.divide(ctx, f);
}

// The first lines of every entry point.  `k`: the context's carried work, null with a null context.
inline int admit(Carried *k, Entry e, const Runtime &rt, void *ctx) {
    const Row &row = ADMISSION[e];
    if (!k) { set_error("null context"); return DOTS_ERR_ARGUMENT; }
    int rc = rt.select_device(ctx);
    if (rc) return rc;
    if (row.access & DROPS) k->drop_for_change();
    if ((row.access & DUALS) && (rc = flush_division(*k, rt, ctx))) return rc;
    if ((row.access & SURFACE) && k->needs_restart) {
        set_error(std::string("dots_") + row.name + ": the vertices were moved (dots_move_vertices): the context needs a dots_restart (cold or warm) first");
        return DOTS_ERR_STATE;
    }
    return 0;
}

// The call has changed the arrays (rows with STATE), at the point where it can no longer be refused without having done so
inline void state_changed(Carried &k) { k.kkt_halo_fresh = 0; }

inline int refuse_unspecified_zmid(const Carried &k, Entry e) {
    if (k.zmid != ZMID_UNSPECIFIED) return 0;
    set_error(ADMISSION[e].stale);
    return DOTS_ERR_STATE;
}
inline int rebuild_zmid(Carried &k, const Runtime &rt, void *ctx) {
    if (k.zmid != ZMID_DEFERRED) return 0;
    k.zmid = ZMID_STORED;
    return rt.rebuild_zmid(ctx);
}
// The call reads z_mid from memory.  `argument`: what a BY_ARGUMENT column of the row depends on holds for this call.
inline int need_zmid(Carried &k, Entry e, const Runtime &rt, void *ctx, bool argument = true) {
    const Row &row = ADMISSION[e];
    int rc;
    if ((row.refuses == ALWAYS || (row.refuses == BY_ARGUMENT && argument)) && (rc = refuse_unspecified_zmid(k, e))) return rc;
    if (row.reads == ALWAYS || (row.reads == BY_ARGUMENT && argument)) return rebuild_zmid(k, rt, ctx);
    return 0;
}

}  // namespace dots

/*
 * dots_socp_hip.h -- C ABI of libdotsocp_hip.so, the MI355X (gfx950) implementation of the
 * DOTs-SOCP ALM hot path.
 *
 * The reference is pure Python (no FFI exists in it); these entry points are what a ctypes
 * binding placed at the reference's solver plug-in boundary would bind.  Each function names the
 * reference code it replaces (paths relative to the reference root, file:line).
 *
 * Conventions
 *   - every function returns 0 on success, a negative dots_status otherwise; the message of the
 *     last failure is available from dots_last_error() (per thread).
 *   - host pointers are borrowed for the duration of the call only; device memory belongs to the
 *     context.  One host thread per context.
 *   - host-side state arrays use the REFERENCE layouts and fp64:
 *       phi                          (T+1, V)
 *       A, lambda_c, mu, z_fst, z_end, beta_fst, beta_end   (T, V)
 *       B, E                         (T+1, F, 3)
 *       z_mid, beta_mid              (T, 2, 3, F, 3)
 *     the device layout (vertex/triangle-major, time fastest) is internal.
 *     A time-slab context (multi-GPU, dots_problem_desc.slab_*) exchanges its OWN time extent only:
 *       phi (n, V); interval arrays (m, V); B, E (n, F, 3) with n = slab_count nodes, m = min(n, T - slab_begin)
 *       intervals; z_mid, beta_mid (n, 2, 3, F, 3) indexed by the NODE an entry is compared with: entry [j][s] is the
 *       reference's [slab_begin + j - s][s] (entries whose interval does not exist: ignored on upload, zero on download).
 *       dots_upload of phi also takes (n + 1, V) on a slab that has a next slab: the last row is phi at that slab's first node,
 *       which stage 3 computes redundantly and step 0 of DOTS_STEP_PALM and the KKT sums read.  Without that row the node keeps
 *       what the last stage 3 left (zero on a fresh context): upload it whenever one of the two follows before a stage 3.
 *   - a context carries deferred work from one call to the next (a penalty division not yet applied, sums and gathers the last
 *     iteration left, a right-hand side launched ahead, a z_mid left to be rebuilt); results never depend on it.  What a call does
 *     to that work follows from four properties, one table row per function (csrc/admission.h; DESIGN.md, "What a call does to
 *     deferred work"): it DROPS what belongs to the old state or parameters; it uses the DUAL arrays, so a pending division is
 *     carried out first; it changes the STATE, so a slab's KKT halos go stale; it steps or measures the iterate on its SURFACE,
 *     so it is refused after dots_move_vertices until a dots_restart.  A call that reads z_mid from memory rebuilds one that
 *     was left to be rebuilt, and where the row says so refuses one that is unspecified.
 *   - no C++ exceptions, torch types or Python objects cross this boundary.
 */
#ifndef DOTS_SOCP_HIP_H
#define DOTS_SOCP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only what this header declares is exported */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define DOTS_ABI_VERSION 7

typedef struct dots_ctx dots_ctx;

enum dots_status {
    DOTS_OK = 0,
    DOTS_ERR_ARGUMENT = -1,
    DOTS_ERR_HIP = -2,
    DOTS_ERR_NO_DEVICE = -3,
    DOTS_ERR_NOT_CONVERGED = -4,
    DOTS_ERR_STATE = -5,
    DOTS_ERR_MEMORY = -6      /* dots_front_setup: the factor (+ its workspace) does not fit the device memory that is free */
};

/* state arrays, same names as SolutionSocpData (dot_surface_socp/utils/type.py:22-38) */
enum dots_array {
    DOTS_PHI = 0, DOTS_A, DOTS_B, DOTS_LAMBDA_C, DOTS_Z_FST, DOTS_Z_MID, DOTS_Z_END,
    DOTS_MU, DOTS_E, DOTS_BETA_FST, DOTS_BETA_MID, DOTS_BETA_END,
    DOTS_N_ARRAYS
};

/* the seven KKT residuals in the order of solver_socp.py:590-640 */
enum dots_kkt_id {
    DOTS_KKT_PRIM_Q = 0, DOTS_KKT_PRIM_Z, DOTS_KKT_DUAL_ALPHA, DOTS_KKT_DUAL_BETA,
    DOTS_KKT_COMP_RHO_FQ, DOTS_KKT_COMP_M_RHO_B, DOTS_KKT_COMP_CONGESTION,
    DOTS_N_KKT
};

/* which Laplacian solver runs in step 1 (replaces laplacian_inverse_socp.py:11-61) */
enum dots_lap_solver {
    DOTS_LAP_SPACETIME_PCG = 0, /* Jacobi-PCG on the assembled space-time operator            */
    DOTS_LAP_MODAL_PCG = 1      /* time eigen-modes decoupled (DCT): batched shifted-surface PCG, or -- once a factor is
                                   installed with dots_front_setup -- the direct multifrontal sweeps (the default of
                                   the Python driver: lap_solver="modal_direct").  T+1 <= 1024 on one GPU; above 256
                                   only the direct sweeps step (dots_step, dots_run_phase(LAPLACIAN) and dots_mg_setup
                                   return DOTS_ERR_STATE without a factor); time slabs need T+1 <= 256 */
};

/*
 * Problem description: the outputs of the reference's operator assembly
 * (utils/surface_pre_computations_socp.py:11-132, solver_socp.py:102-113,161-192) as flat arrays.
 * The host side (dots_socp_amd/geometry.py) builds them; all index arrays are 0-based int32.
 */
typedef struct dots_problem_desc {
    int32_t abi_version;     /* DOTS_ABI_VERSION */
    int32_t device;          /* HIP device ordinal */
    int32_t n_time;          /* T: number of time intervals (T+1 nodes, T+1 <= 1024; see dots_lap_solver) */
    int32_t n_vertices;      /* V */
    int32_t n_triangles;     /* F */
    int32_t n_corners;       /* = 3 F, length of the vertex->corner lists */
    int32_t lap_nnz;         /* non-zeros of the surface stiffness matrix */
    int32_t lap_solver;      /* enum dots_lap_solver */

    const int32_t *triangles;    /* [F][3]                                                     */
    const double *hat_grad;      /* [F][3 corners][3 xyz] hat-function gradients (:31-37)       */
    const double *area_tri;      /* [F]                                                        */
    const double *mass_vert;     /* [V]  = (sum of incident triangle areas) / 3  (solver_socp.py:112) */
    const int32_t *corner_ptr;   /* [V+1] vertex -> corner list (CSR)                           */
    const int32_t *corner_idx;   /* [3F]  entries f*3+k, the corners (f,k) with triangles[f][k]==v */
    const int32_t *lap_rowptr;   /* [V+1]  K = -cotangent Laplacian (= G^T diag(area) G), CSR, SPD-semidefinite */
    const int32_t *lap_col;      /* [nnz]                                                       */
    const double *lap_val;       /* [nnz]                                                       */
    const double *mu0;           /* [V] boundary masses (geometry["mu0"], solver_socp.py:267-270) */
    const double *mu1;           /* [V]                                                         */
    const int32_t *perm_vert;    /* [V] device vertex i is caller vertex perm_vert[i]; NULL = identity */
    const int32_t *perm_tri;     /* [F] device triangle i is caller triangle perm_tri[i]; NULL = identity */
    const double *time_modes;    /* [(T+1)*(T+1)] row-major Q[t][a]: orthonormal eigenvectors of the Neumann
                                    time Laplacian (laplacian_inverse_socp.py:15-31); NULL unless MODAL */
    const double *time_eigs;     /* [T+1] eigenvalues sigma_a >= 0 of -L_time;  NULL unless MODAL */
    /* Multi-GPU (one context per rank): TIME SLABS.  This context holds the time nodes [slab_begin, slab_begin +
     * slab_count) of every state array (and the intervals that start at them) and solves the time modes with the same
     * indices; slab_stride = nodes per rank (ceil((T+1)/n_ranks), the same on every rank; slab_count may be smaller, or
     * 0, on trailing ranks).  All zero = single GPU.  See dots_slab_stage. */
    int32_t slab_begin;
    int32_t slab_count;
    int32_t slab_stride;
    int32_t reserved;
    const int32_t *patch_order;  /* ignored (kept for the layout of ABI version 7; pass NULL) */
} dots_problem_desc;

/* Scalars the host control logic owns (solver_socp.py:97,318-321 and the kwargs of :25-41). */
typedef struct dots_params {
    double r;              /* penalty                                   */
    double scale_z;        /* scale_factor_z                            */
    double const_d;        /* constant_d                                */
    double norm_d;         /* norm_constant_d (:297,380)                */
    double norm_boundary;  /* norm_boundary (:296)                      */
    double congestion;
    double tau;
    double eps;
    double prim_scale;
    double dual_scale;
    double boundary_scale; /* multiplies the boundary term (-mu0, +mu1)/(r h); 1 unless constant scaling (:357-358) */
    double cg_tol;         /* PCG stops when r^T M^-1 r <= cg_tol^2 * b^T M^-1 b */
    int32_t cg_max_iter;
    int32_t reserved;
} dots_params;

typedef struct dots_step_stats {
    int32_t alm_iterations;     /* iterations performed by this call                     */
    int32_t cg_iterations;      /* PCG iterations summed over them                        */
    int32_t cg_last_iterations; /* PCG iterations of the last one                         */
    int32_t cg_not_converged;   /* number of solves that hit cg_max_iter                  */
    double cg_last_rel_residual;
    double ms_rhs;              /* hipEvent times summed over the call, milliseconds      */
    double ms_laplacian;
    double ms_soc;
    double ms_q_lambda_multiplier;
    double ms_total;
} dots_step_stats;

/* ---- lifecycle ------------------------------------------------------------------------- */
int dots_abi_version(void);
const char *dots_last_error(void);

/* Build the device-resident problem: replaces the setup of solver_socp.py:96-313 (constants,
 * Laplacian operator, zero-initialised state as :239-250 with an empty init_solution). */
int dots_create(const dots_problem_desc *desc, dots_ctx **out);
int dots_destroy(dots_ctx *ctx);
int dots_set_params(dots_ctx *ctx, const dots_params *p);
int dots_get_params(dots_ctx *ctx, dots_params *p);
int dots_sync(dots_ctx *ctx);

/* ---- state transfer (init_solution in, SolutionSocpData out; solver_socp.py:239-250,855-869) */
int dots_upload(dots_ctx *ctx, int array_id, const double *host, int64_t count);
int dots_download(dots_ctx *ctx, int array_id, double *host, int64_t count);
int64_t dots_array_count(dots_ctx *ctx, int array_id);

/* ---- the hot loop ------------------------------------------------------------------------ */
/* n ALM iterations, steps 1-3 of solver_socp.py:674-722 (is_palm = False), device resident.
 * stats == NULL: the iterations are only enqueued on the context's stream (no host wait, nothing timed;
 * meant for the direct solver, which needs no host round trip) -- any later call that returns data waits. */
int dots_step(dots_ctx *ctx, int n_iters, dots_step_stats *stats);

/* Flags for the following dots_step / dots_slab_stage calls.
 * DOTS_STEP_SKIP_Z_MID: z_mid (18*T*F values, an intermediate between the cone projection and steps 2+3) is
 * rebuilt on the fly and not stored: the iterate is the same bit for bit, but z_mid in memory is unspecified
 * afterwards.  dots_kkt(PRIM_Z) and dots_download(Z_MID) then fail with DOTS_ERR_STATE until a step without the
 * flag (or an upload / the projection phase) has produced it again.  The host driver sets it on the iterations
 * after which neither KKT residuals nor the solution are read (solver_socp.py's lazy validator, :766-788). */
#define DOTS_STEP_SKIP_Z_MID 1u
/* DOTS_STEP_PALM: every iteration opens with the (q, lambda_c) closed form alone ("Step 0" of is_palm = True,
 * solver_socp.py:668-672: A, B, lambda_c from the current multipliers, the stored z_mid and grad(phi) of the previous
 * iteration).  It reads z_mid from memory, so it cannot be combined with DOTS_STEP_SKIP_Z_MID (DOTS_ERR_ARGUMENT). */
#define DOTS_STEP_PALM 2u
/* DOTS_STEP_RHS_AHEAD (a hint: ignored without the direct solver or on a time slab; DOTS_ERR_ARGUMENT with DOTS_STEP_PALM): the caller expects the
 * iteration AFTER the next dots_step to start from the state that step leaves (no penalty update, no rescaling in between).
 * The first dots_kkt / dots_kkt_sums call after that step then enqueues the next iteration's right-hand side behind its own
 * kernels, so that the device works while the host waits for the residuals and decides; the following dots_step starts at the
 * solve.  Any call in between that changes the state or the parameters (dots_set_params, dots_upload, dots_adjust_penalty,
 * dots_scale_*, dots_run_phase, ...) drops that right-hand side and the step computes it again: results never depend on the
 * flag.  The flag holds for one dots_step. */
#define DOTS_STEP_RHS_AHEAD 4u
/* DOTS_STEP_TIMED: enqueue-only steps (dots_step / dots_slab_stage with stats == NULL) bracket their phases with events of an
 * internal ring of 64 slots (one per dots_step iteration, one per slab stage) WITHOUT waiting for them; dots_step_times collects
 * the finished slots later, oldest first (the reference's per-step timers, utils/admm_tools.py:244-251, without a host wait in
 * the loop).  A step that finds the ring full is simply not timed. */
#define DOTS_STEP_TIMED 8u
/* DOTS_STEP_CARRY (a hint: ignored without the direct solver, with DOTS_STEP_PALM or a time pitch above 128; a time slab with a factor
 * carries too, at its own pitch: its stage 0 packs send_nsq from the carried sums, stages 1 / 6 and 5 stream them): the caller
 * expects the NEXT iteration to start from the state this step leaves.  Steps 2+3 then also store, per corner of every triangle,
 * what the next right-hand side (solver_socp.py:983-986: div_x((B - E) area)) and the next cone projection (:997-1017: the squared
 * norm of D (L B - beta_mid)) would gather from B, E and beta_mid -- they hold those values in registers when they write them
 * (:716-722) -- and the next dots_step streams these per-corner sums instead of reading beta_mid a third time.  Any call in
 * between that changes the state or the parameters drops them and the step gathers from the arrays again: results never depend
 * on the flag, bit for bit (both paths form the same sums in the same order). */
#define DOTS_STEP_CARRY 16u
/* DOTS_STEP_KKT_SUMS (a hint: one GPU, ignored with DOTS_STEP_SKIP_Z_MID): the caller will read KKT residuals after this step.  Steps 2+3
 * then also accumulate the weighted sums of Prim(phi, q), Prim(q, z), Dual(beta) and Comp(rho, cong.) (solver_socp.py:433-464,
 * 484-503, 549-559) from the values they hold in registers as they write the new iterate; a following dots_kkt / dots_kkt_sums
 * whose mask holds only these conditions and Dual(alpha) reduces those partial sums (plus one vertex pass for Dual(alpha))
 * instead of reading the state again.  Any call in between that changes the state or the parameters drops them.  The residuals
 * agree with the stand-alone evaluation to rounding (the sums are formed in a different order). */
#define DOTS_STEP_KKT_SUMS 32u
int dots_step_flags(dots_ctx *ctx, uint32_t flags);      /* also apply to dots_slab_stage */
/* The phase times of the timed steps that have finished (wait != 0: of all timed steps, waiting for them), oldest first, at
 * most `capacity`: one dots_step_stats per dots_step iteration (alm_iterations = 1), or one per slab stage (the stage's time in
 * the field of its phase; stage 3 carries alm_iterations = 1). */
int dots_step_times(dots_ctx *ctx, dots_step_stats *out, int capacity, int wait, int *n_out);

/* ---- time slabs (multi-GPU): one ALM iteration in four stages around three exchanges --------------------------------
 * Every operator of the iteration is local in time except nearest-neighbour couplings (solver_socp.py:884, :892-894,
 * :934-940, :955-957), and the Laplacian solve decouples over the time MODES (laplacian_inverse_socp.py:31-41).  Rank r
 * holds the slab of nodes [r s, (r+1) s) of the whole state (s = slab_stride) and solves the modes [r s, (r+1) s):
 *
 *   stage 0   [is_palm: the (q, lambda_c) closed form]; pack what the neighbours need:
 *               send_x   [V]  (A + lambda_c - mu) of this slab's last interval          -> next rank's  recv_x
 *               send_nsq [V]  the s = 1 half of the cone norms of the interval that ends at this slab's first node
 *                             (formed from this slab's B and beta_mid)                    -> previous rank's recv_nsq
 *   (caller)  neighbour exchange (two V-sized messages per slab boundary)
 *   stage 1   right-hand side of this slab's nodes -> b_send = [V][pitch], and the cone projection of its intervals (one launch);
 *             the cone multipliers of the slab's last interval go to the tail [V] of x_send (the next slab's steps 2+3 read them)
 *             -- or in two halves, so that the exchange overlaps the projection:
 *   stage 6     the right-hand side alone;  (caller) starts the all-gather of b_send;
 *   stage 5     the cone projection alone, enqueued behind stage 6 on the context's stream while the all-gather runs on the
 *               caller's (the projection reads nothing the right-hand side, the all-gather or the solve writes: steps 1-1 and
 *               1-2 of solver_socp.py:674-696 minimise a separable block -- the reference runs them on two threads)
 *   (caller)  all-gather of b_send into b_recv = [n_ranks][V * pitch]
 *   stage 2   forward time transform restricted to this rank's modes, solve (sweeps or PCG); x_send = [V][pitch] solution (+ tail)
 *   (caller)  all-gather of x_send into x_recv = [n_ranks][V * pitch + V]
 *   stage 3   inverse time transform for this slab's nodes (+ the next slab's first node, computed redundantly),
 *             steps 2 and 3
 *   stage 4   (only before KKT residuals are evaluated) pack send_mu [V] (mu of the last interval -> next rank) and
 *             send_b [3F] (B of the first node -> previous rank); the caller exchanges them, then dots_kkt_sums
 *
 * Stages must be called in order 0,1,2,3 or 0,6,5,2,3 (DOTS_ERR_STATE otherwise).  With stats == NULL a stage is only enqueued on the
 * context's stream: the caller orders its exchanges against it with dots_stream_wait (no host wait anywhere).
 * All buffers are DEVICE memory owned by the caller (e.g. torch tensors handed to RCCL), registered once with
 * dots_slab_set_buffers; sizes from dots_slab_elems.  Results are bit-identical for rank counts of equal slab pitch
 * (max(4, slab_stride rounded up to a power of two): the element-wise steps form the same sums in the same order wherever a
 * value is computed, the sweeps of the direct solver split their dot products by that pitch); only the KKT / objective sums
 * differ in rounding (partial sums per slab). */
typedef struct dots_slab_buffers {
    double *send_x, *send_nsq;      /* [V] each: stage 0 output                                              */
    double *recv_x, *recv_nsq;      /* [V] each: from the previous / next rank                               */
    double *b_send, *b_recv;        /* [V * pitch],     [n_ranks][V * pitch]                                 */
    double *x_send, *x_recv;        /* [V * pitch + V], [n_ranks][V * pitch + V]                             */
    double *send_mu, *send_b;       /* [V], [3F]: stage 4 output                                             */
    double *recv_mu, *recv_b;       /* [V], [3F]: from the previous / next rank                              */
} dots_slab_buffers;
enum dots_slab_size { DOTS_SLAB_VERTEX_HALO = 0, DOTS_SLAB_B_CHUNK = 1, DOTS_SLAB_X_CHUNK = 2, DOTS_SLAB_TRIANGLE_HALO = 3 };
int64_t dots_slab_elems(dots_ctx *ctx, int which);      /* doubles; -1 if the context is not a time slab */
int dots_slab_set_buffers(dots_ctx *ctx, const dots_slab_buffers *buffers);
int dots_slab_stage(dots_ctx *ctx, int stage, dots_step_stats *stats);
/* Stream ordering between the context's stream and another HIP stream of the same device (e.g. the one a
 * communication library works on; NULL = the legacy default stream).  ctx_waits = 0: work enqueued on
 * `other_stream` after the call waits for everything enqueued on the context so far; 1: the reverse. */
int dots_stream_wait(dots_ctx *ctx, void *other_stream, int ctx_waits);

/* single phases of one iteration, for per-function parity tests */
enum dots_phase {
    DOTS_PHASE_LAPLACIAN = 0,        /* vanilla_solve_laplacian  solver_socp.py:976-986 + laplacian_inverse_socp.py:52-61 */
    DOTS_PHASE_SOC_PROJECTION = 1,   /* vanilla_solve_proj_soc   solver_socp.py:988-1042 */
    DOTS_PHASE_Q_LAMBDA_MULT = 2,    /* grad_time/grad_space + vanilla_solve_q_lambda :709-714,1044-1065 and the multiplier update :716-722 */
    DOTS_PHASE_Q_LAMBDA = 3          /* vanilla_solve_q_lambda alone (is_palm's step 0, :668-672): no multiplier moves */
};
/* A phase counts as a call that changes the state: a pending penalty division is carried out first, a z_mid left to be rebuilt is
 * materialised, and the carried gathers, the fused KKT sums, a right-hand side ahead and an armed penalty decision are dropped --
 * also by a phase that is then refused.  While z_mid is unspecified (DOTS_STEP_SKIP_Z_MID) DOTS_PHASE_Q_LAMBDA returns DOTS_ERR_STATE
 * (the arrays are untouched); DOTS_PHASE_Q_LAMBDA_MULT is not refused and reads the unspecified z_mid: the caller runs
 * DOTS_PHASE_SOC_PROJECTION (which makes z_mid valid again) or a step without the flag first. */
int dots_run_phase(dots_ctx *ctx, int phase, dots_step_stats *stats);

/* KKT residuals (closures of solver_socp.py:433-559 as wired at :589-643).  mask: bit i set =
 * evaluate condition i.  out[2*i], out[2*i+1] = the two values the reference's wrapper returns
 * (with prim/dual scale, with scale 1); entries of conditions not in mask are left untouched.
 * For conditions 4..6 the second value does not exist in the reference and is set to NaN. */
int dots_kkt(dots_ctx *ctx, uint32_t mask, double *out /* [2*DOTS_N_KKT] */);
/* The same in two halves, for time slabs: the weighted sums of this context's slab (DOTS_KKT_N_SUMS doubles; on a slab
 * the halos of stage 4 must have been exchanged), and the residuals from the sums of the WHOLE problem (the caller adds
 * the slabs' sums: one all-reduce of a small vector, solver_socp.py:433-559). */
#define DOTS_KKT_N_SUMS 24
int dots_kkt_sums(dots_ctx *ctx, uint32_t mask, double *sums /* [DOTS_KKT_N_SUMS] */);
int dots_kkt_combine(dots_ctx *ctx, uint32_t mask, const double *sums, double *out /* [2*DOTS_N_KKT] */);
/* dots_kkt_sums with the result left in DEVICE memory of the caller (DOTS_KKT_N_SUMS doubles, e.g. a torch tensor handed to
 * RCCL's all-reduce): only enqueued on the context's stream, no host wait, no copy -- order the consumer's stream with
 * dots_stream_wait.  Slots of sums the mask does not need (and every slot on a rank without nodes) are zero.  z_mid is
 * refused and rebuilt as by dots_kkt_sums. */
int dots_kkt_sums_device(dots_ctx *ctx, uint32_t mask, double *device_sums /* [DOTS_KKT_N_SUMS], device memory */);

/* The penalty decision ahead of the host (a hint; one GPU, direct solver).  On the iterations where the reference adapts the penalty
 * (utils/admm_tools.py:30-52) the host reads conditions 0-3, takes the decision (solver_socp.py:806-823, admm_tools.py:54-95), divides
 * the dual arrays and only then starts the next iteration: the device idles meanwhile.  Armed with the policy's numbers, the next
 * dots_kkt / dots_kkt_sums whose mask holds conditions 0-3 takes the SAME decision inside the library as soon as the sums have
 * arrived -- if one of the four conditions fails tol: is_org_kkt |= (max of the unit-scale values < 5 tol); gap = max(prim) / max(dual) of
 * the chosen values; factor from the table (the first threshold that max(gap, 1/gap) exceeds; inverted when gap < 1); r' = clamp(r *
 * factor) -- and starts the next iteration's right-hand side + cone projection with r * (r' / r) and the division by r' / r applied
 * as the arrays are read (results in alternate buffers, as with DOTS_STEP_RHS_AHEAD).  The caller then calls dots_adjust_penalty and
 * dots_set_params as it would anyway: if factor and parameters are the ones anticipated (bit for bit) the next dots_step starts at the
 * solve, otherwise -- or after any other call that changes state -- what was started is dropped.  Results never depend on the hint. */
typedef struct dots_penalty_policy {
    double tol;               /* the conditions pass below tol                                            */
    double r_lower, r_upper;  /* the penalty's clamp (admm_tools.py:25-26)                                 */
    int32_t is_org_kkt;       /* the driver's sticky flag (solver_socp.py:806-808)                         */
    int32_t n_steps;          /* entries of the table, <= 16                                               */
    double threshold[16];     /* descending (admm_tools.py:79-90)                                          */
    double factor[16];
} dots_penalty_policy;
int dots_penalty_ahead(dots_ctx *ctx, const dots_penalty_policy *policy);

/* objective_functional (solver_socp.py:417-431) as called at :773-775/:829-831:
 * out[0] = transportation cost, out[1] = Lagrangian / objective value. */
int dots_objective(dots_ctx *ctx, double *out /* [2] */);
int dots_objective_sums(dots_ctx *ctx, double *sums /* [3] */);
int dots_objective_combine(dots_ctx *ctx, const double *sums /* [3] */, double *out /* [2] */);

/* scaling tools (solver_socp.py:367-395).  These update the arrays only; the caller keeps
 * r / scale_z / const_d in dots_params consistent (dots_set_params). */
int dots_adjust_penalty(dots_ctx *ctx, double factor);             /* adjust_penalty :367-371: 5 dual arrays /= factor */
int dots_scale_z(dots_ctx *ctx, double z_mul, double beta_mul, double scale_z_new);
        /* scale_variable_z :373-395: z *= z_mul, beta *= beta_mul, mu = scale_z_new*(beta_fst-beta_end),
           E = -L^T(beta_mid; scale_z_new) */
int dots_scale_arrays(dots_ctx *ctx, uint32_t array_mask, double factor); /* x *= factor for every array in mask (scale_prim_dual :352-358) */

/* weighted squared norms norm_square_* (solver_socp.py:875-878, :215-218) of one state array,
 * and of dt_phi / dx_phi when array_id is DOTS_PHI with part = 1 / 2.
 * On a time slab: the slab's SHARE of the norm (the sum over its own nodes / intervals / corner entries divided by the
 * GLOBAL averaging count); the caller adds the shares of all slabs (is_constant_scaling, solver_socp.py:324-365).  part = 1
 * reads phi at the next slab's first node as the last solve (dots_slab_stage 3) left it.
 * The state is left as it is, but the call is treated as one that changes it: a pending penalty division is carried out, and the
 * carried gathers, the fused KKT sums, a right-hand side ahead and an armed penalty decision are dropped (dots_apply_operator does
 * the same).  DOTS_Z_MID: a z_mid left to be rebuilt is materialised; DOTS_ERR_STATE while z_mid is
 * unspecified (DOTS_STEP_SKIP_Z_MID). */
int dots_norm_square(dots_ctx *ctx, int array_id, int part, double *out);

/* ---- standalone operators (rows a4-a6 of SURVEY.md section 8a), host in / host out, for tests */
enum dots_operator {
    DOTS_OP_GRAD_TIME = 0,       /* (T+1,V)      -> (T,V)        solver_socp.py:881-884 */
    DOTS_OP_DIV_TIME,            /* (T,V)        -> (T+1,V)      :886-896 */
    DOTS_OP_GRAD_SPACE,          /* (T+1,V)      -> (T+1,F,3)    :898-907 */
    DOTS_OP_DIV_SPACE,           /* (T+1,F,3)    -> (T+1,V)      :909-921 */
    DOTS_OP_DECOUPLE,            /* (T+1,F,3)    -> (T,2,3,F,3)  :923-942 (scale) */
    DOTS_OP_DECOUPLE_ADJOINT,    /* (T,2,3,F,3)  -> (T+1,F,3)    :944-959 (scale) */
    DOTS_OP_TIME_AVG_ADJOINT,    /* (T,V)        -> (T+1,V)      :961-974 */
    DOTS_OP_LAPLACIAN_APPLY      /* (T+1,V)      -> (T+1,V)   x -> K x, the operator step 1 inverts (sign: K = -Laplacian + eps M) */
};
int dots_apply_operator(dots_ctx *ctx, int op, double scale, const double *in, int64_t n_in, double *out, int64_t n_out);

/* ---- multigrid preconditioner of the modal PCG (optional; Jacobi is used without it) ----------
 * Smoothed-aggregation hierarchy of the surface stiffness matrix, built on the host
 * (dots_socp_amd/multigrid.py).  Level l holds K_l and M_l on one CSR pattern, the prolongation P_l
 * (n_l x n_{l+1}) and its transpose; level 0 is the context's own K and vertex mass (pass NULL for
 * its rowptr/col/val_k/val_m).  coarse_inverse is (K_L + (sigma_a + eps) M_L)^-1 for every mode a,
 * stored [n_L][n_L][n_cols] (pseudo-inverse for a singular mode): it depends on eps, so call
 * dots_mg_setup again when eps changes. */
typedef struct dots_mg_level {
    int32_t n;                 /* rows of this level */
    int32_t nnz;               /* entries of the K/M pattern (0 for level 0) */
    const int32_t *rowptr;     /* [n+1] */
    const int32_t *col;        /* [nnz] */
    const double *val_k;       /* [nnz] */
    const double *val_m;       /* [nnz] */
    const double *diag_k;      /* [n] (level 0: may be NULL, taken from the context) */
    const double *diag_m;      /* [n] */
    int32_t n_coarse;          /* rows of the next level (0 on the coarsest) */
    int32_t p_nnz;
    const int32_t *p_rowptr;   /* [n+1]        P: n x n_coarse */
    const int32_t *p_col;
    const double *p_val;
    const int32_t *r_rowptr;   /* [n_coarse+1] R = P^T */
    const int32_t *r_col;
    const double *r_val;
    int32_t ap_nnz;            /* K P and M P (n x n_coarse) on one pattern: the post-smoothing kernel applies A P */
    int32_t reserved;
    const int32_t *ap_rowptr;  /* [n+1] */
    const int32_t *ap_col;
    const double *ap_val_k;
    const double *ap_val_m;
    const double *ap_val_p;    /* P itself on the pattern of A P (zero where P has no entry) */
} dots_mg_level;

typedef struct dots_mg_desc {
    int32_t n_levels;          /* >= 2 */
    int32_t n_cols;            /* modes the inverse is given for (= T+1 on one GPU) */
    double omega;              /* Jacobi damping of the smoother */
    const dots_mg_level *levels;
    const double *coarse_inverse;
} dots_mg_desc;

int dots_mg_setup(dots_ctx *ctx, const dots_mg_desc *desc);
int dots_mg_enable(dots_ctx *ctx, int on);   /* switch between multigrid (1) and Jacobi (0) preconditioning */

/* Test and diagnosis entry point; the product path never calls it.  Applies ONE V-cycle, with the launches and the tiling the PCG
 * uses, to a residual given on the host: r and z are [n_modes][V] in the caller's vertex numbering (the layout of phi), rz is
 * [n_modes], frozen is [n_modes] or NULL (non-zero: the mode counts as converged and is skipped; its z stays D^-1 r with
 * D = diag K + (sigma_a + eps) M, the state every cycle starts from, and its rz is 0).  On return z = MG(r) and
 * rz[a] = sum_i r[a][i] z[a][i] as the sum of the per-workgroup partial rows the next PCG kernel would re-reduce.  Uses the PCG's
 * vectors as scratch: a later solve is unaffected.  dots_mg_enable does not bear on it: the cycle of the installed hierarchy runs
 * also while the PCG is switched to Jacobi.  DOTS_ERR_STATE unless the context is DOTS_LAP_MODAL_PCG on one GPU (no time
 * slab) with a hierarchy installed by dots_mg_setup. */
int dots_mg_apply(dots_ctx *ctx, const double *r, double *z, double *rz, const int32_t *frozen);

/* Windowed modal PCG: long horizons without a factor (opt-in; off when a context is created).  The PCG kernels keep their per-mode
 * scalars for 256 modes, so a DOTS_LAP_MODAL_PCG context of T + 1 > 256 is refused by dots_step, dots_run_phase(LAPLACIAN) and
 * dots_mg_setup unless a factor is installed and enabled.  With on = 1 such a context solves step 1 without a factor: the T + 1
 * independent modal problems are taken in windows of 256 -- window k = modes [256 k, 256 k + 256) -- one after the other on the
 * context's stream, each through the PCG kernels at pitch 256 with its own hipGraph, first-burst size and (with multigrid) block of
 * the coarse inverse; the time transforms around them keep mode space compact (window k of a PCG vector is the [V][256] array at
 * offset k * V * 256).  dots_mg_setup then takes n_cols = T + 1 and one coarse inverse [n_L][n_L][T + 1] as below 256.  In
 * dots_step_stats cg_last_iterations is the maximum over the windows, cg_iterations adds that maximum, cg_not_converged counts a
 * solve once if any window hit the cap and cg_last_rel_residual is the worst window's.  An installed and enabled factor keeps
 * precedence: the sweeps run as without the switch, bit for bit.  At T + 1 <= 256 the switch changes nothing.  Changing the
 * setting on a context of T + 1 > 256 releases an installed multigrid hierarchy (its layout belongs to the setting).  Refused
 * above 256 as before: dots_mg_apply, dots_bench_kernel 0-2, time slabs, dots_step_many / dots_laplacian_solve_many without a
 * factor.  DOTS_ERR_STATE on a time slab and on a context that is not DOTS_LAP_MODAL_PCG. */
int dots_pcg_windows(dots_ctx *ctx, int on);

/* ---- direct solve of the modal problems (replaces the T+1 SuperLU factorisations of
 * laplacian_inverse_socp.py:40-61 and their per-iteration triangular solves, :46-60) ----------------
 * Multifrontal Cholesky factor on one nested-dissection tree shared by all modes, built on the host
 * (dots_socp_amd/frontal.py).  Nodes are numbered children-before-parents.  Node p eliminates n[p]
 * separator vertices and touches b[p] boundary vertices of its ancestors; front_idx lists them
 * (separator first) from ioff[p]; its dense block F_p = [L_pp^-1 ; A_bs A_ss^-1], (n+b) x n per mode,
 * starts at row foff[p] of `values` ([n_entries][pitch], mode fastest).  pull0/pull1 (parallel to
 * front_idx) give the position of a front row in the boundary of child 0 / 1 (or -1).  level_nodes
 * lists the nodes by height, level_ptr delimits the heights.  With a factor installed and enabled,
 * step 1 runs the two triangular sweeps instead of the PCG. */
typedef struct dots_front_desc {
    int32_t n_nodes;
    int32_t n_levels;
    int32_t n_modes;             /* modes the factor is given for (= T+1 on one GPU, slab_count on a time slab) */
    int32_t pitch;               /* doubles per entry of values; must equal the context's mode pitch */
    int64_t n_front_rows;        /* length of front_idx, pull0, pull1 */
    int64_t n_entries;           /* rows of values = sum over nodes of (n+b)*n */
    int64_t update_rows;         /* sum of b */
    const int32_t *node_n;
    const int32_t *node_b;
    const int64_t *node_foff;
    const int64_t *node_ioff;
    const int64_t *node_uoff;    /* first row of node p's update vector */
    const int32_t *node_child;   /* [n_nodes][2], -1 = none */
    const int32_t *front_idx;    /* device vertex numbering */
    const int32_t *pull0;
    const int32_t *pull1;
    const int32_t *level_ptr;    /* [n_levels+1] */
    const int32_t *level_nodes;  /* [n_nodes] */
    const double *values;        /* the factor, or NULL: factorise K + (sigma_a + eps) M on the device (eps from dots_params) */
    const int32_t *grounded;     /* [n_modes] 1: the mode's operator is singular (its last root pivot is grounded);
                                    read when values == NULL */
    const int32_t *band_ptr;     /* [n_bands+1] or NULL: tree heights [band_ptr[k], band_ptr[k+1]) are handled by ONE launch
                                    per sweep (0 = band_ptr[0] < ... < band_ptr[n_bands] = n_levels, at most 4 heights per
                                    band): the nodes of a band that hang together are merged into one block, computed on
                                    the device from the factor (csrc/kernels_front.hip).  NULL: one launch per height */
    int32_t n_bands;
    int32_t top_inverse;         /* 1: the nodes of the top band (they have no boundary rows) store the explicit inverse
                                    S^-1 = L'^-T L'^-1 of their merged block: the forward launch of that band writes the
                                    solution itself and the backward sweep starts one band lower (one launch less per solve;
                                    pays on small meshes, where the top band is a few hundred rows) */
} dots_front_desc;

/* DOTS_ERR_MEMORY (nothing allocated, the context stays usable with the PCG): the factor, the copy of the fronts and the Schur
 * complements the numeric factorisation needs beside it, and the per-corner sums of DOTS_STEP_CARRY exceed the free device memory
 * (hipMemGetInfo; DOTS_MEM_BUDGET=<MB> overrides what counts as available).  dots_last_error() names the sizes. */
int dots_front_setup(dots_ctx *ctx, const dots_front_desc *desc);

/* Host-side helpers for dots_front_desc (no device work; the Python reference implementations are in
 * dots_socp_amd/frontal.py).
 * dots_tree_build: geometric nested dissection of the graph (CSR pattern of K, 0-based) of `n_vertices` points
 * `xyz` [V][3]: subsets are cut at the median of their longest bounding-box side (principal axis above 512
 * vertices), the separator is the smaller one-sided vertex boundary of the cut, subsets of <= `leaf` vertices
 * become leaves.  Nodes are numbered children first; copy out with dots_tree_copy: order [V] (vertex eliminated
 * at position k), sep_ptr [n+1], child [n][2], parent [n], height [n].
 * dots_symbolic_build: boundary sets of the tree on the graph given in the numbering `order` refers to:
 * node_b [n], and per front row (separator rows first; dots_symbolic_front_rows of them) front_idx, pull0, pull1. */
/* dots_assemble: the operator assembly of utils/surface_pre_computations_socp.py:11-132 / solver_socp.py:102-113 for the mesh
 * (xyz [V][3], tri [F][3]) on the host: area [F], hat gradients [F][3][3], vertex masses [V], vertex -> corner lists
 * (cptr [V+1], cidx [3F], corners of a vertex ordered by the reference's corner index k F + f) and K = G^T diag(area) G as a
 * sorted CSR (rowptr [V+1], col / val [dots_assemble_nnz]): the arrays dots_problem_desc takes. */
typedef struct dots_mesh_ops dots_mesh_ops;
int dots_assemble(int32_t n_vertices, int32_t n_triangles, const double *xyz, const int32_t *tri, dots_mesh_ops **out);
int64_t dots_assemble_nnz(const dots_mesh_ops *ops);
int dots_assemble_copy(const dots_mesh_ops *ops, double *area, double *hat, double *mass, int32_t *cptr, int32_t *cidx, int32_t *rowptr, int32_t *col, double *val);
void dots_assemble_free(dots_mesh_ops *ops);
/* dots_patch_order: recursive coordinate bisection of the points `xyz` [V][3] (longest side of the bounding box, cut at a
 * multiple of `unit`, leaves of <= unit points, siblings adjacent): order [V]. */
int dots_patch_order(int32_t n_vertices, const double *xyz, int32_t unit, int32_t *order);
typedef struct dots_tree dots_tree;
typedef struct dots_symbolic dots_symbolic;
int dots_tree_build(int32_t n_vertices, const int32_t *indptr, const int32_t *indices, const double *xyz, int32_t leaf, dots_tree **out);
int64_t dots_tree_nodes(const dots_tree *tree);
int dots_tree_copy(const dots_tree *tree, int64_t *order, int64_t *sep_ptr, int32_t *child, int32_t *parent, int32_t *height);
void dots_tree_free(dots_tree *tree);
int dots_symbolic_build(int32_t n_vertices, const int32_t *indptr, const int32_t *indices, int64_t n_nodes, const int64_t *order,
                        const int64_t *sep_ptr, const int32_t *child, dots_symbolic **out);
int64_t dots_symbolic_front_rows(const dots_symbolic *sym);
int dots_symbolic_copy(const dots_symbolic *sym, int32_t *node_b, int32_t *front_idx, int32_t *pull0, int32_t *pull1);
void dots_symbolic_free(dots_symbolic *sym);
int dots_front_enable(dots_ctx *ctx, int on);
/* Several problems on one surface, one factor.  dots_front_share installs the factor of `owner` in `ctx`: the factor, its descriptors and
 * maps are shared (reference-counted: they are freed with the last context that holds them, so the owner may be destroyed first);
 * `ctx` allocates only what one solve writes (its update planes and the carried gathers of DOTS_STEP_CARRY).  DOTS_ERR_ARGUMENT unless
 * both contexts are on one device with the same V, F, T, Laplacian entries, mode pitch and the eps the factor was built with (the
 * caller guarantees the same mesh in the same vertex numbering); DOTS_ERR_STATE when the owner has no factor or either is a time slab.
 * dots_laplacian_solve_many: step 1's operator inverse (the transforms to and from the time modes and the two sweeps) of host_in[k]
 * into host_out[k], both [T+1][V] in the reference layout, for the n contexts cs[k] that share one factor; the sweeps of all of them
 * run as ONE sequence of launches that reads each factor entry once for up to 4 right-hand sides (DOTS_FRONT_NR = 2 / 4 / 8 overrides),
 * every result bit for bit what a call with n = 1 on that context computes.  Uses the solve's scratch of every context (waits for each
 * context's stream; returns when the results are on the host).  DOTS_ERR_STATE for a context without an installed or shared factor,
 * a time slab or a PCG context. */
int dots_front_share(dots_ctx *ctx, dots_ctx *owner);
int dots_laplacian_solve_many(dots_ctx *const *ctxs, int n, const double *const *host_in, double *const *host_out);
/* One ALM iteration of each of the n contexts ctxs[k] that share one factor, each under the step flags set on it (dots_step_flags:
 * DOTS_STEP_SKIP_Z_MID, _PALM, _CARRY, _KKT_SUMS; DOTS_STEP_RHS_AHEAD and DOTS_STEP_TIMED are ignored in a batch): each member's launches before
 * the solve on its own stream, ONE batched pair of sweeps for all of them (on the stream of ctxs[0], ordered by events), each member's
 * launches after the solve on its own stream again.  Every member ends bit for bit where dots_step(ctx, 1, NULL) would have left it, and
 * calls on its own stream afterwards (KKT read-back, download, scaling) see its results.  stats != NULL: the host waits, and the batch's
 * phases as a whole are returned (ms_rhs: first halves and forward transforms, ms_laplacian: the sweeps, ms_q_lambda_multiplier: the rest
 * with the projections; alm_iterations = n).  dots_penalty_ahead on a context stepped in a batch returns DOTS_ERR_STATE until its next
 * dots_step.  DOTS_ERR_STATE for a context without an installed or shared factor, a time slab or a PCG context.
 * dots_bench_many: the batched sweeps alone, `reps` times on whatever the contexts' solve buffers hold, timed by events on ctxs[0]'s
 * stream (milliseconds per batched solve). */
int dots_step_many(dots_ctx *const *ctxs, int n, dots_step_stats *stats);
int dots_bench_many(dots_ctx *const *ctxs, int n, int reps, double *ms_per_solve);
/* ---- coarse-to-fine time cascade: the state of one context on the time grid of another (init_solution, solver_socp.py:38,70-71,
 * 239-250, without the round trip over the host) -----------------------------------------------------------------------------
 * dots_prolong_time fills the twelve state arrays of `dst` with those of `src` interpolated linearly in time: destination
 * time point t of an array takes (1 - w[t]) * (f * a[j[t]]) + w[t] * (f * a[j[t] + 1]) of the same row of `src` (a[j + 1] reads a[j]
 * where the source has one point only), with f the array's factor below (the source's scaled iterate -> the recovered solution,
 * solver_socp.py:397-405; pass 1 to copy the iterate as it is).  Node arrays (phi, B, E) use the node tables, every other array the
 * interval tables; the corner arrays are interpolated along the interval index.  The tables come from the caller
 * (dots_socp_amd/cascade.py: time_weights), so that the result is bit for bit what dots_upload of the same interpolation done on
 * the host in these operations leaves.  Both contexts hold the same mesh on one device, possibly in different device numberings:
 * vmap / fmap give the source row of every destination vertex / triangle (NULL = the same numbering; corner k of a triangle is the
 * same in both).
 * On `src` a pending penalty division is carried out and z_mid is materialised first (DOTS_ERR_STATE if z_mid is stale: the last
 * step ran with DOTS_STEP_SKIP_Z_MID); `dst` is left as twelve dots_upload calls leave it (carried sums, fused KKT sums and a launch
 * ahead dropped), ready for dots_step.  The two streams are ordered by events; the call returns when the destination is filled.
 * DOTS_ERR_ARGUMENT: different V or F, dst == src, a NULL table, a table or map entry out of range; DOTS_ERR_STATE: a time slab,
 * contexts on different devices. */
typedef struct dots_prolong_desc {
    const int32_t *node_j;       /* [T_dst + 1] source node j of every destination node, 0 <= j <= max(T_src - 1, 0)      */
    const double *node_w;        /* [T_dst + 1] weight of source node j + 1, in [0, 1]                                    */
    const int32_t *interval_j;   /* [T_dst]     source interval j of every destination interval, 0 <= j <= max(T_src - 2, 0) */
    const double *interval_w;    /* [T_dst]                                                                               */
    const int32_t *vmap;         /* [V] destination vertex row -> source vertex row, or NULL                              */
    const int32_t *fmap;         /* [F] destination triangle row -> source triangle row, or NULL                          */
    double factor[4];            /* applied to the source values of: phi, A, B, lambda_c / z_fst, z_mid, z_end / mu, E /
                                    beta_fst, beta_mid, beta_end                                                          */
    double *ms;                  /* NULL, or out: milliseconds of the launches on the device (events on dst's stream)     */
} dots_prolong_desc;
int dots_prolong_time(dots_ctx *dst, dots_ctx *src, const dots_prolong_desc *desc);

/* ---- coarse-to-fine cascade in space: the state of a context on the nested refinement of its mesh -----------------------------
 * dots_prolong_space fills the twelve state arrays of `dst` (the refined mesh) from those of `src` (its parent mesh), both on one
 * time grid and one device: a vertex row of `dst` takes f * a where its two source rows are one (a kept vertex: a copy of the
 * recovered value), else (f * a + f * b) * 0.5 (an edge midpoint); a row of a triangle array (B, E) takes f times the row of the same
 * component of the parent triangle (not projected into the child's plane); a row of a corner array (z_mid, beta_mid) f times the
 * parent's row of the same corner, interval end and component.  f is the array's factor, as for dots_prolong_time.  The row maps
 * come from the caller (dots_socp_amd/cascade.py: space_row_maps, from meshes.subdivide's parents and the device numberings of the
 * two contexts), so that the result is bit for bit what dots_upload of the host's prolongation (cascade.prolong_space) leaves.
 * `src` and `dst` are treated as by dots_prolong_time (pending division, z_mid, what `dst` carried; stream order; the call returns
 * when the destination is filled).
 * DOTS_ERR_ARGUMENT: different n_time, dst == src, a NULL map, n_vertices / n_triangles that are not the destination's V / F, a map
 * entry that is no row of the source; DOTS_ERR_STATE: a time slab, contexts on different devices, a stale z_mid.  After an error
 * both contexts are as they were. */
typedef struct dots_prolong_space_desc {
    const int32_t *vmap;         /* [n_vertices][2] destination vertex row -> its two source vertex rows (equal: a copy)  */
    const int32_t *fmap;         /* [n_triangles]   destination triangle -> source triangle (corner k stays corner k)       */
    int32_t n_vertices;          /* entries of the maps: V and F of `dst`                                                  */
    int32_t n_triangles;
    double factor[4];            /* as dots_prolong_desc.factor                                                            */
    double *ms;                  /* NULL, or out: milliseconds of the launches on the device (events on dst's stream)     */
} dots_prolong_space_desc;
int dots_prolong_space(dots_ctx *dst, dots_ctx *src, const dots_prolong_space_desc *desc);

/* ---- cascade in space between two independent triangulations of one surface: barycentric transfer -----------------------------
 * dots_transfer_space fills the twelve state arrays of `dst` from those of `src`, a context on ANOTHER triangulation of the same
 * surface (no nesting, no `parents`), both on one time grid and one device.  It replaces the round trip over the host of a warm
 * start on a mesh that is not a subdivision of the coarse one (init_solution, solver_socp.py:38,70-71, 239-250, filled from
 * cascade.transfer_space_solution): a vertex row of `dst` takes (w0 * (f * a0) + w1 * (f * a1)) + w2 * (f * a2) of its three source
 * vertex rows, in this order of operations and with no special case for weights 0 or 1; a row of a triangle array (B, E) f times
 * the row of the same component of the source triangle fsrc[f'] (not projected into the destination triangle's plane); a row of a
 * corner array (z_mid, beta_mid) f times the row of corner csrc[f'][k] of that triangle, same interval end and component.  f is the
 * array's factor, as for dots_prolong_time.  The tables come from the caller (dots_socp_amd/cascade.py: mesh_transfer locates every
 * destination vertex and triangle centroid on the source mesh, transfer_row_maps puts the result into the device numberings of the
 * two contexts), so that the result is bit for bit what dots_upload of the host's transfer (cascade.transfer_space) leaves.
 * `src` and `dst` are treated as by dots_prolong_time (pending division, z_mid, what `dst` carried; stream order; the call returns
 * when the destination is filled).
 * DOTS_ERR_ARGUMENT: different n_time, dst == src, a NULL table, n_vertices / n_triangles that are not the destination's V / F, a
 * vsrc / fsrc entry that is no row of the source, a csrc entry outside 0 .. 2, a weight that is negative or not finite;
 * DOTS_ERR_STATE: a time slab, contexts on different devices, a stale z_mid.  After an error both contexts are as they were. */
typedef struct dots_transfer_space_desc {
    const int32_t *vsrc;         /* [n_vertices][3] destination vertex row -> its three source vertex rows                 */
    const double *vw;            /* [n_vertices][3] their weights: finite, >= 0                                            */
    const int32_t *fsrc;         /* [n_triangles]   destination triangle -> source triangle                                */
    const int32_t *csrc;         /* [n_triangles][3] corner k of the destination triangle -> corner 0 .. 2 of fsrc         */
    int32_t n_vertices;          /* entries of the tables: V and F of `dst`                                                */
    int32_t n_triangles;
    double factor[4];            /* as dots_prolong_desc.factor                                                            */
    double *ms;                  /* NULL, or out: milliseconds of the launches on the device (events on dst's stream)     */
} dots_transfer_space_desc;
int dots_transfer_space(dots_ctx *dst, dots_ctx *src, const dots_transfer_space_desc *desc);

/* ---- cascade in space and time at once: the state of a context on another mesh AND another time grid ---------------------------
 * dots_carry_spacetime fills the twelve state arrays of `dst` from those of `src`, a context on the parent mesh of `dst`'s (vw NULL:
 * the formulas of dots_prolong_space) or on another triangulation of the same surface (vw given: those of dots_transfer_space), with
 * ANOTHER n_time, on one device.  Space first, then time: every row of `dst` is formed on the source's time grid as the carrier in
 * space forms it (f applied to the source values first), and that row is then interpolated linearly in time as dots_prolong_time
 * does with a factor of 1: time point t takes (1 - w[t]) * x[j[t]] + w[t] * x[j[t] + 1].  The row on the source's time grid exists
 * in on-chip memory only: no third context, one pass over the state.  The tables come from the caller (dots_socp_amd/cascade.py:
 * time_weights, and space_row_maps or transfer_row_maps in the device numberings of the two contexts), so that the result is bit for
 * bit what dots_upload of cascade.carry_spacetime leaves.  `src` and `dst` are treated as by dots_prolong_time (pending division,
 * z_mid, what `dst` carried; stream order; the call returns when the destination is filled).
 * DOTS_ERR_ARGUMENT: the SAME n_time (use dots_prolong_space / dots_transfer_space: on one grid they are the definition), dst == src,
 * a NULL time table, vsrc or fsrc, n_vertices / n_triangles that are not the destination's V / F, a time-table entry out of range,
 * a vsrc / fsrc entry that is no row of the source, a csrc entry outside 0 .. 2, a weight that is negative or not finite;
 * DOTS_ERR_STATE: a time slab, contexts on different devices, a stale z_mid.  After an error both contexts are as they were. */
typedef struct dots_carry_spacetime_desc {
    const int32_t *node_j;       /* the four time tables, as in dots_prolong_desc                                          */
    const double *node_w;
    const int32_t *interval_j;
    const double *interval_w;
    const int32_t *vsrc;         /* vw NULL: [n_vertices][2] the two source vertex rows (equal: a copy), as dots_prolong_space_desc.vmap;
                                    else [n_vertices][3] the three source vertex rows, as dots_transfer_space_desc.vsrc     */
    const double *vw;            /* NULL (nested), or [n_vertices][3] the weights: finite, >= 0                            */
    const int32_t *fsrc;         /* [n_triangles]   destination triangle -> source triangle                                */
    const int32_t *csrc;         /* NULL (corner k stays corner k), or [n_triangles][3] corner k -> corner 0 .. 2 of fsrc  */
    int32_t n_vertices;          /* entries of the tables in space: V and F of `dst`                                       */
    int32_t n_triangles;
    double factor[4];            /* as dots_prolong_desc.factor                                                            */
    double *ms;                  /* NULL, or out: milliseconds of the launches on the device (events on dst's stream)     */
} dots_carry_spacetime_desc;
int dots_carry_spacetime(dots_ctx *dst, dots_ctx *src, const dots_carry_spacetime_desc *desc);

/* ---- read-out of the transport: what the solver plug-ins return (mu, E), formed on the device ---------------------------------
 * dots_readout delivers mu and / or E as dots_download would (reference layouts, the caller's numbering), every value multiplied
 * first by `factor` (the recovered solution, solver_socp.py:397-405: r * dual_scale; 1 = the iterate) and then, where weights are
 * given, by the weight of its vertex / triangle (translate_solution_socp_to_dot, utils/type.py:48-65: area_v / 3 and area_t) --
 * these operations in this order, so that the result equals the host's bit for bit (dots_socp_amd/readout.py: read_out_host).
 * centred: mu on the time-centred grid (socp/solver_decorator.py:29-54): T + 1 layers, mu0, 0.5 * (a_l-1 + a_l) for l = 1 .. T - 1
 * of the T weighted layers a, mu1.  layer_mass / layer_negative: the sum over the vertices of every layer of mu as written, and of
 * its negative entries (utils/evaluate_solution.py:7-45), formed on the device in a fixed order (the same run to run); they may be
 * asked for without mu.  Only what is asked for crosses to the host.
 * A pending penalty division is carried out first, as for a download; z_mid is neither needed nor produced (the call succeeds after
 * a DOTS_STEP_SKIP_Z_MID step); the state, carried sums, fused KKT sums and a launch ahead are left as they are.  Works on contexts
 * of every Laplacian solver and on members of a batch (on their own stream).
 * The outputs are formed in the context's staging buffer (18 F pitch doubles, the size of z_mid) together with the weights, end
 * points and partial sums: (T + 1) 3 F + (T + 1) V + 3 V + F + 2 (T + 1) V / 30 doubles must fit, which holds for every mesh with
 * fewer than about 14 vertices per triangle (a closed surface has 1 / 2).
 * DOTS_ERR_ARGUMENT: NULL desc, centred without mu0 / mu1 (whatever is asked for), nothing asked for; DOTS_ERR_STATE: a time slab,
 * a mesh whose outputs do not fit the staging buffer (dots_download still works). */
typedef struct dots_readout_desc {
    double factor;              /* first multiplier of every value (r * dual_scale for the recovered mu, E; 1 = the iterate) */
    const double *w_vertex;     /* host [V], caller numbering, or NULL: second multiplier of mu (area_v / 3) */
    const double *w_triangle;   /* host [F] or NULL: second multiplier of E (area_t) */
    int32_t centred;            /* 0: mu as stored, T layers; 1: T + 1 layers mu0, 0.5 (a_l + a_l+1), mu1 */
    int32_t reserved;
    const double *mu0, *mu1;    /* host [V], caller numbering; required when centred */
    double *mu;                 /* host out [layers][V], or NULL */
    double *E;                  /* host out [T+1][F][3], or NULL */
    double *layer_mass;         /* host out [layers] or NULL: sum over v of the layer as written */
    double *layer_negative;     /* host out [layers] or NULL: sum of its negative entries */
    double *ms;                 /* NULL, or out: device milliseconds of the launches */
} dots_readout_desc;
int dots_readout(dots_ctx *ctx, const dots_readout_desc *desc);

/* ---- flow map: particles traced through the transport on the device ------------------------------------------------------------
 * dots_flow_map moves n_particles points of the surface along the velocity E / mu of the state the context holds, from time 0 to
 * time 1, and returns where they end up (and, on request, where they are after every interval).  It extends what the reference
 * returns at solver_socp.py:855-869 (mu and E): the transport map is formed from them where they lie, and only a few numbers per
 * particle cross to the host instead of the two arrays.  dots_socp_amd/flow.py: flow_map_host is the specification, and the
 * outputs equal it bit for bit on the downloaded mu and E.
 * A particle is a triangle and three barycentric weights.  In interval j = 0 .. T - 1 (length h = 1 / T) it moves with the
 * velocity u = 0.5 (E[j] + E[j + 1]) / rho of the triangle it is in -- E lives on the nodes, mu on the intervals; rho = the mean
 * of mu[j] over the triangle's vertices, and u = 0 where rho <= floor (or is not a number) -- through the rates hat_grad . u of
 * its weights (the hat gradients of dots_problem_desc; only the tangential part of u enters).  Where a weight reaches 0 before
 * the interval ends the particle crosses the edge opposite that corner into `neighbours` and goes on with the time that is left.
 * On a boundary edge (-1) it stops for good (status 1).  After max_crossings crossings in one interval it rests on the edge until
 * the next interval (`rested` counts these; two triangles that push a particle at each other).  Weights are never renormalised.
 * Particles are taken and returned in the CALLER's triangle numbering; corners keep their index in every numbering.
 * `floor` is in the units of the iterate as stored: mu and E share one recovery factor and only their ratio is used.
 * A pending penalty division is carried out first, as for a download; z_mid is neither needed nor produced (the call succeeds after
 * a DOTS_STEP_SKIP_Z_MID step); the state, carried sums, fused KKT sums and a launch ahead are left as they are.  Works on contexts
 * of every Laplacian solver, at every n_time + 1 <= 1024, and on members of a batch (on their own stream).  One launch of
 * ceil(n_particles / 256) workgroups, one lane per particle; only the outputs cross to the host (counted in dots_debug_counter 9).
 * DOTS_ERR_ARGUMENT (nothing launched): NULL desc or a NULL required pointer, n_particles < 1, a start triangle or a neighbour
 * index out of range, a neighbour entry that does not share the edge opposite its corner, a weight that is negative or not finite,
 * max_crossings outside 1 .. 255, a floor that is not a number; DOTS_ERR_STATE: a time slab. */
typedef struct dots_flow_map_desc {
    int32_t n_particles;
    int32_t max_crossings;          /* 1 .. 255: crossings per interval before the particle rests                       */
    const int32_t *start_triangle;  /* host [n_particles], caller numbering                                             */
    const double *start_weights;    /* host [n_particles][3]: finite, >= 0                                              */
    const int32_t *neighbours;      /* host [F][3], caller numbering: the triangle across the edge opposite corner k
                                       (the edge between corners (k + 1) % 3 and (k + 2) % 3), -1 on a boundary edge    */
    double floor;                   /* densities up to this one carry no velocity                                       */
    int32_t *triangle;              /* host out [n_particles]                                                           */
    double *weights;                /* host out [n_particles][3]                                                        */
    int32_t *status;                /* host out [n_particles]: 0, or 1 stopped at a boundary edge                       */
    int32_t *rested;                /* host out [n_particles]: intervals cut short at max_crossings                     */
    int32_t *crossings;             /* host out [n_particles]: edges crossed in all                                     */
    int32_t *triangles_at;          /* NULL, or host out [T + 1][n_particles]: layer 0 the start, layer l after l intervals */
    double *weights_at;             /* NULL, or host out [T + 1][n_particles][3]                                        */
    double *ms;                     /* NULL, or out: device milliseconds of the launch                                  */
} dots_flow_map_desc;
int dots_flow_map(dots_ctx *ctx, const dots_flow_map_desc *desc);

/* dots_flow_push: the trace of dots_flow_map, and what the particles carry summed onto the vertices on the device -- the push-forward
 * of a mass (compare its last layer with mu1), the Lagrangian interpolation at every time node, an attribute carried along.
 * dots_socp_amd/flow.py: push_forward_host is the specification, and mass_at / attr_at / dropped equal it bit for bit.
 * Channels: c = 0 the mass, c = 1 .. A the attributes.  Particle p carries g[p][0] = mass[p] and g[p][c] = mass[p] *
 * attributes[c - 1][p]; every g must be finite.  Layers: all_layers = 0 gives L = 1, the state after interval T; otherwise
 * L = T + 1, the layers of triangles_at.  At each layer, for each corner k of the triangle f the particle is in and each channel:
 * x = g * l_k, y = x * 2^k_c with k_c = scale_exponent[c]; if |y| < 2^62 is false (a NaN included) the contribution is dropped and
 * counted in `dropped`; otherwise q = rint(y) (to nearest even) is added to a 64-bit integer of (c, layer, vertex k of f) in two's
 * complement -- integer addition is associative: the sums are the same bits for every order of arrival, order of the particles and
 * launch shape; two calls with the same exponents add exactly.  Stopped and resting particles keep depositing where they are.  The
 * result is (double)sum * 2^-k_c in the CALLER's vertex numbering.  The caller chooses the exponents (flow.push_scales:
 * 2^(60 - k_c) >= B_c = sum over p of |g[p][c]| max(1, (w0 + w1) + w2) of the start weights); the call refuses an exponent outside
 * -1000 .. 1000 and one with B_c 2^k_c > 2^61 in its own summation.
 * `map` is checked as dots_flow_map checks it, except that its five per-particle outputs may be NULL (those given are filled, and
 * equal dots_flow_map's); the contract of dots_flow_map holds (pending penalty division, z_mid, state left alone, every Laplacian
 * solver and n_time + 1 <= 1024, batch members on their own stream).  The accumulators ((1 + A) L V 64-bit words) are allocated and
 * zeroed per call: DOTS_ERR_MEMORY when they do not fit, the context stays usable.  Three launches: the zeroing, the trace with
 * its deposits (one no-return 64-bit integer atomic per non-zero q), the conversion; `ms` (and map.ms) cover them.  The output
 * bytes are counted in dots_debug_counter 9.
 * DOTS_ERR_ARGUMENT (nothing launched): what dots_flow_map refuses; NULL mass, scale_exponent or mass_at; n_attributes outside
 * 0 .. 4; NULL attributes or attr_at with n_attributes > 0; a g that is not finite; an exponent as above.  DOTS_ERR_STATE: a time slab. */
typedef struct dots_flow_push_desc {
    dots_flow_map_desc map;         /* the particles and the trace; triangle, weights, status, rested, crossings may be NULL */
    const double *mass;             /* host [n_particles]                                                               */
    int32_t n_attributes;           /* A, 0 .. 4                                                                        */
    int32_t all_layers;             /* 0: L = 1, the state after interval T; else L = T + 1                             */
    const double *attributes;       /* host [A][n_particles], NULL iff A = 0                                            */
    const int32_t *scale_exponent;  /* host [1 + A]: k_c, -1000 .. 1000                                                 */
    double *mass_at;                /* host out [L][V]                                                                  */
    double *attr_at;                /* host out [A][L][V], NULL iff A = 0                                               */
    int64_t *dropped;               /* NULL, or out: contributions that were dropped                                    */
    double *ms;                     /* NULL, or out: device milliseconds of the three launches                          */
} dots_flow_push_desc;
int dots_flow_push(dots_ctx *ctx, const dots_flow_push_desc *desc);

/* dots_flow_trace: the trace of dots_flow_map between any two time nodes, in either direction, with the kinetic action of every
 * particle and, on request, the deposits of dots_flow_push.  dots_socp_amd/flow.py: flow_map_host(..., span, action) and
 * push_forward_host are the specification, and every output equals them bit for bit.
 * n = |node_to - node_from| intervals are traversed: forward (node_to > node_from) j = node_from + i, backward j = node_from - 1 - i,
 * i = 0 .. n - 1.  The steps are those of dots_flow_map in the interval j; backward the velocity is negated, u = -(0.5 (E[j] +
 * E[j + 1]) / rho) (a floored triangle has u = +0 in both directions), which gives the inverse map: a source point for every start
 * on the target.  Every step of a particle adds best * ((u0 u0 + u1 u1) + u2 u2) to its action, `best` the time the step took (a
 * step that ends in a stop or a rest has still spent it) and u as formed (nothing is projected): the time integral of |u|^2 along
 * the path.  Layer i of triangles_at / weights_at is the state after i traversed intervals: n + 1 layers.  With (0, n_time) and a
 * NULL action the outputs equal dots_flow_map's and dots_flow_push's.
 * mass NULL: no deposits, the deposit fields are ignored and the five per-particle outputs of `map` are required.  Otherwise the
 * deposits of dots_flow_push on the layers of this trace: all_layers = 0 gives L = 1, the state at node_to; else L = n + 1.
 * The contract of dots_flow_map / dots_flow_push holds (pending penalty division, z_mid, state left alone, every Laplacian solver
 * and n_time + 1 <= 1024, batch members on their own stream; output bytes in dots_debug_counter 9); the same launches, and the same
 * kernels (k_flow_trace, k_flow_trace_push<A>): dots_flow_map and dots_flow_push are this trace over (0, n_time).
 * DOTS_ERR_ARGUMENT (nothing launched, the context stays usable): what dots_flow_map / dots_flow_push refuse; a node outside
 * 0 .. n_time; node_from == node_to.  DOTS_ERR_STATE: a time slab. */
typedef struct dots_flow_trace_desc {
    dots_flow_map_desc map;         /* the particles and per-particle outputs; triangles_at / weights_at are [n + 1] layers   */
    int32_t node_from, node_to;     /* 0 .. n_time, different                                                            */
    double *action;                 /* NULL, or host out [n_particles]                                                   */
    const double *mass;             /* NULL: no push; else host [n_particles] and the fields below as in dots_flow_push_desc */
    int32_t n_attributes;
    int32_t all_layers;             /* 0: L = 1, the state at node_to; else L = n + 1                                    */
    const double *attributes;
    const int32_t *scale_exponent;
    double *mass_at;                /* host out [L][V]                                                                   */
    double *attr_at;                /* host out [A][L][V], NULL iff A = 0                                                */
    int64_t *dropped;
    double *ms;                     /* NULL, or out: device milliseconds of the launches (map.ms is filled too)          */
} dots_flow_trace_desc;
int dots_flow_trace(dots_ctx *ctx, const dots_flow_trace_desc *desc);

/* dots_flow_slide: dots_flow_trace with the sliding mode of the discontinuous velocity field.  dots_socp_amd/flow.py:
 * flow_map_host(..., span, action, slide=True, areas) and push_forward_host are the specification, and every output equals them
 * bit for bit.
 * Where the triangle a particle has just entered pushes it back across the edge it came through (the rate of the weight of the
 * corner opposite that edge is negative), dots_flow_trace crosses back and forth in zero time until max_crossings and rests for
 * what is left of the interval.  Here the particle moves ALONG the edge instead, with the convex combination of the two
 * velocities whose normal component vanishes (Filippov): s = (mG sP + mP sG) / (mP + mG), sP and sG the two triangles' rates of
 * the weight of one end of the edge with the velocity projected onto the edge, mP and mG their normal speeds times their areas
 * (the context's triangle areas).  The slide lasts until the interval ends or a vertex is reached; there the triangle either
 * passes the particle on round the fan (an ordinary exit with no time spent) or, if it does not, the particle rests at the
 * vertex (`rested`).  A slide counts towards max_crossings within its interval but not in `crossings`; its action is the time
 * spent times the squared speed along the edge.  flow.py states the steps in their order of operations.
 * slides: the slides of every particle; steps: the turns of its inner loop (one per stretch of straight motion or slide).
 * Everything else is dots_flow_trace: the span in either direction, the action, the deposits (trace.mass), the layers; the same
 * contract (pending penalty division, z_mid, state left alone, every Laplacian solver and n_time + 1 <= 1024, batch members on
 * their own stream; output bytes in dots_debug_counter 9: 4 more per particle, 8 with steps); the tracer's other kernel family
 * (k_flow_slide, k_flow_slide_push<A>), the same launches.
 * DOTS_ERR_ARGUMENT (nothing launched, the context stays usable): what dots_flow_trace refuses; a NULL slides.
 * DOTS_ERR_STATE: a time slab. */
typedef struct dots_flow_slide_desc {
    dots_flow_trace_desc trace;     /* everything dots_flow_trace takes and returns                                      */
    int32_t *slides;                /* host out [n_particles], required                                                  */
    int32_t *steps;                 /* NULL, or host out [n_particles]: turns of the inner loop                          */
} dots_flow_slide_desc;
int dots_flow_slide(dots_ctx *ctx, const dots_flow_slide_desc *desc);

/* ---- cost gradients: the potentials at the two ends and the stress of the kinetic energy, reduced on the device ------------------
 * dots_sensitivity returns what the derivative of the transport cost is made of, from the state the context holds, in the caller's
 * numbering (dots_socp_amd/sensitivity.py: potentials_host and stress_host are the specification, and every output equals them bit for
 * bit on the downloaded phi and mu):
 *   phi0[v] = factor_phi * phi[0][v], phiT[v] = factor_phi * phi[n_time][v]: the Kantorovich potential at the two ends, as stored (the
 *     caller fixes the gauge); the cost's derivative in the end masses is -(phi0 - mean) and phiT - mean.
 *   stress[f][k][e], e over the entries (a, b) = 00, 01, 02, 11, 12, 22 of a symmetric 3 x 3 tensor per corner k of triangle f (vertex
 *     v_k = tri[f][k]; corners keep their index in every numbering):
 *       sum over t = 0 .. n_time - 1 of (mu[t][v_k] * mass[v_k]) * 0.5 * (p_t[a] p_t[b] + p_t+1[a] p_t+1[b]),  p_t[a] = phi[t][tri[f][a]],
 *     with phi and mu multiplied by their factors first (one multiplication each; the recovered solution: prim_scale and
 *     r * dual_scale), one accumulator per entry, t ascending, in the order of operations stress_host states.  The discrete kinetic
 *     energy is linear in it, and minus its derivative in the vertex positions at fixed stress is the shape derivative of the cost
 *     without congestion (sensitivity.py: kinetic_energy).
 * One lane per caller vertex and one per caller triangle corner, plain loads and stores; 18 F + 2 V doubles leave the device instead
 * of phi and mu.  Without device_pointers the outputs are formed in the context's staging buffer and copied to the host (counted in
 * dots_debug_counter 9); with it they are written where the caller's device pointers say, and the call returns with the stream
 * synchronised, so that they may be read right away from any stream.
 * A pending penalty division is carried out first, as for a download; z_mid is neither needed nor produced; the state, carried sums,
 * fused KKT sums and a launch ahead are left as they are.  Works on contexts of every Laplacian solver and on members of a batch.
 * DOTS_ERR_ARGUMENT (nothing launched): NULL desc, nothing asked for (phi0, phiT and stress all NULL), a factor that is not finite,
 * a device stress pointer off a 16-byte boundary; DOTS_ERR_STATE: a time slab. */
typedef struct dots_sensitivity_desc {
    double factor_phi;           /* multiplier of every phi (prim_scale for the recovered solution; 1 = the iterate)            */
    double factor_mu;            /* multiplier of every mu (r * dual_scale; 1 = the iterate)                                    */
    const double *mass_vertex;   /* HOST [V], caller numbering (area_vertices / 3), or NULL: the context's own vertex masses    */
    double *phi0, *phiT;         /* out [V] each, or NULL                                                                       */
    double *stress;              /* out [F][3][6], or NULL                                                                      */
    int32_t device_pointers;     /* 0: phi0, phiT, stress are host addresses; 1: device addresses on the context's device      */
    int32_t reserved;
    double *ms;                  /* NULL, or HOST out: device milliseconds of the launches                                      */
} dots_sensitivity_desc;
int dots_sensitivity(dots_ctx *ctx, const dots_sensitivity_desc *desc);

/* ---- solve session: new end masses on a live context ---------------------------------------------------------------------------
 * dots_restart: the context takes the end masses mu0 / mu1 of another transport problem on the same surface and starts over, with
 * everything that does not depend on them kept: the factor (its own or a shared one: only this context's state changes), the
 * multigrid hierarchy, the PCG work arrays, the window setting (dots_pcg_windows), every allocation.  Nothing is rebuilt and nothing
 * crosses to the host.
 *   Boundary data: mu0 / mu1 replace the context's; norm_boundary is formed again.  From host arrays with the loop of dots_create: the
 *     bits of a new context.  With device_pointers the sum is a two-stage reduction on the device in a fixed order (every lane of up
 *     to 1024 workgroups adds its vertices in ascending order, the lanes of a workgroup fold in a fixed tree, one workgroup folds the
 *     workgroups' sums the same way): reproducible from call to call, but not the host loop's bits (the two agree to V roundings).  The caller's device arrays must be complete before the call (it reads them on the context's
 *     stream).
 *   Parameters: dots_params as dots_create leaves them -- r = scale_z = const_d = 1, prim / dual / boundary scale 1, congestion 0,
 *     norm_d as at creation --, except tau, eps, cg_tol and cg_max_iter, which are kept.
 *   DOTS_RESTART_COLD: a pending penalty division is dropped without being applied, the twelve state arrays (one launch of the same
 *     kernel family, stores only) and what is derived from them (the cone multiplier, the buffers written ahead, the PCG vectors and
 *     scalars) are zeroed: a new context's state.
 *   DOTS_RESTART_WARM: a pending penalty division is carried out and z_mid materialised, as for dots_download; then every element of
 *     array k is multiplied once by factors[group(k)] -- groups (phi, A, B, lambda_c), the z arrays, (mu, E), the beta arrays: the
 *     recovered solution (solver_socp.py:397-405) -- in place, in ONE launch (two time columns per lane, 16-byte accesses; the
 *     padding columns are zero afterwards).  The state then holds the bits that downloading the twelve arrays, multiplying them on the
 *     host and uploading them into a new context at r = 1 leaves.
 *   Both modes drop what belongs to the old run: a right-hand side enqueued ahead, an armed penalty decision, the carried gathers,
 *     the fused KKT sums, the step path, the step flags, the KKT halo flag, the mailbox sequence and the step-time ring (records not
 *     yet collected by dots_step_times are lost).
 * The call returns with the stream synchronised.  DOTS_ERR_ARGUMENT (the context is untouched): NULL desc or mass array, an unknown
 * mode, a host mass that is not finite, a WARM factor that is not finite and positive; DOTS_ERR_STATE (untouched as well): a time slab,
 * WARM when z_mid was not materialised by the last step (dots_step_flags).  dots_bench_kernel(which = 5) times the WARM launch alone. */
enum { DOTS_RESTART_COLD = 0, DOTS_RESTART_WARM = 1 };
typedef struct dots_restart_desc {
    const double *mu0, *mu1;     /* [V] each, in the numbering of dots_problem_desc (the device numbering)                      */
    int32_t device_pointers;     /* 0: mu0 / mu1 are host addresses; 1: device addresses on the context's device               */
    int32_t mode;                /* DOTS_RESTART_COLD or DOTS_RESTART_WARM                                                     */
    double factors[4];           /* WARM: multipliers of (phi, A, B, lambda_c), the z arrays, (mu, E), the beta arrays          */
    double *ms;                  /* NULL, or HOST out: device milliseconds of the call's launches and memsets                  */
} dots_restart_desc;
int dots_restart(dots_ctx *ctx, const dots_restart_desc *desc);

/* ---- Wasserstein barycentres: one mirror-descent step on the device ---------------------------------------------------------------
 * dots_barycenter_update moves the common first end mass nu of n transport problems (nu -> mu_k) on one surface along the weighted
 * sum of their cost gradients and renormalises it (dots_socp_amd/barycenter.py: update_host is the specification), from potentials
 * and masses that are device memory: phi0[k] is what dots_sensitivity(device_pointers = 1) wrote for problem k, as stored (no gauge
 * fixed).  With V = n_vertices, in this order:
 *   m_k = sum(phi0[k]) / V
 *   g[v] = 0; for k ascending: g[v] = g[v] + weights[k] * (-(phi0[k][v] - m_k))
 *   y[v] = nu[v] * exp((-eta) * g[v]);  S = sum(y);  nu[v] = y[v] * (mass / S)
 *   scalars = { S, sum |nu_new - nu|, max |g|, min nu_new }
 * Element by element the operations of update_host in its order; exp is the device library's (within 1 ulp), and every sum is a
 * two-stage reduction in a fixed order carried with error-free additions, so it equals the host's exactly rounded sum to an ulp:
 * reproducible from call to call, equal to update_host to rounding.  Four launches (csrc/kernels_barycenter.hip), plain loads and
 * stores; 32 bytes cross to the host.
 * The call takes NO context: it needs nothing of a solve's state, so it reads and changes none, and what a call does to the deferred
 * work of a context (csrc/admission.h) does not arise.  What it needs of the surface comes in the descriptor: the device, the
 * vertex count, the stream its launches run on (the caller orders it against whatever wrote the inputs; the call returns with that
 * stream synchronised), scratch of dots_barycenter_scratch(V) doubles, and -- for nu_device_order, the values in the vertex
 * numbering of the contexts, which dots_restart(device_pointers = 1) reads -- the row of every caller vertex in that numbering
 * (the inverse of dots_problem_desc.perm_vert; an entry outside [0, V) is not written).
 * DOTS_ERR_ARGUMENT (nothing launched, nu untouched): a NULL desc, phi0, phi0[k], weights, nu, scratch or scalars; n outside 1 .. 16;
 * n_vertices < 1; a weight, eta or mass that is not finite; vertex_row without nu_device_order; nu, nu_device_order and scratch that
 * overlap.  An entry of nu that is not positive is the caller's business (update_host refuses it). */
typedef struct dots_barycenter_desc {
    int32_t n;                   /* potentials, 1 .. 16                                                                         */
    int32_t device;              /* HIP device ordinal of every device pointer below                                            */
    int32_t n_vertices;          /* V                                                                                           */
    int32_t reserved;
    const double *const *phi0;   /* HOST [n] of DEVICE pointers to [V] doubles, caller numbering                                */
    const double *weights;       /* HOST [n]                                                                                    */
    double eta;                  /* step                                                                                        */
    double mass;                 /* the total mass nu is normalised to                                                          */
    double *nu;                  /* DEVICE [V], caller numbering, updated in place                                              */
    double *nu_device_order;     /* DEVICE [V] or NULL: out, nu_device_order[vertex_row[v]] = nu[v]                             */
    const int32_t *vertex_row;   /* DEVICE [V] or NULL (the identity): caller vertex -> row of nu_device_order                  */
    double *scratch;             /* DEVICE [dots_barycenter_scratch(V)], contents unspecified before and after                  */
    void *stream;                /* the HIP stream of the launches; NULL = the legacy default stream                            */
    double *scalars;             /* HOST out [4]: sum, change, gmax, min                                                        */
    double *ms;                  /* NULL, or HOST out: device milliseconds of the launches                                      */
} dots_barycenter_desc;
int64_t dots_barycenter_scratch(int32_t n_vertices);      /* doubles; -1 if n_vertices < 1 */
int dots_barycenter_update(const dots_barycenter_desc *desc);

/* ---- Linearised transport: tangent vectors at a reference measure and their Gram matrix, on the device ------------------------------
 * With the N problems (sigma -> mu_i) solved from one reference measure sigma, the initial velocities v_i = grad phi0_i are the
 * logarithmic map at sigma, and G_ij = sum_f w[f] v_i[f] . v_j[f] -- w[f] the mass of sigma on triangle f -- is their Gram matrix in
 * L2(sigma): G_ii + G_jj - 2 G_ij approximates W2^2(mu_i, mu_j) with no further solve (dots_socp_amd/tangent.py holds the
 * specifications velocities_host, weights_host and gram_host).  Three calls, from potentials and masses that are device memory:
 *   dots_tangent_velocities   velocities[i][f][d] = (hat[f][0][d] * p0 + hat[f][1][d] * p1) + hat[f][2][d] * p2, p_c = phi0[i][triangles[f][c]];
 *                             phi0[i] is what dots_sensitivity(device_pointers = 1) wrote for problem i, as stored (no gauge is
 *                             fixed: the hat gradients of a triangle sum to zero).  The specification's bits.
 *   dots_tangent_weights      rho_c = sigma[v_c] / mass_vert[v_c]; w[f] = ((rho_0 + rho_1) + rho_2) * (area_tri[f] * (1.0 / 3.0)); sigma may
 *                             have zeros.  The specification's bits.
 *   dots_tangent_gram         G[i][j] = sum over f of w[f] * ((A[i][f][0] * B[j][f][0] + A[i][f][1] * B[j][f][1]) + A[i][f][2] * B[j][f][2]); B = NULL
 *                             means B = A.  The terms are the specification's; the sum is a two-stage reduction in an order that
 *                             depends on F alone, carried with error-free additions, so it equals the host's exactly rounded sum to an
 *                             ulp, is the same from call to call, is symmetric bit for bit when B is A, and a block of rows and
 *                             columns computed alone equals that block of the whole.  na * nb doubles cross to the host.
 * The calls take NO context (as dots_barycenter_update): they need nothing of a solve's state, so what a call does to the deferred
 * work of a context (csrc/admission.h) does not arise.  What they need of the surface comes in dots_tangent_desc, in the CALLER's
 * numbering: the device, V, F, the stream of the launches (the caller orders it against whatever wrote the inputs; every call returns
 * with that stream synchronised), and device pointers to the triangles, the hat gradients, the triangle areas and the vertex masses
 * (dots_problem_desc's tables, which are in the device numbering, permuted back).  A call reads only the tables it needs and checks
 * only those.  A triangle index outside [0, V) is not the library's business: the kernels read phi0, sigma and mass_vert at the
 * indices they find.
 * DOTS_ERR_ARGUMENT (nothing launched): a NULL desc, table or array; V or F below 1; n, na or nb below 1 or na or nb above 4096; a NULL
 * phi0[i]; an output (velocities, w, G's scratch) that overlaps an input of the same call.  csrc/kernels_tangent.hip. */
typedef struct dots_tangent_desc {
    int32_t device;              /* HIP device ordinal of every device pointer                                                  */
    int32_t n_vertices;          /* V                                                                                           */
    int32_t n_triangles;         /* F                                                                                           */
    int32_t reserved;
    const int32_t *triangles;    /* DEVICE [F][3], caller numbering         (velocities, weights)                               */
    const double *hat_grad;      /* DEVICE [F][3][3] [f][corner][xyz]       (velocities)                                        */
    const double *area_tri;      /* DEVICE [F]                              (weights)                                           */
    const double *mass_vert;     /* DEVICE [V]                              (weights)                                           */
    void *stream;                /* the HIP stream of the launches; NULL = the legacy default stream                            */
    double *ms;                  /* NULL, or HOST out: device milliseconds of the call's launches                               */
} dots_tangent_desc;
/* phi0: HOST [n] of DEVICE pointers to [V] doubles; velocities: DEVICE out [n][F][3] */
int dots_tangent_velocities(const dots_tangent_desc *desc, int32_t n, const double *const *phi0, double *velocities);
/* sigma: DEVICE [V]; w: DEVICE out [F] */
int dots_tangent_weights(const dots_tangent_desc *desc, const double *sigma, double *w);
/* doubles of scratch a Gram call needs; -1 if na, nb or F is out of range */
int64_t dots_tangent_gram_scratch(int32_t na, int32_t nb, int32_t n_triangles);
/* A: DEVICE [na][F][3]; B: DEVICE [nb][F][3] or NULL (= A, nb must equal na); w: DEVICE [F]; scratch: DEVICE
 * [dots_tangent_gram_scratch(na, nb, F)], contents unspecified before and after; G: HOST out [na][nb] */
int dots_tangent_gram(const dots_tangent_desc *desc, int32_t na, const double *A, int32_t nb, const double *B, const double *w,
                      double *scratch, double *G);

/* ---- solve session: moved vertices on a live context ----------------------------------------------------------------------------
 * dots_move_vertices: the context takes other vertex positions of the SAME triangulation.  Everything that depends on the mesh graph
 * only is kept (tri, the corner lists, the CSR pattern, the permutations, the time modes, the elimination tree, the band plan, the
 * sweep schedule and every allocation); every table that depends on the positions is formed again on the device (kernels_geometry.hip:
 * the formulas of dots_assemble and dots_create in their order of operations, the same bits): hat, area_f, mass_v, c_D, fk_D, c_gA,
 * c_area, val, kdiag.  The host constants of dots_create (the KKT normalisation constants, norm_d, the vertex masses of norm_boundary's
 * loop, the hash dots_front_share compares, norm_boundary from the masses the context holds) are formed again from area_f, mass_v and
 * val downloaded once (about 10 V doubles) in dots_create's loops: a new context's bits for the moved mesh.
 *   Before the geometry changes a pending penalty division is carried out and z_mid materialised with the OLD geometry, as for
 *     dots_download; a launch ahead, an armed penalty decision, the carried gathers and the fused sums are dropped.
 *   A factor the context owns is computed again from K + (sigma_a + eps) M into the allocations it has: the numeric factorisation,
 *     the merged blocks, the top band's inverse, the leaves' packed inverses and coupling records.  Nothing of the schedule changes.
 *   The state arrays are left as they are.  The iterate's derived quantities and the parameters belong to a run on the old surface:
 *     the context requires a dots_restart (cold or warm) before it steps; until then dots_step, dots_step_many, dots_run_phase,
 *     dots_kkt*, dots_objective* return DOTS_ERR_STATE.  dots_restart then forms norm_boundary from the new vertex masses.
 *   ms (optional, HOST out [3]): device milliseconds of the assembly launches, of the factor refresh, of the whole call.
 * DOTS_ERR_ARGUMENT, the context keeping its old geometry, factor and state, fully usable: NULL arguments, a coordinate that is not
 * finite, a triangle whose area is not positive, a vertex whose mass is not positive (areas and hat gradients are formed in scratch
 * first; host positions are checked for finiteness on the host).  DOTS_ERR_STATE (untouched as well): a time slab, a factor store that
 * is shared (a sharer, or an owner with sharers), a multigrid hierarchy installed, a non-modal context, a factor installed from the
 * caller's values, params.eps other than the factor's.  DOTS_ERR_MEMORY (untouched): the temporaries of the factorisation do not fit.
 * A pivot that is not positive in the refresh (impossible for valid areas and eps >= 0) releases the factor and returns the
 * factorisation's error: the context is then a PCG context, as after a failed dots_front_setup. */
typedef struct dots_move_desc {
    const double *vertices;      /* [V][3], in the numbering of dots_problem_desc (the device numbering)                        */
    int32_t device_pointers;     /* 0: a host address; 1: a device address on the context's device                              */
    int32_t reserved;
    double *ms;                  /* NULL, or HOST out [3]                                                                       */
} dots_move_desc;
int dots_move_vertices(dots_ctx *ctx, const dots_move_desc *desc);

/* dots_move_vertices_many: every holder of ONE factor store (dots_front_share) takes the other vertex positions together -- a batch
 * whose surface moves.  ctxs[0 .. n) are exactly the holders of the store: pairwise distinct, all with the same store, n its number
 * of holders; one context that holds its store alone (or has no factor) is the case n = 1, which is dots_move_vertices bit for bit.
 * dots_move_vertices itself keeps refusing a shared store.
 *   Every check runs for every member before any member changes; the positions are validated once, on ctxs[0], in scratch.  After a
 *     refusal all contexts keep geometry, factor and state and stay fully usable.  DOTS_ERR_ARGUMENT: NULL arguments, a coordinate
 *     that is not finite, an area or a vertex mass that is not positive.  DOTS_ERR_STATE: what dots_move_vertices refuses a context
 *     for (a time slab, a multigrid hierarchy, a non-modal context, a factor from the caller's values, another eps, scratch that does
 *     not fit), a list that is not the whole set of holders, members whose triangle tables are numbered differently.
 *     DOTS_ERR_MEMORY: the temporaries of the factorisation do not fit.
 *   Then every member does on its own stream what dots_move_vertices does to its context: the pending division and z_mid with the OLD
 *     geometry, the launch ahead and what goes with it dropped, the nine tables committed (from the one scratch), a dots_restart
 *     required before it steps.  The host constants are formed once, from one download of area_f, mass_v and val, and every member
 *     gets the same bits (and the same hash: a new context on the moved mesh can share, one on the old mesh cannot); norm_boundary
 *     is formed per member from the masses that member holds.
 *   The factor is refreshed ONCE into the store's allocations, after every member's stream has been synchronised (no sweep in flight
 *     on the old factor), and every stream is synchronised again before the call returns: launches, events and stream
 *     synchronisation only.  A pivot that is not positive releases the factor of EVERY member (all are PCG contexts then) and
 *     returns the factorisation's error.
 *   ms (HOST out [3]) as for dots_move_vertices: the assembly launches summed over the members, the one refresh, the whole call. */
int dots_move_vertices_many(dots_ctx *const *ctxs, int n, const dots_move_desc *desc);

/* dots_geometry_copy: the geometry tables of the context, copied device -> host behind a stream synchronisation (read-only; NULL
 * members are skipped).  Device numbering; corner_scale and corner_grad_area in corner-list order. */
typedef struct dots_geometry_tables {
    double *area_tri;            /* [F]        */
    double *hat_grad;            /* [F][3][3]  */
    double *mass_vert;           /* [V]        */
    double *lap_val;             /* [nnz]      */
    double *kdiag;               /* [V]        */
    double *corner_scale;        /* [3F] c_D = sqrt(area / mass) per corner-list entry */
    double *corner_grad_area;    /* [3F][3] c_gA = hat gradient * area per corner-list entry */
} dots_geometry_tables;
int dots_geometry_copy(dots_ctx *ctx, const dots_geometry_tables *out);

/* ---- levels of a cascade in space from ONE mesh: coarsen on the host, locate on the device ------------------------------------
 * dots_coarsen: half-edge-collapse decimation of the mesh (xyz [V][3], tri [F][3]) towards `n_target` vertices, host only (no
 * device work; dots_socp_amd/meshes.py: coarsen(backend="python") is the specification and states the rules; both return the same
 * arrays).  Coarse vertices are a subset of the fine ones.  Copy out with dots_coarsen_copy: kept [dots_coarsen_vertices] (ascending
 * fine indices), tri [dots_coarsen_triangles][3] (the surviving triangles in fine order and corner order, in FINE vertex indices).
 * The target may not be reached (nothing collapsible is left): the caller sees the count.
 * DOTS_ERR_ARGUMENT before any work: NULL pointers, sizes < 1, n_target < 1, an index out of range, non-finite coordinates, a
 * zero-area triangle, an edge with more than two triangles, two triangles crossing an edge in the same direction. */
typedef struct dots_coarse_mesh dots_coarse_mesh;
int dots_coarsen(int32_t n_vertices, int32_t n_triangles, const double *xyz, const int32_t *tri, int32_t n_target, dots_coarse_mesh **out);
int64_t dots_coarsen_vertices(const dots_coarse_mesh *mesh);
int64_t dots_coarsen_triangles(const dots_coarse_mesh *mesh);
int dots_coarsen_copy(const dots_coarse_mesh *mesh, int32_t *kept, int32_t *tri);
void dots_coarsen_free(dots_coarse_mesh *mesh);

/* dots_mesh_locate: the closest point of the mesh (vertices, triangles) to every one of `points`, over ALL triangles, on device
 * `device` (no context: it runs once per pair of levels).  Per point and triangle the region test of Ericson's closest point on a
 * triangle in a fixed order of operations (dots_socp_amd/cascade.py: closest_scalar_order); the winner is the smallest (squared
 * distance, triangle index).  The outputs equal cascade.locate_exact bit for bit.  With corner_points: for point i the corner of
 * triangle[i] with the largest clamped weight of each of its three corner points with respect to that one triangle, the first
 * maximum on a tie (cascade.corner_exact).  A uniform grid over the mesh is built on the host; one lane per point walks rings of
 * cells until the best distance certifies the result or the ring covers the grid.
 * DOTS_ERR_ARGUMENT (nothing launched): NULL desc or a NULL required pointer, sizes < 1, corner without corner_points, an index out of
 * range, a zero-area triangle, non-finite coordinates or points; DOTS_ERR_NO_DEVICE without a HIP device. */
typedef struct dots_mesh_locate_desc {
    int32_t n_points, n_vertices, n_triangles, reserved;
    const double *points;          /* host [n_points][3]                                                              */
    const double *vertices;        /* host [n_vertices][3]                                                            */
    const int32_t *triangles;      /* host [n_triangles][3]                                                           */
    const double *corner_points;   /* NULL, or host [n_points][3][3]: three points per point, for `corner`           */
    int32_t *triangle;             /* host out [n_points]                                                             */
    double *weights;               /* host out [n_points][3]: clamped barycentric weights, >= 0, summing to 1         */
    double *distance;              /* host out [n_points]                                                             */
    int32_t *corner;               /* NULL, or host out [n_points][3] (needs corner_points)                           */
    double *ms;                    /* NULL, or out: milliseconds of the launches on the device                        */
} dots_mesh_locate_desc;
int dots_mesh_locate(const dots_mesh_locate_desc *desc, int device);

/* The three queries below are admitted as calls that change something: a pending penalty division is carried out and what the context
 * carried is dropped (results do not depend on it).
 * launches one direct solve takes: 2 x bands of tree heights (one per band and sweep; a band is one height unless
 * dots_front_desc.band_ptr merges heights), minus one with dots_front_desc.top_inverse */
int dots_front_launches(dots_ctx *ctx);
/* out[4]: factor bytes one solve reads with one block per tree node (both sweeps: the algorithmic bytes of the solve),
 * the bytes it reads as installed (merged bands store more), tree heights, bands */
int dots_front_info(dots_ctx *ctx, double *out);
/* the mode pitch `values` must be laid out with (power of two >= the context's mode count, >= 8) */
int dots_front_pitch(dots_ctx *ctx);

/* ---- measurement ------------------------------------------------------------------------- */
/* Launch the dominant kernel (the PCG operator application) `reps` times on the context's stream
 * between two hipEvents and return the average milliseconds per launch and the algorithmic bytes
 * one launch moves (DESIGN.md section "roofline"). */
/* which: 0 PCG operator application, 1 PCG vector update, 2 one multigrid V-cycle, 3 both sweeps of the direct
 * solve, 4 one calibration launch (k_calib_stream: reads and writes *bytes_per_launch bytes each, 8 B per lane)
 * for the PMC traffic counters, 5 the in-place rescaling launch of dots_restart(DOTS_RESTART_WARM) over the twelve state arrays with
 * every factor 1 (the state keeps its values; not on a time slab).  DOTS_ERR_STATE for 0, 1 and 2 on a modal context of T+1 > 256
 * (the PCG takes 256 modes) */
int dots_bench_kernel(dots_ctx *ctx, int which, int reps, double *ms_per_launch, double *bytes_per_launch);

/* diagnostics: which = 0 KKT read-backs whose mailbox sequence number never arrived (the sums were then copied from the
 * device scalars instead: never stale), 1 mailbox hand-overs so far, 2 penalty decisions taken ahead of the host (dots_penalty_ahead), 3 those the
 * caller's own decision then confirmed, 4 tree leaves the sweeps of the direct solve handle as explicit local inverses
 * (0: the leaves' band runs in the band kernels), 5 whether those leaves take their coupling from per-row
 * records (1) or from the CSR of K (0: a row holds more entries than a record, or DOTS_FRONT_LEAFINV=2), 6 whether steps 2+3 stream
 * beta_mid with the non-temporal hint (decided by dots_front_setup from the sizes of factor and state), 7 sweep launches the last
 * batched solve (dots_laplacian_solve_many, dots_step_many, dots_bench_many) enqueued, read on the batch's first context, 8 of those, the
 * launches that took fewer right-hand sides than their chunk of DOTS_FRONT_NR problems held because NR regions of LDS would not fit or
 * a workgroup of 1024 threads takes fewer (the launch was split), 9 bytes this context has copied device -> host through dots_download,
 * dots_readout, dots_flow_map, dots_flow_push, dots_flow_trace and dots_flow_slide since it was created (the layer sums of dots_readout are written by the device itself and not copied), 10 device
 * allocations this context holds for its factor: its own (update planes, carried gathers) plus those of the store it holds with
 * the factor's other sharers (0 without a factor, also after a dots_front_setup that failed), 11 the launches the
 * last multigrid V-cycle enqueued on this context took, as a bit mask: 1 restriction with a workgroup per coarse row, 2 restriction
 * with a thread per entry, 4 coarsest solve with a workgroup per row, 8 coarsest solve with a thread per entry, 16 the one-launch
 * coarse tail, 32 post-smoothing of a level between the finest and the tail, 64 the down kernel on such a level, bits 8-11 the
 * number of levels inside the tail launch (0: no cycle since dots_mg_setup installed or released the hierarchy, or since
 * dots_mg_enable(ctx, 0)), 12 the launches of the last dots_step iteration on this context, as a bit mask: the right-hand-side kernel
 * (1 k_rhs, 2 k_rhs_modes, 4 k_rhs_modes2, 8 k_rhs_modes_mfma), 16 it streamed the carried per-corner sums (CARRIED), 32 it applied a
 * pending penalty division (DIV), 64 the cone projection rode in that launch, 128 it ran as k_soc_projection; steps 2+3 (256
 * k_q_lambda_mult_triangle, 512 ..._triangle2, 1024 ..._carry), bits 11-12 their z_mid mode (0 read, 1 rebuild and store, 2 rebuild
 * only), 8192 with the fused KKT sums, 16384 with the division, 32768 beta_mid streamed with the non-temporal hint, 65536 z_mid
 * deferred (0: no iteration since a call that changed state or parameters; a right-hand side enqueued ahead of its iteration by
 * DOTS_STEP_RHS_AHEAD starts the record of that iteration), 13 the path of the last launches of the PCG kernels on this context (a
 * solve of step 1 without the direct solver, dots_mg_apply, the laplacian_apply operator, dots_bench_kernel 0-2), as a bit mask with the
 * tiling packed above it: 1 the batched per-mode PCG (clear: the coupled space-time operator), 2 the per-workgroup partial rows are
 * summed by k_collapse behind every producer, 4 workgroups of fewer than 1024 threads, 8 multigrid preconditioner; bits 8-19 the
 * vertices per tile, bits 20-31 the CSR entries of a tile staged in LDS (further entries are read from global memory), from bit 32 the
 * number of workgroups (0: no such launch yet; on a windowed context the last window's), 14 low byte: the windows the last PCG
 * solve on this context ran (0: none yet, or it ran unwindowed), bit 8: the windowed time transforms ran (dots_pcg_windows),
 * 15 which of the launches around the direct solve last ran in the form that keeps its loads in flight (time pitch 8, 16 or 32; by
 * rule where a compute unit gets few workgroups, DOTS_RHS_DEEP=0/1 forces either): 1 the right-hand side with the carried sums
 * (k_rhs_modes2_deep; a right-hand side starts a new record), 2 the inverse time transform (k_time_modes_tile_fast); same results
 * bit for bit either way;
 * -1 for an unknown counter */
int64_t dots_debug_counter(dots_ctx *ctx, int which);

/* device memory in use by the context, bytes */
int64_t dots_device_bytes(dots_ctx *ctx);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DOTS_SOCP_HIP_H */

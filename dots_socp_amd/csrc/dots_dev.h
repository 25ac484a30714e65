// Internal declarations shared by the HIP translation units of libdotsocp_hip.so (gfx950 only).
//
// Device data layout ("time-fastest"): every spatial gather of the path -- a vertex reading its
// neighbours / corners, a triangle reading its three vertices -- touches one contiguous row of
// TP doubles (TP = time pitch, power of two >= T+1), so all HBM reads coalesce:
//     node / interval arrays   x[v][t]                 idxV(v,t)       = v*TP + t
//     triangle arrays          B[f][c][t]              idxF(f,c,t)     = (f*3+c)*TP + t
//     corner arrays            z_mid[f][k][s][c][t]    idxM(f,k,s,c,t) = ((((f*3+k)*2+s)*3+c)*TP + t
// Interval arrays use t in [0,T), node arrays t in [0,T]; padding columns stay zero.
// Corner entries live in the column of the NODE they are compared with (z_mid[t][s] pairs with B[t + s],
// solver_socp.py:934-940): column t + s.  The thread that owns B[f][c][node] then owns every corner entry of
// its column, which is what lets the time axis be cut into slabs without any exchange inside steps 2+3.
//
// Time slabs (multi-GPU, one context per rank): a context holds the columns of the nodes [t0, t0 + nl) only
// (local column j = node t0 + j = interval t0 + j); T stays the GLOBAL number of intervals.  What a kernel needs
// from the neighbouring slabs arrives in small per-vertex / per-triangle halo arrays (X_lo ... B_hi below).
// On one GPU t0 = 0, nl = T + 1, ni = T and no halo is ever read.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/dots_socp_hip.h"
#include "admission.h"
#include "step_choice.h"

namespace dots {

constexpr int BLOCK = 256;           // threads per workgroup = 4 wave64
constexpr int TILE_ELEMS = 1024;     // (vertex,time) elements per workgroup tile
constexpr int LDS_NNZ_CAP = 1536;    // CSR entries of one row block staged in LDS (18 KB)
constexpr int MAX_SUMS = 24;         // reduction slots per kernel
constexpr double INV_SQRT3 = 0.57735026918962576451;

void set_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define DOTS_HIP(call)                                                        \
    do {                                                                      \
        hipError_t e__ = (call);                                              \
        if (e__ != hipSuccess) return ::dots::hip_fail(e__, #call, __FILE__, __LINE__); \
    } while (0)

// A run-time choice as a template argument: fn(std::integral_constant<T, V>{}) for the listed V that equals v (the last one when none does)
template <auto V, auto... Vs, typename Fn>
inline void with_constant(decltype(V) v, Fn &&fn) {
    if constexpr (sizeof...(Vs) > 0) {
        if (v != V) return with_constant<Vs...>(v, fn);
    }
    fn(std::integral_constant<decltype(V), V>{});
}

// Everything a kernel needs, passed by value.
struct Dev {
    int T, V, F, TP, tp_shift;
    int t0;          // global index of the node in local column 0
    int nl;          // nodes held here (columns [0, nl));  T + 1 on one GPU
    int ni;          // intervals held here = min(nl, T - t0);  T on one GPU
    int slab;        // 1: this context is one time slab of a multi-GPU solve
    int VT;          // vertices per tile = TILE_ELEMS / TP
    int n_vtiles;    // ceil(V / VT)
    int FT;          // (triangle,component) rows per tile = TILE_ELEMS / TP
    int n_ftiles;    // ceil(3F / FT)
    double h;        // 1 / T
    // mesh constants
    const int *tri;          // [F][3]
    const double *hat;       // [F][3][3]
    const double *area_f;    // [F]
    const double *mass_v;    // [V]
    const int *cptr;         // [V+1]
    const int *cidx;         // [3F]  f*3+k
    const double *c_D;       // [3F]  sqrt(area_f / mass_v) per corner-list entry
    const double *c_gA;      // [3F][3] hat gradient * area_f per corner-list entry
    const double *c_area;    // [3F]  area_f per corner-list entry
    const double *fk_D;      // [3F]  the same sqrt(area_f / mass_v), indexed by corner f*3+k
    const int *rowptr;       // [V+1]
    const int *col;          // [nnz]
    const double *val;       // [nnz]
    const double *kdiag;     // [V] diagonal of K
    const double *mu0, *mu1; // [V]
    const int *perm_v, *perm_f;
    const double *Q;         // [(T+1)^2] or null
    const double *Qpad, *QpadT;  // [TP][TP] Q and its transpose, zero padded (operands of the MFMA transform)
    const double *sigma;     // [T+1] or null
    // state
    double *phi, *A, *B, *lam, *zf, *zm, *ze, *mu, *E, *bf, *bm, *be;
    double *B_st, *bm_st;    // where steps 2+3 (ql_lane) STORE the new B and beta_mid: the arrays themselves, or -- on an iteration whose z_mid may
                             // be asked for -- the alternate B buffer and z_mid's storage (Carried::zmid).  Every Dev a context keeps has
                             // B_st == B and bm_st == bm; only the copy launch_q_lambda_mult hands to k_q_lambda_mult_carry ever differs, so
                             // the tile kernels (k_q_lambda_mult_triangle, k_q_lambda_mult_triangle2) store to the arrays themselves.
    double *lamc;            // [V][TP] cone multiplier of the last projection (z_mid = lamc/D * pre-image, rebuilt in steps 2+3)
    // DOTS_STEP_CARRY (one GPU, direct solver, pitch <= 128; null otherwise): what the right-hand side and the cone projection of the
    // NEXT iteration gather per corner, stored by steps 2+3 in corner-LIST order (row j = position in cidx; cpos: f*3+k -> j)
    double *cn_sq;           // [3F][2][TP] halves s = 0, 1 of sum_xyz (D (sz/sqrt3 B - beta_mid))^2, column = interval
    double *cn_g;            // [3F][TP]    sum_xyz area * hat * (B - E), column = node
    double *cn_e;            // [3F][TP]    sum_xyz area * hat * E, column = node: the gather of Dual(alpha) (read-back iterations only)
    double *cn_lo;           // [3F] time slab: the s = 1 half of interval t0 - 1 (formed at this slab's first node; summed into send_nsq)
    const int *cpos;         // [3F]
    // halos of a time slab (device arrays, written by dots_slab_unpack / the inverse transform; see SlabHalo in dots_api.hip)
    const double *X_lo;      // [V]  (A + lambda_c - mu) of interval t0 - 1           (right-hand side at node t0)
    const double *lamc_lo;   // [V]  cone multiplier of interval t0 - 1                (steps 2+3 at node t0)
    const double *mu_lo;     // [V]  mu of interval t0 - 1                             (KKT: Dual(alpha), Comp(m, rho o B))
    const double *nsq_hi;    // [V]  s = 1 half of the cone's squared norm for interval t0 + nl - 1, formed by the next slab
    double *phi_hi;          // [V]  phi at node t0 + nl (written by this rank's inverse transform)
    const double *B_hi;      // [3F] B at node t0 + nl                                  (KKT: Comp(rho, f(q)))
    // PCG workspace (node layout)
    double *cg_b, *cg_r, *cg_z, *cg_p0, *cg_p1, *cg_Ap, *cg_x;
    double *partials;        // [MAX_SUMS or NC][n partial blocks]
    double *scal;            // device scalars, see CgScal / sums
    int *flags;
    int cg_ncol;             // columns the PCG works on (T+1 on one GPU; the rank's modes when sharded)
};

// One level of the multigrid hierarchy (device pointers).  A_l = K_l + s M_l on one pattern;
// level 0 has vM == nullptr (M is the diagonal mass, held in dM).
struct MgLevelDev {
    int n, nc;                               // rows of this level / of the next coarser one
    const int *rp, *col;
    const double *vK, *vM, *dK, *dM;
    const int *p_rp, *p_col;                 // P: n x nc
    const double *p_val;
    const int *r_rp, *r_col;                 // R = P^T: nc x n
    const double *r_val;
    const int *ap_rp, *ap_col;               // A P = K P + s M P: n x nc, two value arrays on one pattern
    const double *ap_vK, *ap_vM, *ap_vP;     // ap_vP: P itself on the pattern of A P (zeros where absent)
    double *b, *bt, *t;                      // level vectors [n][TP]: rhs, D^-1 rhs / result, residual (level 0 borrows the PCG's r, z, Ap)
};
// Launches one V-cycle took (Ctx::mg_path, dots_debug_counter 11): a test pinned to one kernel asserts that it still runs there
enum {
    MG_PATH_RESTRICT_ROWS = 1, MG_PATH_RESTRICT_FLAT = 2, MG_PATH_COARSE_ROWS = 4, MG_PATH_COARSE_FLAT = 8, MG_PATH_TAIL = 16,
    MG_PATH_POST = 32,           // k_mg_post: a level above the tail other than the finest
    MG_PATH_DOWN_ABOVE0 = 64,    // k_mg_down on such a level (vM != nullptr)
    MG_PATH_TAIL_LEVELS_SHIFT = 8      // levels inside k_mg_tail (1: the dense solve alone), bits 8-11
};
// Tiling and kernel family of the last PCG launches (Ctx::cg_path, dots_debug_counter 13), written by make_args: a test pinned to one
// path of the PCG kernels asserts that the launcher still puts it there.  Host bookkeeping only.
enum {
    CG_PATH_MODAL = 1,           // the batched per-mode PCG (0: the coupled space-time operator)
    CG_PATH_COLLAPSE = 2,        // k_collapse sums the partial rows behind every producer
    CG_PATH_SMALL_WG = 4,        // workgroups of fewer than 1024 threads
    CG_PATH_MG = 8,              // multigrid preconditioner
    CG_PATH_VT_SHIFT = 8,        // vertices per tile, bits 8-19
    CG_PATH_CAP_SHIFT = 20,      // staged CSR entries per tile, bits 20-31
    CG_PATH_G_SHIFT = 32         // workgroups, from bit 32
};
struct MgDev {
    int nlev = 0;
    MgLevelDev lv[10]{};
    const double *coarse_inv = nullptr;      // [nL][nL][TP]; on a windowed context one block [nL][nL][256] per window, one after the other
    int64_t coarse_win_stride = 0;           // doubles per window block (0: installed unwindowed)
    double omega = 2.0 / 3.0;
};

// Direct (multifrontal) solve of the modal problems: the factor of dots_socp_amd/frontal.py on the device.
// F_p = [L_pp^-1 ; A_bs A_ss^-1] of node p starts at F + (foff[p] << tp_shift), entry (i, j, mode) at
// ((i * n_p + j) << tp_shift) + mode: the mode index is fastest, as in every node array.
struct FrontNode {            // a node of the elimination tree as the numeric factorisation sees it (kernels_factor.hip)
    int n, b;                 // separator rows eliminated here / boundary rows
    int k0;                   // elimination index of the first separator row
    int parent;               // parent node (-1: root)
    int64_t foff;             // first (row, col) entry of F_p
    int64_t bdoff;            // first boundary row of this node in bd_vertex
    int c0, c1;               // children (-1: none)
    int64_t ioff;             // first front row in the pull maps
    int64_t soff;             // first entry of the b x b Schur complement
};
// One node of the SWEEPS (kernels_front.hip): an original node, or the nodes of a band of tree heights that hang together
// merged into one block F' = [L'^-1 ; G'] (row stride n; L'^-1 block lower triangular over the members, children first).
struct SweepNode {
    int n, b;                 // columns = separator rows of all members / boundary rows (those of the band's top node)
    int k0;                   // sweep-order index of the first separator row
    int planes;               // update planes of this node that a child writes (the launch reads the band's bucket: 0, 2, 4 or 8)
    int64_t foff;             // first (row, col) entry of F'
    int64_t woff;             // first row of this node's update planes in W, m rows each
    int64_t parent_w;         // first row of the plane this node writes in its parent's W (-1: root)
    int64_t bdoff;            // first boundary row of this node in bd_vertex / cmap
};
// One workgroup of a sweep: the node's record and its block of rows (columns), in ONE 96-byte record so that the
// kernel's dependent-load chain starts with a single (scalar) load instead of descriptor -> node record.
struct FrontWork {
    SweepNode nd;
    int first;                // first row (forward) / first column (backward) of the block
    int lo;                   // forward: first column that can be nonzero in the block's rows; backward: number of row ranges
    int rs[4], re[4];         // backward: separator-row ranges [rs, re) that can be nonzero in the block's columns (rs[0] = first)
    int end;                  // backward: one past the last column of the block's member; forward: > 0 = every row of the block runs over
                              // the columns [lo, end) (a node that stores an explicit inverse), 0 = up to the diagonal
    int pad;
};
// One leaf of the tree when the leaves' band is stored as explicit local inverses (kernels_front.hip: k_front_leaf_fwd / _bwd)
struct LeafWork {
    int k0, n, b, pad;        // first sweep-order index (= device vertex: the leaf is numbered in place), separator / boundary rows
    int64_t soff;             // first entry of S = A_ss^-1 (lower triangle packed by rows) in FrontDev::leafS
    int64_t bdoff;            // first boundary row in bd_vertex / cmap
    int64_t parent_w;         // first row of the plane this leaf writes in its parent's W
    int64_t rowoff;           // first record of its boundary rows in FrontDev::leaf_bd
};
// The leaf's coupling to its boundary, copied once from the CSR of K into one record per row (the sweeps then reach it with ONE load
// behind the leaf's record instead of vertex -> row pointer -> entries): entries in CSR order, so the sums are the CSR path's, bit for bit
constexpr int LEAF_KC = 6, LEAF_KE = 8;
struct LeafBdRow {            // boundary row: where it goes in the parent's plane, its entries inside the leaf (position in the leaf, value; padded with zeros)
    int cm, cnt;
    int u[LEAF_KC];
    double v[LEAF_KC];
};
struct LeafSepRow {           // separator row (indexed by vertex): its entries OUTSIDE the leaf (vertex, value)
    int cnt, pad;
    int u[LEAF_KE];
    double v[LEAF_KE];
};
// One original node inside a merged band node (k_merge_member builds F' from the members' own blocks)
struct MergeMember {
    int n, b;                 // its separator / boundary rows
    int o, c0;                // first own column / first column of its subtree inside the merged node
    int64_t foff;             // its block [L^-1 ; G] in the factor (row stride n)
    int64_t ioff;             // first front row in the pull maps
    int64_t dst;              // first entry of the merged node's F'
    int64_t uoff;             // first entry of U_s (the update operator of its subtree on its boundary; columns from c0)
    int ns;                   // row stride of F' = columns of the merged node
    int ustride;              // row stride of U_s
    int uin;                  // U_s lives in: 0 the factor (its own G rows: no child inside the band), 1 scratch, 2 F' (the band's top node)
    int ch[2];                // its children inside the band by pull map (index of the member record, -1: none or below the band)
    int pad;
};
struct FrontDev {
    int n_nodes = 0, n_levels = 0;        // original nodes; launches per sweep (= bands of tree heights)
    const FrontNode *nodes = nullptr;     // original tree (factorisation)
    const int *vmap = nullptr;            // sweep-order index -> device vertex; nullptr when the device numbering is the sweep order
    const int *bd_vertex = nullptr;       // device vertex of every boundary row
    const int *cmap = nullptr;            // position of every boundary row in the parent's front
    const double *F = nullptr;            // original blocks, then the merged ones
    double *W = nullptr;                  // update planes [rows][TP]; entries no child writes stay zero
    const FrontWork *fwd_desc = nullptr, *bwd_desc = nullptr;             // per workgroup: node record + its block
    const double *leafS = nullptr;        // leaves as explicit inverses: S_p = A_ss^-1 of every leaf, one after the other (n_leaves > 0)
    const LeafWork *leaf_desc = nullptr;
    const LeafBdRow *leaf_bd = nullptr;   // coupling records (nullptr: the leaf kernels walk the CSR)
    const LeafSepRow *leaf_sep = nullptr;
    int n_leaves = 0, leaf_nmax = 0;      // leaves handled by the leaf kernels (0: the band kernels take band 0), their largest n
};

// What installing a factor decided about the sweeps (front_setup; dots_front_share copies it whole): one record per band = launch of a sweep
struct FrontBand {
    int fwd_first, fwd_n;     // its workgroups in fwd_desc
    int bwd_first, bwd_n;     // ... in bwd_desc
    int fwd_rb, bwd_cb;       // rows / columns per workgroup
    int fwd_nb, bwd_nb;       // threads per workgroup (256, or 1024 where a band has few rows)
    int fwd_qw;               // forward launch: -1 the fold kernel (k_front_fwd), >= 0 the row kernel with 2^qw lane groups per row
    int fwd_lds;              // row kernel: columns of w a workgroup stages in LDS (the band's longest block)
    int planes;               // update planes the forward launch reads per node (0, 2, 4 or 8)
};
struct FrontSchedule {
    static constexpr int MAX_BANDS = 64;
    int vec2 = 1;             // two modes per lane in the sweeps wherever the pitch allows (DOTS_FRONT_VEC2=0: never); the one field front_release keeps
    int n_bands = 0;          // launches per sweep (= FrontDev::n_levels)
    int top_inverse = 0;      // the top band holds explicit inverses: its forward launch writes x, the backward sweep skips it
    int heights = 0;          // tree heights of the installed factor
    int bm_nt = 0;            // steps 2+3 stream beta_mid with the non-temporal hint (decided by dots_front_setup: see ql_lane; DOTS_BM_NT = 0 / 1 overrides)
    int64_t w_rows = 0;       // rows of W (the sharers allocate as many)
    double bytes = 0.0;       // factor bytes one solve reads (both sweeps, merged blocks as stored)
    double bytes_unmerged = 0.0;   // the same for one launch per tree height (no merged bands)
    double eps = 0.0;         // eps the installed factor was built with
    FrontBand band[MAX_BANDS]{};
};
static_assert(std::is_trivially_copyable<FrontSchedule>::value, "Ctx is copied by value (dots_apply_operator, dots_laplacian_solve_many)");

// Layout of the device scalar block used by the PCG (all arrays have NC entries, NC <= 256).
struct CgScalOffsets {
    static constexpr int NCMAX = 256;
    static constexpr int RZ = 0;
    static constexpr int PAP = NCMAX;
    static constexpr int ALPHA = 2 * NCMAX;
    static constexpr int BETA = 3 * NCMAX;
    static constexpr int BREF = 4 * NCMAX;
    static constexpr int BMEAN = 5 * NCMAX;
    static constexpr int SUMS = 6 * NCMAX;     // MAX_SUMS reduction results for KKT / norms
    static constexpr int TOTAL = 6 * NCMAX + 64;
};
// flags: [0..NCMAX) done per column, [NCMAX] iteration counter
constexpr int FLAG_ITERS = CgScalOffsets::NCMAX;
constexpr int FLAG_TOTAL = CgScalOffsets::NCMAX + 8;

// Weighted sums the KKT residuals are combined from (kernels_kkt.hip; solver_socp.py:433-559): vertex sums, then triangle sums
enum {
    V_DPHI2 = 0, V_A2, V_LAM2, V_RESMU2, V_RFST2, V_REND2, V_MU2, V_AUX1_2, V_MUAUX1_2,
    V_COMP_AUX2, V_COMP_RES2, V_CONG_RES2, V_DUALAUX2, N_VSUMS,
    F_DX2 = N_VSUMS, F_B2, F_RESE2, F_E2, F_AUX2_2, F_EAUX2_2, F_AUX5_2, F_AUX5M_2, F_RMID2, N_SUMS
};
constexpr int N_FSUMS = N_SUMS - N_VSUMS;
static_assert(N_SUMS <= MAX_SUMS, "too many reduction slots");
struct KktArgs {
    uint32_t mask;
    double r, sz, cd, cong, ps, ds, bs;   // penalty, scale_factor_z, constant_d, congestion, prim/dual/boundary scale
};
// DOTS_STEP_KKT_SUMS: the sums steps 2+3 can form from their registers while they write the new iterate -- everything the
// conditions Prim(phi, q), Prim(q, z), Dual(beta) and Comp(rho, cong.) need (no gather across rows): per workgroup partial sums
struct KktFused {
    double *part_v = nullptr, *part_f = nullptr;   // [N_VSUMS][nv], [N_FSUMS][nf] (only the fused slots are written)
    int nv = 0, nf = 0;                            // workgroups of the vertex / triangle part of the launch that wrote them
};
constexpr uint32_t KKT_FUSED_MASK = 1u | 2u | 8u | 64u;

// What the PCG keeps between solves per set of columns it iterates on: the instantiated hipGraph of `iters` iterations (Dev is captured by
// value, so a window of modes has its own) and the iteration count that sizes the next solve's first burst.
// The captured Dev is a derived view (pcg_view): it carries d's state, cn_* and halo pointers as they were at capture.  That is sound
// because the kernels in the graph (k_cg_apply, k_cg_update, k_collapse, the k_mg_* of the V-cycle) read none of them: neither the
// pointers the two swaps of Ctx move (zf, ze, lamc, B, bm, zm, B_st, bm_st) nor cn_sq / cn_g / cn_e / cn_lo nor a halo -- only the mesh
// constants, sigma, the PCG vectors, partials, scal and flags (profiles/device_views/README.md has the list per view).
struct CgCache {
    hipGraphExec_t graph = nullptr;
    int iters = 0;
    double eps = -1.0, tol = -1.0;
    int mg = -1;
    int last_iters = 0;
};
constexpr int PCG_WINDOW = CgScalOffsets::NCMAX;      // modes per window of a windowed context (dots_pcg_windows)
constexpr int PCG_WINDOW_SHIFT = 8;
constexpr int PCG_MAX_WINDOWS = TILE_ELEMS / PCG_WINDOW;
static_assert((1 << PCG_WINDOW_SHIFT) == PCG_WINDOW, "window pitch");

struct Ctx;
struct FrontRecord;      // kernels_front.hip
// ---- launch wrappers implemented in the kernel files (all asynchronous on ctx stream) ----
int launch_soc_projection(Ctx *c, int zmid_mode = 0, bool with_inverse = false);   // 0: write z_mid; 1: write only the cone multiplier; with_inverse: extra workgroups do the modes -> time transform of phi
void preload_alm_kernels();
void preload_kkt_kernels();
void preload_transform_kernels();
struct RhsAhead;
// with_soc (only when rhs_writes_modes): the cone projection rides in the same launch; dv != 0 (only when rhs_divides: DOTS_ERR_STATE otherwise): a
// pending penalty division is applied to what is read; ahead: a launch ahead of its iteration names where the rider writes and the penalty
int launch_rhs(Ctx *c, bool with_soc = false, double dv = 0.0, const RhsAhead *ahead = nullptr);
bool rhs_divides(const Ctx *c);
bool ql_divides(const Ctx *c, int zmid_mode);
int launch_q_lambda_mult(Ctx *c, int zmid_mode = 0, double dv = 0.0);    // 0: read z_mid; 1: rebuild it from the multiplier and store it; 2: rebuild, do not store; dv != 0 (only when ql_divides): the dual arrays are divided as they are read and written back divided
int launch_rebuild_zmid(Ctx *c);                         // z_mid rebuilt from the old B / beta_mid a deferred step kept (admission.h: rebuild_zmid)
int launch_q_lambda_only(Ctx *c);                       // the (q, lambda_c) closed form alone (is_palm's step 0): z_mid is read from memory
int launch_adjust_penalty(Ctx *c, double factor);
int launch_scale_z(Ctx *c, double z_mul, double beta_mul, double sz_new);
int launch_scale_array(Ctx *c, int array_id, double factor);
int launch_to_device_layout(Ctx *c, int array_id, double *dev, const double *staged);      // dev: the array in device layout (the state's: c->arr(array_id))
int launch_from_device_layout(Ctx *c, int array_id, const double *dev, double *staged);
// The tables of a state carry (kernels_carry.hip), the caller's or their copies on the device.  mode: how a row is formed in space.
enum { CARRY_NESTED = 0, CARRY_LOCATED = 1, CARRY_SAME = 2 };
struct CarryTables {
    const int32_t *node_j, *interval_j;      // [T + 1], [T] source time point of every destination time point; null: one time grid
    const double *node_w, *interval_w;       // weight of source point j + 1
    const int32_t *vsrc;                     // [V][2] nested, [V][3] located, [V] or null same: source vertex rows
    const double *vw;                        // [V][3] located: weights
    const int32_t *fsrc;                     // [F] source triangle; same: or null
    const int32_t *csrc;                     // [F][3] source corner of every corner, or null: the same corner
    int mode;
};
// array `array_id` of dst = the one of src carried over with the device tables t, times factor, on dst's stream
int launch_carry(Ctx *dst, Ctx *src, int array_id, const CarryTables &t, double factor, const char *who);
int launch_operator(Ctx *c, int op, double scale, const double *in_staged, double *out_staged);
int launch_calibration(Ctx *c, double *bytes_each_way);
int cg_solve(Ctx *c, dots_step_stats *stats, bool defer_inverse = false);   // defer_inverse: phi is produced by the caller (soc_takes_inverse)
int cg_apply_operator(Ctx *c, const double *x_node, double *y_node);  // y = K x in node layout
int cg_finish_sharded(Ctx *c);                                        // phi of this time slab from all ranks' mode-space solutions (slab.x_recv)
int launch_slab_pack_iteration(Ctx *c);     // halos the neighbours need before the right-hand side / the projection -> slab.send_x, slab.send_nsq
int launch_slab_pack_kkt(Ctx *c);           // halos the neighbours' KKT kernels need -> slab.send_mu, slab.send_b
int cg_bench(Ctx *c, int which, int reps, double *ms, double *bytes);
int64_t cg_partials_needed(const Dev &d);   // doubles of Dev::partials the PCG uses
int front_setup(Ctx *c, const dots_front_desc *desc);
void front_release(Ctx *c);
// `zero_entries` > 0: T holds an old factor; that many entries of it are zeroed once the temporaries are allocated (front_refresh)
int front_factorize(Ctx *c, const dots_front_desc *desc, FrontDev &f, const std::vector<FrontNode> &nodes, double *T, const int *grounded_host, int64_t zero_entries = 0);
// dots_move_vertices: the numeric phases of front_setup again, into the allocations of the installed factor (Ctx::front_record)
int front_refresh_check(Ctx *c);      // DOTS_ERR_STATE / DOTS_ERR_MEMORY before anything is touched
int front_refresh(Ctx *c);
int front_solve(Ctx *c, const double *bhat, double *y, double *x);   // x = A^-1 bhat for every mode of the PCG view (y: scratch)
// the same for n problems on one shared factor (dots_front_share), up to Ctx::front_nr_max per launch, on cs[0]'s stream; n = 1 is front_solve
int front_solve_many(Ctx *const *cs, int n, const double *const *bhat, double *const *y, double *const *x);
// the time transforms around step 1's solve (kernels_modes.hip).  One GPU: b^ = Q^T `in` into `out`, and phi = Q x^ back
void modes_forward(Ctx *c, const double *in, double *out, bool direct, bool col0_sums = true);   // col0_sums: the PCG's forms leave the partial sums of mode 0 (mean removal)
int modes_inverse(Ctx *c, const double *x, double *phi, bool direct);
void modes_forward_sharded(Ctx *c, bool direct);   // time slab: this rank's modes of the all-gathered right-hand side (slab.b_recv) into the PCG view's cg_p0
int modes_forward_sums(const Ctx *c);              // partial sums of mode 0 the PCG's forward transform of this context leaves in Dev::partials (k_cg_bmean adds them)
int modes_windows_sums(const Dev &d);              // ... of a windowed context (cg_partials_needed: they lie in front of the PCG's own)
// enqueue z = MG(r) on the PCG view d (the context's own, or one window of it) with that view's coarse inverse; z holds D^-1 r on entry
int mg_vcycle(Ctx *c, const Dev &d, const double *coarse_inv, const double *r, double *z, double *t0, double *rz_part, int nb, int ept, int vt, int G);
int cg_mg_apply(Ctx *c, double *rz);        // dots_mg_apply: one V-cycle on what the PCG view's cg_r holds, as the PCG launches it; rz[mode] = sum of the r.z partial rows
int kkt_evaluate(Ctx *c, uint32_t mask, double *out);
int kkt_sums(Ctx *c, uint32_t mask, double *sums);                          // the weighted sums of this context's time slab
int kkt_sums_device(Ctx *c, uint32_t mask, double *device_sums);            // the same, left in the caller's device buffer (enqueue only)
int kkt_combine(Ctx *c, uint32_t mask, const double *sums, double *out);    // the residuals from the sums of the whole problem
int penalty_decision_ahead(Ctx *c, uint32_t mask, const double *sums);       // dots_penalty_ahead: the decision + the next iteration's first launch
bool env_int(const char *name, int lo, int hi, int *out);                   // validated integer switch from the environment
int kkt_n_sums();
int objective_evaluate(Ctx *c, double *out);
int objective_sums(Ctx *c, double *sums);
int objective_combine(Ctx *c, const double *sums, double *out);
int norm_square(Ctx *c, int array_id, int part, double *out);
int reduce_partials(Ctx *c, const double *partials, int n_slots, int n_blocks, int first_slot);  // -> scal[SUMS+first_slot+slot]
// dots_readout (kernels_readout.hip): mu (or E) in the caller's numbering and the reference layout, scaled, into `out`; one launch per chunk of
// 256 layers, each followed by ev[k]; part != null (mu): per-workgroup layer sums [layers][2][readout_workgroups], folded by launch_readout_fold
int launch_readout(Ctx *c, bool is_E, double *out, const int *inv, const double *w, const double *m0, const double *m1, int centred, double factor,
                   double *part, hipEvent_t *ev, int *n_chunks);
int readout_workgroups(const Ctx *c);
int launch_readout_fold(Ctx *c, const double *part, int layers, int n_wg, double *out);      // out[2 l], out[2 l + 1]: sum / negative sum of layer l
void preload_readout_kernels();
// dots_sensitivity (kernels_sensitivity.hip): the potentials at the two ends (one lane per caller vertex) and the stress (one lane per
// caller triangle corner).  Inputs in the DEVICE numbering, outputs in the caller's; an output that is null is not formed.
struct SensArgs {
    const double *phi, *mu;      // the state where it lies: [V][TP]
    const int *tri;              // [F][3]
    const int *inv_v, *inv_f;    // caller vertex / triangle -> device row, or null (same numbering)
    const int *perm_v;           // device vertex -> caller vertex, or null
    const double *mass;          // [V] vertex masses in the CALLER's numbering, or null: mass_dev
    const double *mass_dev;      // [V] Dev::mass_v
    double *phi0, *phiT;         // [V]
    double *stress;              // [F][3][6], on a 16-byte boundary
    double factor_phi, factor_mu;
    int V, F, T, tp_shift;
};
int launch_sensitivity(Ctx *c, const SensArgs &a);
// dots_restart (kernels_restart.hip): every element of state array k times factor[group(k)] in place, ONE launch over the twelve
// arrays (the padding columns are written as zeros), or with factor == null every element zeroed; *bytes (or null): what the launch
// reads and writes
int launch_restart_scale(Ctx *c, const double factor[4], double *bytes);
// sum over v of (mu0[v]^2 + mu1[v]^2) / mass_v[v] of two DEVICE arrays in a fixed order, left in *out on the host (waits for the stream)
int restart_boundary_sum(Ctx *c, const double *mu0, const double *mu1, double *out);
void preload_restart_kernels();
// dots_barycenter_update (kernels_barycenter.hip): nu <- nu * exp(-eta * sum_k w_k * (-(phi_k - mean_k))), renormalised to `mass`, in
// four launches on the caller's stream.  Every array in the CALLER's numbering except nu_dev (a second one); scratch from the caller.
constexpr int BARY_MAX_N = 16;                 // dots_barycenter_desc.n
constexpr int BARY_MAX_WORKGROUPS = 1024;      // of the update and the finish: the partial sums one workgroup folds
struct BaryArgs {
    const double *phi[BARY_MAX_N];      // [n] potentials, [V] each
    double w[BARY_MAX_N];
    double eta, mass;
    double *nu;                  // [V], updated in place
    double *nu_dev;              // [V] the same values in a second numbering, or null
    const int *inv_v;            // caller vertex -> row of nu_dev, or null (same numbering)
    double *y;                   // scratch [V]
    double *mean;                // scratch [BARY_MAX_N]
    double *part;                // scratch [6][G]
    double *out;                 // [4] sum, change, gmax, min
    int n, V, G;                 // G = barycenter_workgroups(V)
};
int barycenter_workgroups(int V);
int launch_barycenter(hipStream_t stream, const BaryArgs &a);
void preload_barycenter_kernels();
// dots_tangent_velocities / _weights / _gram (kernels_tangent.hip): the gradients of potentials per triangle, the reference measure's
// mass per triangle and the weighted Gram matrix of such fields, on the caller's stream, every array in the CALLER's numbering.
constexpr int TANGENT_VEL_N = 16;              // potentials per launch of k_tangent_velocities
constexpr int TANGENT_TILE = 4;                // entries per side of the Gram kernel's register tile
constexpr int TANGENT_CHUNK = 2048;            // triangles per workgroup of the Gram kernel, while the chunks are fewer than
constexpr int TANGENT_MAX_CHUNKS = 1024;       //   this: then every workgroup takes more
constexpr int TANGENT_MAX_N = 4096;            // fields per side of one Gram call
struct TangentVelArgs {
    const double *phi[TANGENT_VEL_N];      // [n] potentials, [V] each
    const int *tri;                        // [F][3]
    const double *hat;                     // [F][3][3]
    double *out;                           // [n][F][3]
    int n, F;
};
struct TangentGramArgs {
    const double *A, *B;      // [na][F][3], [nb][F][3] (B may be A)
    const double *w;          // [F]
    double *part;             // scratch [C][na * nb][2]
    double *G;                // [na][nb]
    int na, nb, F, C;         // C = tangent_chunks(F)
};
int tangent_chunks(int F);
int launch_tangent_velocities(hipStream_t stream, const TangentVelArgs &a);
int launch_tangent_weights(hipStream_t stream, const int *tri, const double *sigma, const double *mass_v, const double *area, double *w, int F);
int launch_tangent_gram(hipStream_t stream, const TangentGramArgs &a);
void preload_tangent_kernels();

// ---- dots_move_vertices (kernels_geometry.hip): the geometry tables from vertex positions, dots_assemble's and dots_create's bits
struct GeomScratch {
    double *area, *hat, *mass;   // [F], [F][3][3], [V]
    int *flag;                   // raised for a coordinate that is not finite, an area or a mass that is not positive
};
int launch_geometry_validate(Ctx *c, const double *xyz, const GeomScratch &s);      // triangle pass and the vertex masses, into scratch
int launch_geometry_commit(Ctx *c, const GeomScratch &s);                           // every table of the context from the scratch
void preload_geometry_kernels();
// The flow map (kernels_flow.hip): one lane per particle, the loop over the intervals inside the kernel.  Everything in the DEVICE
// numbering except the triangles written out, which perm_f takes back to the caller's.  A launch takes FlowArgs and FlowSpan, with
// deposits FlowPush, with the sliding mode FlowSlide: separate by-value kernel arguments, in the order args, push, span, slide.
struct FlowArgs {
    const double *mu, *E;        // the state where it lies: [V][TP], [F][3][TP]
    const int *tri;              // [F][3]
    const double *hat;           // [F][3][3]
    const int *nbr;              // [F][3] the triangle across the edge opposite corner k, packed (flow_pack_neighbour); -1 on the boundary
    const int *perm_f;           // device triangle -> caller triangle, or null
    const int *start_tri;        // [P]
    const double *start_w;       // [P][3]
    int *o_tri, *o_status, *o_rested, *o_cross;      // [P]
    double *o_w;                 // [P][3]
    int *tri_at;                 // [T + 1][P], or null
    double *w_at;                // [T + 1][P][3], or null
    double floor, h;
    int P, T, tp_shift, max_crossings;      // T is the number of intervals traversed, h is 1 / n_time
};
// turn i = 0 .. T - 1 takes the interval j0 + i dj; dj = -1 traces backward (the velocity negated).  The whole horizon is j0 = 0, dj = 1.
struct FlowSpan {
    double *action;              // [P] sum of best |u|^2 over the steps, or null
    int j0, dj;
};
// neighbour g, and the corners of g that name the vertices of corners (k + 1) % 3 and (k + 2) % 3 of the triangle the entry belongs to
constexpr int FLOW_MAX_TRIANGLES = 1 << 27;
inline int flow_pack_neighbour(int g, int ca, int cb) { return (g << 4) | (ca << 2) | cb; }
// what the tracer deposits besides.  Channel 0 is the mass, channels 1 .. A the mass times an attribute.
constexpr int FLOW_PUSH_CHANNELS = 5;
struct FlowPush {
    unsigned long long *acc;     // [A + 1][L][V] fixed-point sums, DEVICE vertex numbering, then one word: the contributions that
                                 // did not fit (|y| < 2^62 false); zeroed by the call
    const double *mass;          // [P]
    const double *attr;          // [A][P]
    int k[FLOW_PUSH_CHANNELS];             // the exponents k_c
    int A, L, V;                 // L = T + 1 (all the layers), or 1 (the state after the last interval)
};
struct FlowPushFinish {
    const unsigned long long *acc;
    const int *inv;              // caller vertex -> device vertex, or null
    double *out;                 // [A + 1][L][V], caller numbering
    double unscale[FLOW_PUSH_CHANNELS];    // 2^-k_c
    int A, L, V;
};
// What the sliding mode reads and writes besides.  The slide kernels write their five per-particle counters as the rows of ONE array
// and leave FlowArgs::o_status / o_rested / o_cross alone: five output pointers held in scalar registers through the loop made
// k_flow_slide_push<A> spill 12 - 18 of them.
struct FlowSlide {
    const double *area_f;        // [F] Dev::area_f, device numbering
    int *o_counts;               // [5][P]: status, rested, crossings, slides, steps (the turns of the inner loop)
};
int launch_flow(Ctx *c, const FlowArgs &a, const FlowSpan &s, const FlowPush *push, const FlowSlide *slide);      // push / slide: null without
int launch_flow_push_finish(Ctx *c, const FlowPushFinish &q);
void preload_flow_kernels();
// what dots_flow_map checks the caller's tables against, downloaded once per context
struct FlowHost {
    std::vector<int> tri;        // [F][3] device numbering
    std::vector<int> inv_f;      // caller triangle -> device triangle (empty: the same numbering)
};

// The one owner of device memory, and the one place that allocates and frees it: what a pool holds goes when it is released or
// destroyed.  A call that fails leaves the pool holding what it held before, or the new allocation as well: never a pointer nobody frees.
// Copies and fills go on the caller's stream (never the legacy default stream: another context of this process may be capturing a graph).
struct DevicePool {
    int device;
    explicit DevicePool(int dev) : device(dev) {}
    DevicePool(const DevicePool &) = delete;
    DevicePool &operator=(const DevicePool &) = delete;
    ~DevicePool() { release(); }
    // `count` elements (room for at least one, 8 bytes), zeroed on `stream` unless told otherwise
    template <typename T>
    int alloc(T **out, int64_t count, hipStream_t stream, bool zero = true) {
        const size_t n = sizeof(T) * (size_t)(count > 1 ? count : 1), bytes = n > 8 ? n : 8;
        held.reserve(held.size() + 1);      // (nothing below can fail between the allocation and its record)
        void *p = nullptr;
        DOTS_HIP(hipMalloc(&p, bytes));
        held.push_back(p);
        held_bytes += (int64_t)bytes;
        if (zero) DOTS_HIP(hipMemsetAsync(p, 0, bytes, stream));
        *out = (T *)p;
        return 0;
    }
    // device copy of `count` elements of a host array (null: zeros); the stream is synchronised: host buffers are borrowed for the call only
    template <typename T>
    int upload(const T **out, const T *host, int64_t count, hipStream_t stream) {
        T *p = nullptr;
        const int rc = alloc(&p, count, stream, host == nullptr);
        if (rc) return rc;
        if (host) DOTS_HIP(hipMemcpyAsync(p, host, sizeof(T) * (size_t)count, hipMemcpyHostToDevice, stream));
        DOTS_HIP(hipStreamSynchronize(stream));
        *out = p;
        return 0;
    }
    template <typename T>
    int upload(const T **out, const std::vector<T> &v, hipStream_t stream) { return upload(out, v.data(), (int64_t)v.size(), stream); }
    void release() {
        if (held.empty()) return;
        (void)hipSetDevice(device);
        for (void *p : held) (void)hipFree(p);
        held.clear();
        held_bytes = 0;
    }
    int64_t size() const { return (int64_t)held.size(); }
    int64_t bytes() const { return held_bytes; }

private:
    std::vector<void *> held;
    int64_t held_bytes = 0;
};

// ... and of pinned host memory
struct PinnedPool {
    PinnedPool() = default;
    PinnedPool(const PinnedPool &) = delete;
    PinnedPool &operator=(const PinnedPool &) = delete;
    ~PinnedPool() { release(); }
    template <typename T>
    int alloc(T **out, size_t count, unsigned flags) {
        held.reserve(held.size() + 1);
        void *p = nullptr;
        DOTS_HIP(hipHostMalloc(&p, sizeof(T) * count, flags));
        held.push_back(p);
        *out = (T *)p;
        return 0;
    }
    void release() {
        for (void *p : held) (void)hipHostFree(p);
        held.clear();
    }

private:
    std::vector<void *> held;
};

// What the two derived views of a context's device data hold besides `d` (pcg_view, time_view below).  Zero on one GPU, where both
// views ARE d; on a time slab build fills them (cg_x: dots_slab_set_buffers) and nothing else writes them.
struct PcgRecord {          // the PCG's view: this rank's mode count and sigma slice, its own vectors; same partition and pitch as the slab
    int cg_ncol = 0;
    const double *sigma = nullptr;
    double *cg_r = nullptr, *cg_z = nullptr, *cg_p0 = nullptr, *cg_p1 = nullptr, *cg_Ap = nullptr;
    double *cg_x = nullptr; // slab.x_send: the mode-space solution is written where the second all-gather reads it
};
struct TimeRecord {         // the transforms' view: the same pointers under the geometry of the whole time axis (pitch >= T + 1)
    int TP = 0, tp_shift = 0, t0 = 0, nl = 0, ni = 0, slab = 0, VT = 0, FT = 0, n_vtiles = 0, n_ftiles = 0;
};
// Where a right-hand-side launch that runs ahead of its iteration puts what the riding projection writes (z_fst, z_end, the cone
// multiplier), and the penalty it forms the boundary term with: laid over launch_rhs's own copy of the device data, never over the context's
struct RhsAhead {
    double *zf, *ze, *lamc;
    double r;
};

struct Ctx {
    Dev d{};                // the one stored view of the device data; pcg_view and time_view derive the other two
    // Multi-GPU: this context is one TIME SLAB of the problem.  Rank r holds the nodes [r * stride, r * stride + count) of
    // every state array (d: local pitch, t0, nl, ni) AND solves the time modes with the same indices (pcg_view).
    int shard_begin = 0;    // first node = first time mode of this context
    int shard_count = 0;    // nodes = modes of this context (may be 0 on trailing ranks)
    int shard_stride = 0;   // nodes per rank (same on every rank) = layout of the gathered buffers; 0 = not sharded
    int shard_ranks = 0;    // ranks with at least one node
    PcgRecord pcg{};
    TimeRecord gt{};
    dots_slab_buffers slab{};     // exchange buffers (caller's device memory, dots_slab_set_buffers)
    int64_t slab_b_chunk = 0;     // doubles one rank contributes to the right-hand-side all-gather: V * pitch
    int64_t slab_x_chunk = 0;     // ... to the all-gather of the mode-space solution: V * pitch + V (the last interval's cone multipliers)
    int slab_stage = 0;           // next stage dots_slab_stage expects
    dots_params prm{};
    int device;
    int lap_solver = 0;
    int nnz = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[12]{};
    double *stage = nullptr;      // device staging buffer (largest state array)
    int64_t stage_count = 0;
    double *h_pinned = nullptr;   // pinned host scalars
    double *h_mail = nullptr;     // coherent pinned host memory the device writes itself: [0, MAX_SUMS) sums, [MAX_SUMS] sequence number (fetch_sums)
    uint64_t mail_seq = 0;
    int *kkt_counter = nullptr;   // device counter of k_reduce_mail (last workgroup publishes)
    int64_t mail_spins = 20000000;   // host spins on the mailbox before it blocks on the stream (DOTS_MAIL_SPINS)
    int64_t mail_fallbacks = 0;   // evaluations whose sequence number never arrived: sums copied from the device scalars instead
    int mail_test_drop = 0;       // DOTS_MAIL_TEST_DROP=n (tests): every n-th evaluation publishes a wrong sequence number
    int front_rows = 1;           // row-per-lane-group sweep kernels on bands of short rows (DOTS_FRONT_ROWS: 0 never, 1 by rule, 2 wherever they fit)
    int front_leafinv = 1;        // DOTS_FRONT_LEAFINV=0: the leaves keep [L^-1 ; G] blocks like every other node; 2: local inverses, coupling read from the CSR (no records)
    int front_tune = 0;           // DOTS_FRONT_TUNE=1 print the per-band timing table, 2 also apply the fastest choice
    int *h_flags = nullptr;
    int n_partial_blocks = 0;
    int last_cg_iters = 0;        // iterations of the last solve (windowed: of its slowest window)
    int pcg_windows = 0;          // dots_pcg_windows: above 256 modes and without an enabled factor, step 1 solves the modes in windows of 256
    int pcg_windows_ran = 0;      // dots_debug_counter 14: windows of the last PCG solve (0: unwindowed), bit 8: the windowed transforms ran
    MgDev mg{};                   // multigrid preconditioner (nlev == 0: Jacobi only)
    int use_mg = 1;
    int mg_path = 0;              // MG_PATH_* of the last mg_vcycle (0: none since mg_release / dots_mg_enable(0))
    int64_t cg_path = 0;          // CG_PATH_* of the last PCG tiling handed to a launch (make_args, kernels_cg.hip; 0: none yet)
    int kkt_two = 1;              // KKT sums with two nodes per lane (one GPU; DOTS_KKT_TWO=0: one)
    // DOTS_STEP_TIMED: phase events of enqueue-only steps, collected later by dots_step_times (no host wait in the loop)
    static constexpr int TIME_SLOTS = 64;
    hipEvent_t tev[TIME_SLOTS][6]{};  // created on first use
    int tkind[TIME_SLOTS]{};      // 0 / 16: a whole dots_step iteration (6 events; 16: the projection rode in the right-hand-side launch), 1 + stage: one dots_slab_stage (events 0 and 1)
    int t_head = 0, t_count = 0;  // ring: oldest slot, slots in flight
    int step_timed = 0;           // dots_step_flags
    int step_skip_zmid = 0;       // dots_step_flags: steps leave z_mid unspecified (never written, rebuilt on the fly)
    int step_palm = 0;            // dots_step_flags: every iteration opens with the (q, lambda_c) closed form (is_palm = True)
    // What the context carries from one call to the next, and what each entry point does to it (admission.h).  A penalty update
    // (dots_adjust_penalty) is not carried out at once: the next iteration's kernels divide the five dual arrays as they read them
    // and steps 2+3 write them back divided (one pass over beta_mid saved: solver_socp.py:367-371 is 5 passes in the reference).
    Carried carried;
    int lazy_div = 1;             // DOTS_LAZY_DIV=0: divide at once (A/B measurements)
    int step_kkt = 0;             // dots_step_flags: steps 2+3 also form the KKT sums they hold in registers (kkt_fused)
    KktFused kkt_fused{};         // their per-workgroup partial sums (own buffer: d.partials serves the other reductions)
    int64_t kkt_fused_cap_v = 0, kkt_fused_cap_f = 0;   // workgroups the buffers hold per slot
    int step_carry = 0;           // dots_step_flags: steps 2+3 also store the next iteration's per-corner gathers (cn_sq, cn_g)
    // The launches around the direct solve at a pitch of 8, 16 or 32 have a form that keeps its loads in flight (k_rhs_modes2_deep: every
    // carried row of a vertex at once; k_time_modes_tile_fast) at the price of registers: taken while a CU gets few of the launch's workgroups
    int rhs_deep = -1;            // DOTS_RHS_DEEP: 0 never (the launches as they were), 1 wherever the kernels exist, -1 (default) the rule deep_launch_wins
    int n_cu = 0;                 // compute units of the device
    // z_mid on demand (one GPU, carry mapping): an iteration after which z_mid MAY be read (residuals read back, possibly the last one) does
    // not store it (18 T F values that are almost never read); instead steps 2+3 write the new beta_mid into z_mid's storage and the new B
    // into an alternate buffer and the pointers are swapped, so that the old B and beta_mid -- the pre-image of the projection, from which
    // z_mid = (lambda / D) * D (s_z/sqrt3 B_old - beta_mid_old) is rebuilt bit for bit (k_rebuild_zmid) -- survive until the next iteration.
    double *B_alt = nullptr;      // [3F][TP]
    double zmid_dv = 0.0, zmid_sz = 0.0;   // the penalty division that was pending during that step (0: none); scale_factor_z of that step
    int zmid_defer = 1;           // DOTS_ZMID_DEFER=0: store z_mid on those iterations as before (A/B measurements)
    FrontDev front{};             // multifrontal factor (n_nodes == 0: none)
    int use_front = 0;
    FrontSchedule sched{};        // what its installation decided about the sweeps
    dots_penalty_policy penalty_policy{};
    double ahead_dv = 0.0, ahead_r = 0.0;   // what the launch ahead anticipated
    int64_t penalty_ahead_started = 0, penalty_ahead_confirmed = 0;   // diagnostics (dots_debug_counter 2, 3)
    double *zf_alt = nullptr, *ze_alt = nullptr, *lamc_alt = nullptr;   // [V][TP] each (one GPU): written ahead, swapped in by the step that takes them
    // The factor's device memory.  What every sharer of it reads (factor, node records, maps, leaf inverses and tables, work lists) is in one
    // reference-counted store, created by front_setup and freed with its last holder (dots_front_share copies the pointer); W (update
    // planes) and the carried gathers are this context's own
    std::shared_ptr<DevicePool> front_store;
    DevicePool front_own;
    std::shared_ptr<FrontRecord> front_record;      // what front_setup planned, kept with the store: dots_move_vertices refreshes the factor from it
    int front_nr_max = 4;         // right-hand sides per launch of front_solve_many (DOTS_FRONT_NR: 2, 4 or 8)
    hipEvent_t ev_batch = nullptr;   // orders this context's stream against the others of a batched solve (created on first use)
    int front_cap_fault = 0;      // a multi-rhs launch was asked for more right-hand sides than its workgroup shape takes (front_solve_many reports it)
    int64_t front_many_launches = 0, front_many_split = 0;   // sweep launches of the last front_solve_many, those split below their chunk (dots_debug_counter 7, 8)
    uint64_t lap_hash_graph = 0;  // ... its state after rowptr and col (dots_move_vertices goes on from there)
    uint64_t tri_hash = 0;        // FNV-1a of triangles, corner_ptr and corner_idx: dots_move_vertices_many forms the triangle tables of all members from one scratch
    uint64_t lap_hash = 0;        // FNV-1a of the Laplacian (rowptr, col, val) and the vertex masses: dots_front_share compares it with the owner's
    int batched = 0;              // stepped by dots_step_many since its last dots_step: dots_penalty_ahead is refused
    // dots_readout: built on first use
    int *inv_perm_v = nullptr, *inv_perm_f = nullptr;   // caller vertex / triangle -> device row (null with the identity numbering)
    int readout_ready = 0;
    hipStream_t copy_stream = nullptr;   // device -> host copies of finished layer ranges, beside the launches of the next
    hipEvent_t ro_ev[8]{};        // one per chunk of 256 layers of mu (0-3) and E (4-7)
    double *h_ro_sums = nullptr;  // coherent pinned host memory the fold kernel writes: [layers][2]
    char *h_ring = nullptr;       // DOTS_READOUT_PINNED=<KB>: two pinned slots of that size the copies go through (A/B measurements)
    hipEvent_t ring_ev[2]{};
    int readout_pinned = 0;       // KB per slot; 0: copies go straight into the caller's memory
    int64_t d2h_bytes = 0;        // bytes copied device -> host by dots_download, dots_readout and dots_flow_map (dots_debug_counter 9)
    std::shared_ptr<FlowHost> flow;      // dots_flow_map: built on first use
    // dots_restart: what the parameters of a new context are formed from besides mu0 / mu1
    std::shared_ptr<std::vector<double>> mass_host;      // [V] vertex masses, device numbering (norm_boundary's loop)
    double norm_d0 = 0.0;         // norm_d as dots_create leaves it
    DevicePool mg_pool;           // the multigrid hierarchy (mg_release)
    // constants of the KKT normalisation (solver_socp.py:303-313)
    double c_prim_q = 0, c_prim_z = 0, c_dual_alpha = 0, c_dual_beta = 0, c_comp_rho = 0, c_comp_m = 0;
    DevicePool pool;              // what dots_create allocated and what the read-out added on first use: dots_device_bytes
    PinnedPool pinned;            // h_pinned, h_flags, h_mail, h_ro_sums, h_ring
    // hipGraph cache of the PCG iteration body: the context's own columns, and one per window of a windowed context
    CgCache cgc{};
    CgCache cgw[PCG_MAX_WINDOWS]{};
    void cg_graphs_release() {
        for (CgCache *k : {&cgc, &cgw[0], &cgw[1], &cgw[2], &cgw[3]})
            if (k->graph) { (void)hipGraphExecDestroy(k->graph); k->graph = nullptr; }
    }
    // The two places that move state pointers of `d` after build.  The taken launch ahead: the projection ran with the right-hand side
    // (RhsAhead), its results become the current z_fst, z_end and cone multiplier
    void swap_ahead_projection() {
        std::swap(d.zf, zf_alt);
        std::swap(d.ze, ze_alt);
        std::swap(d.lamc, lamc_alt);
    }
    RhsAhead ahead_target(double r) const { return RhsAhead{zf_alt, ze_alt, lamc_alt, r}; }
    // The deferred z_mid: steps 2+3 wrote the new B into B_alt and the new beta_mid into z_mid's storage.  Afterwards B_alt holds the B
    // the projection read, z_mid's storage the beta_mid it read, and B_st == B, bm_st == bm again
    void swap_deferred_zmid() {
        std::swap(d.B, B_alt);
        std::swap(d.bm, d.zm);
        d.B_st = d.B;
        d.bm_st = d.bm;
    }
    double *arr(int id) {
        double *t[12] = {d.phi, d.A, d.B, d.lam, d.zf, d.zm, d.ze, d.mu, d.E, d.bf, d.bm, d.be};
        return t[id];
    }
    explicit Ctx(int dev) : device(dev), front_own(dev), mg_pool(dev), pool(dev) {}
    Ctx(const Ctx &) = delete;
    Ctx &operator=(const Ctx &) = delete;
    // the one list of what a context owns (the caller has set the device: dots_create, dots_destroy)
    ~Ctx() {
        if (stream) (void)hipStreamSynchronize(stream);
        cg_graphs_release();
        mg_pool.release();
        front_own.release();
        pool.release();
        pinned.release();
        for (auto &e : ro_ev) if (e) (void)hipEventDestroy(e);
        for (auto &e : ring_ev) if (e) (void)hipEventDestroy(e);
        if (copy_stream) { (void)hipStreamSynchronize(copy_stream); (void)hipStreamDestroy(copy_stream); }
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
        if (ev_batch) (void)hipEventDestroy(ev_batch);
        front_store.reset();      // (a shared factor: freed with its last holder)
        for (auto &slot : tev)
            for (auto &e : slot) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// Which form of the time-mode transforms a pitch takes (the kernels are in kernels_modes.hip, their bodies and LDS sizes in modes_dev.h);
// the rules below, which dots_api.hip, kernels_cg.hip and kernels_alm.hip ask, are built from these three.
// T + 1 <= 256: a tile of rows and Q (in chunks of <= 32 KB) staged in LDS (k_time_modes_tile, k_rhs_modes)
inline bool time_modes_tile_ok(const Dev &d) { return d.TP <= BLOCK && d.VT >= 1; }
// T + 1 >= 64: the transforms are [V x (T+1)] x [(T+1) x (T+1)] fp64 GEMMs worth the matrix cores (k_time_modes_mfma)
inline bool time_modes_mfma_ok(const Dev &d) { return d.TP >= 64 && d.TP <= 256 && d.Qpad != nullptr; }
// pitch 8, 16 or 32 (all of Q is one chunk): the form with the pitch as a template argument (k_time_modes_tile_fast, k_rhs_modes2_deep)
inline bool time_modes_fast_ok(const Dev &d) { return (d.TP == 8 || d.TP == 16 || d.TP == 32) && d.VT * d.TP == TILE_ELEMS; }
// ... and whether a launch of `wgs` workgroups takes it (and the right-hand side its deep corner walk).  Side by side on tori at T = 31 the
// deep right-hand side is shorter at every size measured, by 30 % at 2 workgroups per CU and still by 12 % at 16
// (profiles/rhs_deep/threshold.txt); nothing was measured between 16 and torus100k's 24, where the launch moves its bytes at full
// occupancy, so the rule ends where the measurement does
constexpr int DEEP_WGS_PER_CU = 16;
inline bool deep_launch_wins(const Ctx *c, int wgs) {
    if (!time_modes_fast_ok(c->d) || c->rhs_deep == 0) return false;
    return c->rhs_deep == 1 || wgs <= DEEP_WGS_PER_CU * c->n_cu;
}
// direct solver on one GPU, T + 1 < 64: the inverse time transform of phi rides in the cone-projection launch (the
// projection reads neither phi nor anything the solve writes: steps 1-1 and 1-2 are a separable block)
inline bool soc_takes_inverse(const Ctx *c);
// direct solver on one GPU: the right-hand-side kernel writes the mode-space right-hand side itself
inline bool rhs_writes_modes(const Ctx *c) {
    return c->use_front && c->front.n_nodes > 0 && c->shard_stride == 0 && c->lap_solver == DOTS_LAP_MODAL_PCG && time_modes_tile_ok(c->d);
}

inline bool soc_takes_inverse(const Ctx *c) { return rhs_writes_modes(c) && !time_modes_mfma_ok(c->d); }
// Windowed modal PCG (dots_pcg_windows): one GPU, more than 256 modes, no enabled factor.  Mode space is then COMPACT: window k = modes
// [256 k, 256 k + 256) of a PCG vector is a [V][256] array at base + k V 256 (the windows of a pitch-512 / 1024 array fill it exactly).
inline bool pcg_windowed(const Ctx *c) {
    return c->pcg_windows && c->lap_solver == DOTS_LAP_MODAL_PCG && c->shard_stride == 0 && c->d.cg_ncol > PCG_WINDOW &&
           !(c->use_front && c->front.n_nodes > 0);
}
inline int pcg_window_count(const Dev &g) { return (g.cg_ncol + PCG_WINDOW - 1) / PCG_WINDOW; }
// the PCG kernels' view of window k: pitch 256, its own tiling, column count, sigma slice and vectors
inline Dev pcg_window_view(const Dev &g, int k) {
    Dev w = g;
    w.TP = PCG_WINDOW;
    w.tp_shift = PCG_WINDOW_SHIFT;
    w.VT = w.FT = TILE_ELEMS / PCG_WINDOW;
    w.n_vtiles = (g.V + w.VT - 1) / w.VT;
    w.n_ftiles = (3 * g.F + w.FT - 1) / w.FT;
    w.cg_ncol = g.cg_ncol - k * PCG_WINDOW < PCG_WINDOW ? g.cg_ncol - k * PCG_WINDOW : PCG_WINDOW;
    w.sigma = g.sigma + k * PCG_WINDOW;
    const int64_t off = (int64_t)k * g.V * PCG_WINDOW;
    w.cg_r = g.cg_r + off; w.cg_z = g.cg_z + off; w.cg_p0 = g.cg_p0 + off; w.cg_p1 = g.cg_p1 + off; w.cg_Ap = g.cg_Ap + off; w.cg_x = g.cg_x + off;
    return w;
}
// The PCG's view of a context: d with the PcgRecord laid over it (one GPU: d unchanged).  By value, like pcg_window_view: it carries d's
// pointers as they are now, whatever was swapped or installed since the record was filled.
inline Dev pcg_view(const Ctx *c) {
    Dev g = c->d;
    if (c->shard_stride == 0) return g;
    const PcgRecord &p = c->pcg;
    g.cg_ncol = p.cg_ncol; g.sigma = p.sigma;
    g.cg_r = p.cg_r; g.cg_z = p.cg_z; g.cg_p0 = p.cg_p0; g.cg_p1 = p.cg_p1; g.cg_Ap = p.cg_Ap; g.cg_x = p.cg_x;
    return g;
}
// ... and the view of the time transforms of a slab: d with the TimeRecord laid over it (one GPU: d unchanged)
inline Dev time_view(const Ctx *c) {
    Dev t = c->d;
    if (c->shard_stride == 0) return t;
    const TimeRecord &r = c->gt;
    t.TP = r.TP; t.tp_shift = r.tp_shift; t.t0 = r.t0; t.nl = r.nl; t.ni = r.ni; t.slab = r.slab;
    t.VT = r.VT; t.FT = r.FT; t.n_vtiles = r.n_vtiles; t.n_ftiles = r.n_ftiles;
    return t;
}
// the scalars of the PCG view a site may want alone: its mode count; its pitch is d's (PcgRecord)
inline int pcg_ncol(const Ctx *c) { return c->shard_stride == 0 ? c->d.cg_ncol : c->pcg.cg_ncol; }
// steps 2+3 can form the next iteration's per-corner gathers (k_q_lambda_mult_carry: whole triangles per 192-lane workgroup)
// (one GPU or a time slab; the direct solver's iteration)
inline bool carry_possible(const Ctx *c) {
    return c->d.cn_sq && c->d.TP >= 4 && c->d.TP <= 128 && c->use_front && c->front.n_nodes > 0 && c->lap_solver == DOTS_LAP_MODAL_PCG &&
           (rhs_writes_modes(c) || c->d.slab);
}

// a KKT evaluation of the conditions in `mask` reduces the sums the last steps-2+3 launch left (kernels_kkt.hip: kkt_sums) and reads no z_mid
inline bool kkt_takes_fused(const Ctx *c, uint32_t mask) {
    return c->carried.kkt_fused_valid && !(mask & ~(KKT_FUSED_MASK | 4u)) && c->h_mail && c->kkt_counter;
}

int64_t array_count_host(const Dev &d, int array_id);    // elements in the reference layout
int64_t array_count_device(const Dev &d, int array_id);  // elements in the device layout
int array_kind(int array_id);  // 0 node (T+1,V), 1 interval (T,V), 2 triangle (T+1,F,3), 3 corner (T,2,3,F,3)

#ifdef __HIPCC__
// ---- device helpers ---------------------------------------------------------------------
__device__ __forceinline__ int idxV(const Dev &d, int v, int t) { return (v << d.tp_shift) + t; }
__device__ __forceinline__ int64_t idxF(const Dev &d, int f, int c, int t) { return ((int64_t)(f * 3 + c) << d.tp_shift) + t; }
// t: LOCAL interval index (interval - t0), -1 <= t; the entry sits in the column of its node t + s
__device__ __forceinline__ int64_t idxM(const Dev &d, int fk, int s, int c, int t) {
    return ((int64_t)((fk * 2 + s) * 3 + c) << d.tp_shift) + t + s;
}
// two consecutive time columns of a row in one aligned 16-byte word (even first column)
// (DN<N>: the N consecutive time columns a lane owns, N = 2 that word, N = 1 one double; ldn / stn and their _nt forms below)
template <int N> struct DN { double v[N]; };
using D2 = DN<2>;
__device__ __forceinline__ D2 ld2(const double *p) { const double2 t = *reinterpret_cast<const double2 *>(p); return D2{{t.x, t.y}}; }
__device__ __forceinline__ void st2(double *p, const D2 &x) { *reinterpret_cast<double2 *>(p) = make_double2(x.v[0], x.v[1]); }
// the same with a streaming hint (non-temporal): data written once and read once by the next launch (the carried per-corner sums)
// or not read at all in the loop (z_mid on read-back iterations) should not displace the factor and beta_mid from the caches.
// (Measured in round 4, plain loads and stores against these: knot 9 720-10 020 -> 10 160-10 210 it/s, sphere10k 4 795-4 813 ->
// 4 936-4 983, torus100k 619 -> 631-646, knot63 unchanged; profiles/studies/r04_nontemporal.txt)
typedef double dots_d2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ D2 ld2_nt(const double *p) {
    const dots_d2v t = __builtin_nontemporal_load(reinterpret_cast<const dots_d2v *>(p));
    return D2{{t.x, t.y}};
}
__device__ __forceinline__ double ld1_nt(const double *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st2_nt(double *p, const D2 &x) {
    dots_d2v t;
    t.x = x.v[0];
    t.y = x.v[1];
    __builtin_nontemporal_store(t, reinterpret_cast<dots_d2v *>(p));
}
// a lane's N columns: 16-byte accesses for N = 2, 8-byte ones for N = 1
template <int N> __device__ __forceinline__ DN<N> ldn(const double *p) { if constexpr (N == 2) return ld2(p); else return DN<1>{{*p}}; }
template <int N> __device__ __forceinline__ DN<N> ldn_nt(const double *p) { if constexpr (N == 2) return ld2_nt(p); else return DN<1>{{ld1_nt(p)}}; }
template <int N> __device__ __forceinline__ void stn(double *p, const DN<N> &x) { if constexpr (N == 2) st2(p, x); else *p = x.v[0]; }
template <int N> __device__ __forceinline__ void stn_nt(double *p, const DN<N> &x) { if constexpr (N == 2) st2_nt(p, x); else __builtin_nontemporal_store(x.v[0], p); }
// slab predicates for local column t
__device__ __forceinline__ bool first_node(const Dev &d, int t) { return d.t0 + t == 0; }       // global node 0
__device__ __forceinline__ bool last_node(const Dev &d, int t) { return d.t0 + t == d.T; }      // global node T
__device__ __forceinline__ bool has_prev_interval(const Dev &d, int t) { return d.t0 + t > 0; } // interval t - 1 exists
// node t + 1 of a node array x (halo when it belongs to the next slab)
__device__ __forceinline__ double next_node(const Dev &d, const double *x, const double *hi, int64_t row, int t) {
    return (t + 1 < d.nl) ? x[(row << d.tp_shift) + t + 1] : hi[row];
}

// Blocks are dealt round-robin over the 8 XCDs (b and b+8 share an L2).  Give every XCD one
// contiguous range of tiles so that neighbouring tiles, which gather the same rows, share an L2.
__device__ __forceinline__ int xcd_tile(int b, int n_tiles) {
    int per = (n_tiles + 7) >> 3;
    return (b & 7) * per + (b >> 3);
}
inline int xcd_grid(int n_tiles) { return ((n_tiles + 7) / 8) * 8; }

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;
}

// Sum N per-thread values over the workgroup; thread 0 gets the totals.  Fixed order -> deterministic.
template <int N, int NW = 4>
__device__ __forceinline__ void block_sum(double (&v)[N], double *lds /* [N*4] */) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = wave_sum(v[i]);
        if (lane == 0) lds[i * 4 + w] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = NW == 4 ? (lds[i * 4] + lds[i * 4 + 1]) + (lds[i * 4 + 2] + lds[i * 4 + 3]) : (lds[i * 4] + lds[i * 4 + 1]) + lds[i * 4 + 2];
    }
}
#endif

}  // namespace dots

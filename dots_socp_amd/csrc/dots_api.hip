// C ABI of libdotsocp_hip.so (see include/dots_socp_hip.h): context lifecycle, state transfer,
// the ALM step driver.  Everything here is host code around the kernels of kernels_*.hip.
#include "dots_dev.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

struct dots_ctx : dots::Ctx { using Ctx::Ctx; };

namespace dots {

static thread_local std::string g_last_error;

void set_error(const std::string &msg) { g_last_error = msg; }

int hip_fail(hipError_t e, const char *what, const char *file, int line) {
    char buf[512];
    snprintf(buf, sizeof buf, "HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
    set_error(buf);
    return DOTS_ERR_HIP;
}

// An integer switch from the environment: unset keeps *out; anything that is not an integer in [lo, hi] is an error.
bool env_int(const char *name, int lo, int hi, int *out) {
    const char *e = getenv(name);
    if (!e) return true;
    char *end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end == e || *end != '\0' || v < lo || v > hi) {
        char buf[256];
        snprintf(buf, sizeof buf, "environment: %s=%s is not an integer in [%d, %d]", name, e, lo, hi);
        set_error(buf);
        return false;
    }
    *out = (int)v;
    return true;
}

int array_kind(int id) {
    switch (id) {
        case DOTS_PHI: return 0;
        case DOTS_B: case DOTS_E: return 2;
        case DOTS_Z_MID: case DOTS_BETA_MID: return 3;
        default: return 1;
    }
}
int64_t array_count_host(const Dev &d, int id) {
    switch (array_kind(id)) {      // a time slab exchanges its own time extent (corner arrays: one block per node)
        case 0: return (int64_t)d.nl * d.V;
        case 1: return (int64_t)d.ni * d.V;
        case 2: return (int64_t)d.nl * d.F * 3;
        default: return (int64_t)(d.slab ? d.nl : d.ni) * 18 * d.F;
    }
}
int64_t array_count_device(const Dev &d, int id) {
    switch (array_kind(id)) {
        case 0: case 1: return (int64_t)d.V << d.tp_shift;
        case 2: return ((int64_t)3 * d.F) << d.tp_shift;
        default: return ((int64_t)18 * d.F) << d.tp_shift;
    }
}

// the context's own arrays (Ctx::pool): zeroed, or the device copy of a host array
template <typename T>
static int dev_alloc(Ctx *c, T **out, int64_t count) { return c->pool.alloc(out, count, c->stream); }
template <typename T>
static int dev_upload(Ctx *c, const T **out, const T *host, int64_t count) { return c->pool.upload(out, host, count, c->stream); }

// norm_boundary = r h sqrt(norm_square_center(boundary / mass)) at r = 1 (solver_socp.py:296) from the end masses: the sum in vertex
// order on the host (dots_create, dots_restart with host arrays: one loop, the same bits), the norm from a sum however it was formed
static double boundary_sum(const double *mu0, const double *mu1, const double *mass, int V) {
    double nb = 0.0;
    for (int v = 0; v < V; ++v) nb += (mu0[v] * mu0[v] + mu1[v] * mu1[v]) / mass[v];
    return nb;
}
static double boundary_norm(double nb, int T) { return std::sqrt(nb / (T + 1)); }

// The host constants of a run on the geometry tables `mass` (V), `area` (F) and `val` (nnz), for the n contexts cs[0 .. n) that hold
// them (dots_create: one; a move: every holder of the factor, the sums formed once): the hash of what the factor is built from,
// continued from the graph's (dots_front_share); the KKT normalisation constants (solver_socp.py:303-313), means of the broadcast
// weight arrays summed in index order; norm_d; the masses dots_restart forms norm_boundary from; norm_boundary of cs[k]'s end masses
// ends[2 k], ends[2 k + 1].
static void run_constants(Ctx *const *cs, int n, const std::shared_ptr<std::vector<double>> &mass, const double *area, const double *val,
                          const double *const *ends) {
    const int V = cs[0]->d.V, F = cs[0]->d.F;
    uint64_t h = cs[0]->lap_hash_graph;
    auto mix = [&h](const void *data, size_t bytes) {
        const unsigned char *b = static_cast<const unsigned char *>(data);
        for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    };
    mix(val, sizeof(double) * (size_t)cs[0]->nnz);
    mix(mass->data(), sizeof(double) * (size_t)V);
    double sm = 0.0, sa = 0.0;
    for (int v = 0; v < V; ++v) sm += (*mass)[(size_t)v];
    for (int f = 0; f < F; ++f) sa += area[f];
    const double mean_v = sm / V, mean_f = sa / F;
    for (int k = 0; k < n; ++k) {
        Ctx *c = cs[k];
        c->lap_hash = h;
        c->c_prim_q = 0.5 * (mean_v + mean_f);
        c->c_prim_z = (mean_v + mean_f + mean_v) / 3.0;
        c->c_dual_alpha = mean_v;
        c->c_dual_beta = 0.5 * (mean_v + mean_f);
        c->c_comp_rho = mean_v;
        c->c_comp_m = mean_f;
        c->prm.norm_d = c->norm_d0 = std::sqrt(2.0 * sa);
        c->mass_host = mass;
        c->prm.norm_boundary = boundary_norm(boundary_sum(ends[2 * k], ends[2 * k + 1], mass->data(), V), c->d.T);
    }
}

// The parameters a run starts from, in dots_create and in dots_restart (tau, eps and the PCG's tolerance and cap are the caller's)
static void fresh_run_params(Ctx *c) {
    dots_params &q = c->prm;
    q.r = 1.0; q.scale_z = 1.0; q.const_d = 1.0;
    q.congestion = 0.0; q.prim_scale = 1.0; q.dual_scale = 1.0; q.boundary_scale = 1.0;
}

static int build(Ctx *c, const dots_problem_desc *p) {
    Dev &d = c->d;
    d.T = p->n_time;
    d.V = p->n_vertices;
    d.F = p->n_triangles;
    int tpg = 8, shg = 3;                     // global pitch: power of two >= T + 1
    while (tpg < d.T + 1) { tpg <<= 1; ++shg; }
    if (tpg > TILE_ELEMS) { set_error("n_time too large: T+1 must be <= 1024"); return DOTS_ERR_ARGUMENT; }
    const bool sharded = p->slab_count > 0 || p->slab_stride > 0;
    // the modal context takes T + 1 <= 1024 on one GPU; above 256 only the direct solver steps it (modal_needs_factor), and time
    // slabs keep T + 1 <= 256 (their scalar and halo layouts)
    if (p->lap_solver == DOTS_LAP_MODAL_PCG && sharded && tpg > BLOCK) { set_error("time slabs need T + 1 <= 256"); return DOTS_ERR_ARGUMENT; }
    d.t0 = 0; d.nl = d.T + 1; d.ni = d.T; d.slab = 0;
    int tp = tpg, sh = shg;
    if (sharded) {
        if (p->lap_solver != DOTS_LAP_MODAL_PCG || p->slab_stride < 1 || p->slab_begin < 0 || p->slab_count < 0 ||
            p->slab_begin + p->slab_count > d.T + 1 || p->slab_count > p->slab_stride ||
            (p->slab_count > 0 && p->slab_begin % p->slab_stride != 0) ||
            (p->slab_count < p->slab_stride && p->slab_count > 0 && p->slab_begin + p->slab_count != d.T + 1)) {
            set_error("bad time slab (needs the modal solver, begin = rank * stride, 0 <= count <= stride, a short slab only at the end)");
            return DOTS_ERR_ARGUMENT;
        }
        c->shard_begin = p->slab_begin;
        c->shard_count = p->slab_count;
        c->shard_stride = p->slab_stride;
        c->shard_ranks = (d.T + 1 + p->slab_stride - 1) / p->slab_stride;
        tp = 4; sh = 2;                       // local pitch: power of two >= the nodes per rank
        while (tp < p->slab_stride) { tp <<= 1; ++sh; }
        d.t0 = p->slab_begin; d.nl = p->slab_count; d.slab = 1;
        d.ni = std::max(0, std::min(d.nl, d.T - d.t0));
    }
    d.TP = tp;
    d.tp_shift = sh;
    if (((int64_t)d.V << sh) >= ((int64_t)1 << 31)) {      // node arrays are indexed with 32-bit arithmetic (idxV)
        set_error("V * time pitch must stay below 2^31 per context: cut the time axis into more slabs");
        return DOTS_ERR_ARGUMENT;
    }
    d.VT = d.FT = TILE_ELEMS / tp;
    d.n_vtiles = (d.V + d.VT - 1) / d.VT;
    d.n_ftiles = (3 * d.F + d.FT - 1) / d.FT;
    d.h = 1.0 / d.T;
    d.cg_ncol = d.T + 1;
    c->nnz = p->lap_nnz;
    {   // what the factor is built from, in this numbering (dots_front_share)
        uint64_t h = 1469598103934665603ull;
        auto mix = [&h](const void *data, size_t bytes) {
            const unsigned char *b = static_cast<const unsigned char *>(data);
            for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
        };
        mix(p->lap_rowptr, sizeof(int32_t) * ((size_t)p->n_vertices + 1));
        mix(p->lap_col, sizeof(int32_t) * (size_t)p->lap_nnz);
        c->lap_hash_graph = h;      // (lap_hash continues it over the values: run_constants)
        h = 1469598103934665603ull;
        mix(p->triangles, sizeof(int32_t) * 3 * (size_t)p->n_triangles);
        mix(p->corner_ptr, sizeof(int32_t) * ((size_t)p->n_vertices + 1));
        mix(p->corner_idx, sizeof(int32_t) * (size_t)p->n_corners);
        c->tri_hash = h;
    }
    c->lap_solver = p->lap_solver;

    const int V = d.V, F = d.F, nC = p->n_corners;
    // host-side derived per-corner tables (constants of solver_socp.py:172-192 kept per corner, never broadcast)
    std::vector<double> cD(nC), cgA((size_t)nC * 3), cArea(nC), kdiag(V, 0.0);
    for (int v = 0; v < V; ++v) {
        for (int j = p->corner_ptr[v]; j < p->corner_ptr[v + 1]; ++j) {
            const int fk = p->corner_idx[j], f = fk / 3;
            if (f < 0 || f >= F || p->triangles[fk] != v) { set_error("corner list inconsistent with triangles"); return DOTS_ERR_ARGUMENT; }
            cD[j] = std::sqrt(p->area_tri[f] / p->mass_vert[v]);
            cArea[j] = p->area_tri[f];
            for (int cc = 0; cc < 3; ++cc) cgA[(size_t)j * 3 + cc] = p->hat_grad[(size_t)fk * 3 + cc] * p->area_tri[f];
        }
        bool has_diag = false;
        for (int j = p->lap_rowptr[v]; j < p->lap_rowptr[v + 1]; ++j) {
            if (p->lap_col[j] < 0 || p->lap_col[j] >= V) { set_error("lap_col out of range"); return DOTS_ERR_ARGUMENT; }
            if (p->lap_col[j] == v) { kdiag[v] += p->lap_val[j]; has_diag = true; }
        }
        if (!has_diag || !(kdiag[v] > 0.0)) { set_error("surface stiffness matrix needs a positive diagonal"); return DOTS_ERR_ARGUMENT; }
    }
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < 3; ++k)
            if (p->triangles[f * 3 + k] < 0 || p->triangles[f * 3 + k] >= V) { set_error("triangle index out of range"); return DOTS_ERR_ARGUMENT; }

    int rc = 0;
#define UP(field, src, n) if ((rc = dev_upload(c, &d.field, src, (int64_t)(n)))) return rc
    UP(tri, p->triangles, F * 3);
    UP(hat, p->hat_grad, F * 9);
    UP(area_f, p->area_tri, F);
    UP(mass_v, p->mass_vert, V);
    UP(cptr, p->corner_ptr, V + 1);
    UP(cidx, p->corner_idx, nC);
    UP(c_D, cD.data(), nC);
    {
        std::vector<double> fkD((size_t)nC);
        for (int j = 0; j < nC; ++j) fkD[(size_t)p->corner_idx[j]] = cD[(size_t)j];
        UP(fk_D, fkD.data(), nC);
    }
    {
        std::vector<int> cpos((size_t)nC);
        for (int j = 0; j < nC; ++j) cpos[(size_t)p->corner_idx[j]] = j;
        UP(cpos, cpos.data(), nC);
    }
    UP(c_gA, cgA.data(), nC * 3);
    UP(c_area, cArea.data(), nC);
    UP(rowptr, p->lap_rowptr, V + 1);
    UP(col, p->lap_col, p->lap_nnz);
    UP(val, p->lap_val, p->lap_nnz);
    UP(kdiag, kdiag.data(), V);
    UP(mu0, p->mu0, V);
    UP(mu1, p->mu1, V);
    if (p->perm_vert) UP(perm_v, p->perm_vert, V);
    if (p->perm_tri) UP(perm_f, p->perm_tri, F);
    if (p->lap_solver == DOTS_LAP_MODAL_PCG) {
        if (!p->time_modes || !p->time_eigs) { set_error("modal solver needs time_modes and time_eigs"); return DOTS_ERR_ARGUMENT; }
        UP(Q, p->time_modes, (d.T + 1) * (d.T + 1));
        {
            const int n = d.T + 1;
            std::vector<double> qp((size_t)tpg * tpg, 0.0), qt((size_t)tpg * tpg, 0.0);
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) {
                    qp[(size_t)i * tpg + j] = p->time_modes[i * n + j];
                    qt[(size_t)j * tpg + i] = p->time_modes[i * n + j];
                }
            UP(Qpad, qp.data(), (int64_t)tpg * tpg);
            UP(QpadT, qt.data(), (int64_t)tpg * tpg);
        }
        std::vector<double> sig(tpg, 0.0);
        for (int i = 0; i <= d.T; ++i) sig[i] = p->time_eigs[i];
        UP(sigma, sig.data(), tpg);
    }
#undef UP

    double **state[12] = {&d.phi, &d.A, &d.B, &d.lam, &d.zf, &d.zm, &d.ze, &d.mu, &d.E, &d.bf, &d.bm, &d.be};
    for (int id = 0; id < DOTS_N_ARRAYS; ++id)
        if ((rc = dev_alloc(c, state[id], array_count_device(d, id)))) return rc;
    const int64_t nnode = (int64_t)V << sh;
    if (!sharded && (rc = dev_alloc(c, &d.cg_b, nnode))) return rc;      // a slab writes its right-hand side into slab.b_send
    if ((rc = dev_alloc(c, &d.lamc, nnode))) return rc;
    if (!sharded && ((rc = dev_alloc(c, &c->zf_alt, nnode)) || (rc = dev_alloc(c, &c->ze_alt, nnode)) || (rc = dev_alloc(c, &c->lamc_alt, nnode)))) return rc;
    if (!sharded && c->zmid_defer && p->lap_solver == DOTS_LAP_MODAL_PCG && (rc = dev_alloc(c, &c->B_alt, array_count_device(d, DOTS_B)))) return rc;
    d.B_st = d.B;
    d.bm_st = d.bm;
    if (sharded) {
        double *hv = nullptr;
        if ((rc = dev_alloc(c, &hv, V))) return rc;
        d.phi_hi = hv;
    }
    if (!sharded) {
        double **cgv[6] = {&d.cg_r, &d.cg_z, &d.cg_p0, &d.cg_p1, &d.cg_Ap, &d.cg_x};
        for (auto q : cgv)
            if ((rc = dev_alloc(c, q, nnode))) return rc;
    }
    const int gv = xcd_grid(d.n_vtiles), gf = xcd_grid(d.n_ftiles);
    // KKT kernels: one workgroup per quarter tile, N_VSUMS + N_FSUMS <= MAX_SUMS slots each
    const int64_t npart = std::max<int64_t>({(int64_t)MAX_SUMS * std::max(gv, gf) * (TILE_ELEMS / BLOCK) * 2, cg_partials_needed(d), 4096});
    if ((rc = dev_alloc(c, &d.partials, npart))) return rc;
    if ((rc = dev_alloc(c, &d.scal, CgScalOffsets::TOTAL))) return rc;
    if ((rc = dev_alloc(c, &d.flags, FLAG_TOTAL))) return rc;
    if (!sharded && tp >= 4) {      // DOTS_STEP_KKT_SUMS: per-workgroup partial sums of the steps-2+3 launch (carry or tile mapping)
        const int64_t tw = tp <= 128 ? (2 * 192 / tp) / 3 : 1;
        c->kkt_fused_cap_v = gv;
        c->kkt_fused_cap_f = xcd_grid((int)((F + tw - 1) / tw));
        if ((rc = dev_alloc(c, &c->kkt_fused.part_v, (int64_t)N_VSUMS * c->kkt_fused_cap_v))) return rc;
        if ((rc = dev_alloc(c, &c->kkt_fused.part_f, (int64_t)N_FSUMS * c->kkt_fused_cap_f))) return rc;
    }
    c->stage_count = array_count_device(d, DOTS_Z_MID);
    if ((rc = dev_alloc(c, &c->stage, c->stage_count))) return rc;
    if ((rc = c->pinned.alloc(&c->h_pinned, CgScalOffsets::TOTAL, hipHostMallocDefault))) return rc;
    if ((rc = c->pinned.alloc(&c->h_flags, FLAG_TOTAL, hipHostMallocDefault))) return rc;
    if ((rc = dev_alloc(c, &c->kkt_counter, 2))) return rc;
    if ((rc = c->pinned.alloc(&c->h_mail, MAX_SUMS + 8, hipHostMallocCoherent | hipHostMallocMapped))) return rc;
    for (int i = 0; i < MAX_SUMS + 8; ++i) c->h_mail[i] = 0.0;

    // what the PCG's view and, on a slab, the global-time view of the transforms hold besides d (pcg_view, time_view)
    if (sharded) {
        PcgRecord &g = c->pcg;     // modes [shard_begin, shard_begin + shard_count): same partition, same pitch as the slab
        g.cg_ncol = p->slab_count;
        std::vector<double> sig(tp, 0.0);
        for (int i = 0; i < p->slab_count; ++i) sig[i] = p->time_eigs[p->slab_begin + i];
        if ((rc = dev_upload(c, &g.sigma, sig.data(), tp))) return rc;
        double **cgv[5] = {&g.cg_r, &g.cg_z, &g.cg_p0, &g.cg_p1, &g.cg_Ap};     // cg_x = slab.x_send (dots_slab_set_buffers)
        for (auto q : cgv)
            if ((rc = dev_alloc(c, q, nnode))) return rc;
        TimeRecord &t = c->gt;
        t.TP = tpg; t.tp_shift = shg; t.t0 = 0; t.nl = d.T + 1; t.ni = d.T; t.slab = 0;
        t.VT = t.FT = TILE_ELEMS / tpg;
        t.n_vtiles = (d.V + t.VT - 1) / t.VT;
        t.n_ftiles = (3 * d.F + t.FT - 1) / t.FT;
        c->slab_b_chunk = nnode;
        c->slab_x_chunk = nnode + V;
    }

    const double *const ends[2] = {p->mu0, p->mu1};
    run_constants(&c, 1, std::make_shared<std::vector<double>>(p->mass_vert, p->mass_vert + V), p->area_tri, p->lap_val, ends);
    fresh_run_params(c);
    c->prm.tau = 1.9; c->prm.eps = 0.0; c->prm.cg_tol = 1e-8; c->prm.cg_max_iter = 20000;
    DOTS_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// The runtime's side of admission.h: every entry point opens with admit(c, E_...); what reads z_mid from memory says need_zmid
static const Runtime RUNTIME = {
    [](void *ctx) -> int {
        const hipError_t e = hipSetDevice(static_cast<Ctx *>(ctx)->device);
        return e == hipSuccess ? 0 : hip_fail(e, "hipSetDevice", __FILE__, __LINE__);
    },
    [](void *ctx, double factor) -> int { return launch_adjust_penalty(static_cast<Ctx *>(ctx), factor); },
    [](void *ctx) -> int { return launch_rebuild_zmid(static_cast<Ctx *>(ctx)); }};
static int admit(Ctx *c, Entry e) { return admit(c ? &c->carried : nullptr, e, RUNTIME, c); }
static int need_zmid(Ctx *c, Entry e, bool argument = true) { return need_zmid(c->carried, e, RUNTIME, c, argument); }
static int flush_division(Ctx *c) { return flush_division(c->carried, RUNTIME, c); }

// The modal PCG keeps per-mode scalars for NC <= CgScalOffsets::NCMAX = 256 modes: a modal context of T + 1 > 256 steps with the
// direct solver only (a factor installed or shared, and enabled), unless the caller switched the windowed PCG on (dots_pcg_windows).
static int modal_needs_factor(const Ctx *c, const char *what) {
    if (c->lap_solver != DOTS_LAP_MODAL_PCG || pcg_ncol(c) <= CgScalOffsets::NCMAX || (c->use_front && c->front.n_nodes > 0)) return 0;
    if (pcg_windowed(c)) return 0;      // dots_pcg_windows: the PCG takes the modes in windows of 256
    set_error(std::string(what) + ": T + 1 > 256 needs the direct solver (dots_front_setup); the modal PCG takes T + 1 <= 256");
    return DOTS_ERR_STATE;
}

// first half of an iteration: right-hand side + solve (for this context's modes)
static int palm_step0(Ctx *c) {
    if (!c->step_palm) return 0;
    if (int rc = refuse_unspecified_zmid(c->carried, E_STEP)) return rc;
    c->carried.drop_for_step0();
    return launch_q_lambda_only(c);
}

// ---- time slabs: the stages of one iteration (include/dots_socp_hip.h, dots_slab_stage) ---------------------------
__global__ __launch_bounds__(BLOCK) void k_slab_append_multiplier(Dev d, double *__restrict__ tail) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    // the cone multiplier of the interval that ends at the next slab's first node
    if (v < d.V) tail[v] = (d.ni == d.nl && d.nl > 0) ? d.lamc[idxV(d, v, d.nl - 1)] : 0.0;
}

// dots_upload of phi with the next slab's first node as one more row (reference layout: vertex v of the host is row perm_v^-1 here)
__global__ __launch_bounds__(BLOCK) void k_slab_phi_hi(Dev d, const double *__restrict__ row, double *__restrict__ phi_hi) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < d.V) phi_hi[i] = row[d.perm_v ? d.perm_v[i] : i];
}

static int slab_stage(Ctx *c, int stage) {
    int rc;
    const Dev &d = c->d;
    switch (stage) {
        case 0:       // [is_palm: step 0]; halos for the right-hand side and the projection
            if (d.nl > 0 && (rc = palm_step0(c))) return rc;
            return launch_slab_pack_iteration(c);
        case 1:       // right-hand side of this slab's nodes -> b_send, and the cone projection of its intervals (one launch)
        case 6:       // ... the right-hand side alone: the caller starts the all-gather of b behind it and enqueues stage 5
        case 5:       // ... the cone projection alone (it reads nothing the right-hand side or the solve writes); the multipliers of
                      //     the slab's last interval go to the tail of x_send: the NEXT slab's steps 2+3 need them, after the solve
            if (d.nl > 0) {
                if (stage == 5) { if ((rc = launch_soc_projection(c, 1, false))) return rc; }
                else if ((rc = launch_rhs(c, stage == 1))) return rc;
                if (stage != 6) {
                    hipLaunchKernelGGL(k_slab_append_multiplier, dim3((d.V + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, d,
                                       c->slab.x_send + ((int64_t)d.V << d.tp_shift));
                    DOTS_HIP(hipGetLastError());
                }
            }
            return 0;
        case 2:       // forward transform of this rank's modes + solve -> x_send
            return cg_solve(c, nullptr);
        case 3:       // inverse transform for this slab, steps 2 and 3
            if ((rc = cg_finish_sharded(c))) return rc;
            c->carried.stepped(c->step_skip_zmid);
            state_changed(c->carried);
            if (d.nl == 0) return 0;
            return launch_q_lambda_mult(c, c->step_skip_zmid ? 2 : 1);
        case 4:       // halos of the KKT kernels
            c->carried.kkt_halo_fresh = 1;
            return launch_slab_pack_kkt(c);
        default:
            set_error("slab_stage: unknown stage");
            return DOTS_ERR_ARGUMENT;
    }
}

// a free slot of the timing ring (its events created on first use), or nullptr when the ring is full: the step is then not timed
constexpr int TKIND_FUSED = 16;      // tkind of a whole iteration whose projection rode in the right-hand-side launch
static hipEvent_t *time_slot(Ctx *c, int kind) {
    if (!c->step_timed || c->t_count >= Ctx::TIME_SLOTS) return nullptr;
    const int s = (c->t_head + c->t_count) % Ctx::TIME_SLOTS;
    for (auto &e : c->tev[s])
        if (!e && hipEventCreate(&e) != hipSuccess) return nullptr;
    c->tkind[s] = kind;
    c->t_count += 1;
    return c->tev[s];
}

// the milliseconds of one stage of a slab's iteration, booked where dots_slab_stage (with stats) and dots_step_times report them
static void book_stage(dots_step_stats &st, int stage, float t) {
    st.ms_total = t;
    if (stage == 0 || stage == 6) st.ms_rhs = t;                // packing the halos; the right-hand side alone
    if (stage == 5) st.ms_soc = t;
    if (stage == 1) st.ms_rhs = st.ms_soc = 0.5 * t;            // one launch: right-hand side and projection together
    if (stage == 2) st.ms_laplacian = t;
    if (stage == 3) { st.ms_q_lambda_multiplier = t; st.alm_iterations = 1; }
}

// What the first half of an iteration decided, for its second half (iteration_before / iteration_after)
struct IterPlan {
    double dv = 0.0;          // a pending penalty division the iteration's kernels apply as they read
    int zmode = 1;            // steps 2+3: 1 store z_mid, 2 skip it
    int ahead_kind = 0;       // the right-hand side (1) / and the projection (2) were enqueued ahead (DOTS_STEP_RHS_AHEAD)
    bool fused_rhs = false;   // the projection rides in the right-hand-side launch
    bool fuse = false;        // the projection takes the inverse time transform
};

// First half of an enqueue-only iteration, up to the right-hand side of step 1 (dots_step and dots_step_many); `timed`: the caller
// brackets the phases with events and waits (no division rides in the kernels then).  The solve follows: cg_solve, or in a batch the
// time transform, front_solve_many and the inverse transform.
static int iteration_before(Ctx *c, bool timed, IterPlan &p, hipEvent_t *tv) {
    int rc;
#define MARK(i) do { if (tv) DOTS_HIP(hipEventRecord(tv[i], c->stream)); } while (0)
    MARK(0);
    Carried &k = c->carried;
    if (k.zmid == ZMID_DEFERRED) {      // nobody asked for the last iterate's z_mid: its storage (holding the old beta_mid) is simply stale
        if (c->step_palm) { if ((rc = rebuild_zmid(k, RUNTIME, c))) return rc; }      // (step 0 reads z_mid)
        else k.zmid = ZMID_UNSPECIFIED;
    }
    // a pending penalty division rides in this iteration's kernels when both of them can apply it; otherwise it is carried out first
    p.zmode = c->step_skip_zmid ? 2 : 1;
    p.dv = 0.0;
    if (k.pending_div != 0.0) {
        if (!timed && !c->step_palm && k.rhs_ahead == 2 && k.ahead_div == k.pending_div && ql_divides(c, p.zmode)) {
            p.dv = k.pending_div;      // the launch ahead (penalty_decision_ahead) divided as it read: steps 2+3 do the same and write back divided
            k.pending_div = 0.0;
        } else if (!timed && !c->step_palm && !k.rhs_ahead && rhs_divides(c) && ql_divides(c, p.zmode)) {
            p.dv = k.pending_div;
            k.pending_div = 0.0;
        } else if ((rc = flush_division(c))) return rc;      // (a launch ahead that divided as it read saw the values the arrays now hold)
    }
    k.ahead_div = 0.0;
    if ((rc = palm_step0(c))) return rc;
    // the right-hand side of this iteration was enqueued behind the KKT kernels of the last one (DOTS_STEP_RHS_AHEAD) and nothing
    // it reads has changed since: start at the solve; the projection then runs with the inverse transform
    p.ahead_kind = (c->step_palm || k.rhs_ahead > 2) ? 0 : k.rhs_ahead;      // (3, 4: an anticipated penalty update the caller did not confirm)
    const bool ahead = p.ahead_kind != 0;
    k.rhs_ahead = 0;
    if (p.ahead_kind == 2) c->swap_ahead_projection();      // the projection ran ahead too: its results become the current z_fst, z_end and cone multiplier
    if (timed) return 0;      // (the timed path of run_iteration_body goes on itself)
    k.stepped(c->step_skip_zmid);
    p.fused_rhs = rhs_writes_modes(c) && !ahead;      // [right-hand side + projection] -> sweeps -> inverse transform -> steps 2+3
    p.fuse = !p.fused_rhs && soc_takes_inverse(c) && p.ahead_kind != 2;
    if (p.fused_rhs) { if ((rc = launch_rhs(c, true, p.dv))) return rc; }
    else if (!ahead && (rc = launch_rhs(c))) return rc;
    MARK(1);
    return 0;
}

// Second half, behind the solve: the projection (unless it rode in the right-hand side or ran ahead) and steps 2+3
static int iteration_after(Ctx *c, const IterPlan &p, hipEvent_t *tv) {
    int rc;
    MARK(2);
    if (p.fused_rhs) {
        MARK(3);      // (no separate projection launch: dots_step_times splits the first phase between ms_rhs and ms_soc)
        if ((rc = launch_q_lambda_mult(c, p.zmode, p.dv))) return rc;
        MARK(4);
        MARK(5);      // back to back with 4: what one event costs on the stream, taken off every phase (dots_step_times)
        if (tv) c->tkind[(c->t_head + c->t_count - 1) % Ctx::TIME_SLOTS] = TKIND_FUSED;
        return 0;
    }
    if (p.ahead_kind != 2 && (rc = launch_soc_projection(c, 1, p.fuse))) return rc;
    MARK(3);
    if ((rc = launch_q_lambda_mult(c, p.zmode, p.dv))) return rc;
    MARK(4);
    MARK(5);
    return 0;
#undef MARK
}

static int run_iteration_body(Ctx *c, dots_step_stats *st, hipEvent_t *tv) {
    int rc;
    IterPlan p;
    if ((rc = iteration_before(c, st != nullptr, p, tv))) return rc;
    if (!st) {   // asynchronous: enqueue only (the direct solver needs no host round trip); nothing is timed
        if ((rc = cg_solve(c, nullptr, p.fuse))) return rc;
        return iteration_after(c, p, tv);
    }
    const int ahead_kind = p.ahead_kind;
    const bool ahead = ahead_kind != 0;
    DOTS_HIP(hipEventRecord(c->ev[0], c->stream));
    if (!ahead && (rc = launch_rhs(c))) return rc;
    DOTS_HIP(hipEventRecord(c->ev[1], c->stream));
    const bool fuse = soc_takes_inverse(c) && ahead_kind != 2;
    if ((rc = cg_solve(c, st, fuse))) return rc;
    DOTS_HIP(hipEventRecord(c->ev[2], c->stream));
    if (ahead_kind != 2 && (rc = launch_soc_projection(c, 1, fuse))) return rc;
    DOTS_HIP(hipEventRecord(c->ev[3], c->stream));
    if ((rc = launch_q_lambda_mult(c, c->step_skip_zmid ? 2 : 1))) return rc;
    c->carried.stepped(c->step_skip_zmid);
    DOTS_HIP(hipEventRecord(c->ev[4], c->stream));
    DOTS_HIP(hipEventSynchronize(c->ev[4]));
    float t;
    DOTS_HIP(hipEventElapsedTime(&t, c->ev[0], c->ev[1])); st->ms_rhs += t;
    DOTS_HIP(hipEventElapsedTime(&t, c->ev[1], c->ev[2])); st->ms_laplacian += t;
    DOTS_HIP(hipEventElapsedTime(&t, c->ev[2], c->ev[3])); st->ms_soc += t;
    DOTS_HIP(hipEventElapsedTime(&t, c->ev[3], c->ev[4])); st->ms_q_lambda_multiplier += t;
    DOTS_HIP(hipEventElapsedTime(&t, c->ev[0], c->ev[4])); st->ms_total += t;
    st->alm_iterations += 1;
    return 0;
}

// A slot of the timing ring is taken before the phases are enqueued: if enqueueing fails midway the slot is given back, so that a
// later dots_step_times never waits on events that were not recorded (and does not hide the original error behind its own).
static int run_iteration(Ctx *c, dots_step_stats *st) {
    hipEvent_t *tv = st ? nullptr : time_slot(c, 0);
    const int rc = run_iteration_body(c, st, tv);
    if (rc && tv) c->t_count -= 1;
    return rc;
}

static void mg_release(Ctx *c) {
    c->mg_pool.release();
    c->mg = MgDev{};
    c->mg_path = 0;      // no cycle of this (or no) hierarchy yet
}

}  // namespace dots

using namespace dots;

extern "C" {

int dots_abi_version(void) { return DOTS_ABI_VERSION; }
const char *dots_last_error(void) { return g_last_error.c_str(); }

int dots_create(const dots_problem_desc *desc, dots_ctx **out) {
    if (!desc || !out) { set_error("null argument"); return DOTS_ERR_ARGUMENT; }
    *out = nullptr;
    if (desc->abi_version != DOTS_ABI_VERSION) { set_error("ABI version mismatch"); return DOTS_ERR_ARGUMENT; }
    if (desc->n_time < 1 || desc->n_vertices < 3 || desc->n_triangles < 1 || desc->n_corners != 3 * desc->n_triangles) {
        set_error("bad problem sizes");
        return DOTS_ERR_ARGUMENT;
    }
    if (!desc->triangles || !desc->hat_grad || !desc->area_tri || !desc->mass_vert || !desc->corner_ptr || !desc->corner_idx ||
        !desc->lap_rowptr || !desc->lap_col || !desc->lap_val || !desc->mu0 || !desc->mu1) {
        set_error("null array in problem description");
        return DOTS_ERR_ARGUMENT;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error("no HIP device"); return DOTS_ERR_NO_DEVICE; }
    if (desc->device < 0 || desc->device >= ndev) { set_error("device ordinal out of range"); return DOTS_ERR_ARGUMENT; }
    DOTS_HIP(hipSetDevice(desc->device));
    std::unique_ptr<dots_ctx> c(new dots_ctx(desc->device));      // (deleted on every failing exit)
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, desc->device) != hipSuccess) c->n_cu = 0;      // (unknown: deep_launch_wins never)
    // measurement switches: every value is validated -- a typo must not silently select the default
    {
        bool ok = true;
        ok &= env_int("DOTS_KKT_TWO", 0, 1, &c->kkt_two);
        ok &= env_int("DOTS_ZMID_DEFER", 0, 1, &c->zmid_defer);    // 0: read-back iterations store z_mid as before
        ok &= env_int("DOTS_LAZY_DIV", 0, 1, &c->lazy_div);        // 0: a penalty update divides the dual arrays at once
        ok &= env_int("DOTS_RHS_DEEP", 0, 1, &c->rhs_deep);        // 0: the right-hand side and inverse transform as they were, 1: their deep forms wherever the kernels exist (default: deep_launch_wins)
        ok &= env_int("DOTS_FRONT_VEC2", 0, 1, &c->sched.vec2);      // 0: one mode per lane in the sweeps everywhere
        ok &= env_int("DOTS_FRONT_ROWS", 0, 2, &c->front_rows);      // 0: the fold kernels everywhere, 1: row kernels where the rules say (default), 2: wherever they fit
        ok &= env_int("DOTS_FRONT_LEAFINV", 0, 2, &c->front_leafinv);
        ok &= env_int("DOTS_FRONT_TUNE", 0, 2, &c->front_tune);
        ok &= env_int("DOTS_FRONT_NR", 2, 8, &c->front_nr_max);      // right-hand sides per launch of a batched solve (2, 4 or 8; A/B measurements)
        if (c->front_nr_max != 2 && c->front_nr_max != 4 && c->front_nr_max != 8) { set_error("DOTS_FRONT_NR must be 2, 4 or 8"); ok = false; }
        ok &= env_int("DOTS_MAIL_TEST_DROP", 0, 1 << 20, &c->mail_test_drop);
        ok &= env_int("DOTS_READOUT_PINNED", 0, 1 << 20, &c->readout_pinned);      // n > 0: dots_readout copies through two pinned slots of n KB (A/B measurements)
        int spins = -1;
        ok &= env_int("DOTS_MAIL_SPINS", 0, 2000000000, &spins);
        if (spins >= 0) c->mail_spins = spins;
        if (!ok) return DOTS_ERR_ARGUMENT;
    }
    DOTS_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (auto &ev : c->ev) (void)hipEventCreate(&ev);
    int rc = build(c.get(), desc);
    if (rc) return rc;
    preload_alm_kernels();
    preload_kkt_kernels();
    preload_transform_kernels();
    preload_readout_kernels();
    preload_restart_kernels();
    preload_barycenter_kernels();
    preload_tangent_kernels();
    preload_geometry_kernels();
    *out = c.release();
    return 0;
}

int dots_destroy(dots_ctx *c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    delete c;      // (~Ctx lists what goes)
    return 0;
}

int dots_set_params(dots_ctx *c, const dots_params *p) {
    // the penalty update the library anticipated (penalty_decision_ahead): only r moves, to the anticipated value
    const bool anticipated = c && p && c->carried.rhs_ahead == 4 && p->r == c->ahead_r && p->scale_z == c->prm.scale_z && p->const_d == c->prm.const_d &&
                             p->eps == c->prm.eps && p->boundary_scale == c->prm.boundary_scale && p->congestion == c->prm.congestion && p->tau == c->prm.tau;
    int rc = admit(c, E_SET_PARAMS);
    if (rc) return rc;
    if (!p || !(p->r > 0) || !(p->scale_z > 0) || !(p->cg_tol > 0) || p->eps < 0 || !(p->boundary_scale > 0)) { set_error("bad parameters"); return DOTS_ERR_ARGUMENT; }
    c->prm = *p;
    if (anticipated && c->carried.pending_div == c->ahead_dv) {
        c->carried.rhs_ahead = 2;
        c->carried.ahead_div = c->ahead_dv;
        c->penalty_ahead_confirmed += 1;
    }
    return 0;
}

int dots_penalty_ahead(dots_ctx *c, const dots_penalty_policy *policy) {
    int rc = admit(c, E_PENALTY_AHEAD);
    if (rc) return rc;
    if (c->batched) { set_error("penalty_ahead: the context is stepped in a batch (dots_step_many)"); return DOTS_ERR_STATE; }
    if (!policy || policy->n_steps < 0 || policy->n_steps > 16 || !(policy->tol > 0) || !(policy->r_lower > 0) || !(policy->r_upper >= policy->r_lower)) {
        set_error("penalty_ahead: bad policy");
        return DOTS_ERR_ARGUMENT;
    }
    c->penalty_policy = *policy;
    c->carried.penalty_armed = 1;
    return 0;
}
int dots_get_params(dots_ctx *c, dots_params *p) {
    if (!c || !p) { set_error("null argument"); return DOTS_ERR_ARGUMENT; }
    *p = c->prm;
    return 0;
}
int dots_sync(dots_ctx *c) {
    int rc = admit(c, E_SYNC);
    if (rc) return rc;
    DOTS_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int64_t dots_array_count(dots_ctx *c, int id) {
    if (!c || id < 0 || id >= DOTS_N_ARRAYS) return -1;
    return array_count_host(c->d, id);
}
int64_t dots_device_bytes(dots_ctx *c) { return c ? c->pool.bytes() : -1; }

int dots_upload(dots_ctx *c, int id, const double *host, int64_t count) {
    int rc = admit(c, E_UPLOAD);
    if (rc) return rc;
    // a time slab that has a next slab may bring phi at that slab's first node along, as one more row: it becomes phi_hi, which only
    // this rank's inverse transform writes otherwise (step 0 of DOTS_STEP_PALM and the KKT kernels read it before the first solve)
    const bool with_hi = id == DOTS_PHI && host && c->d.slab && c->d.phi_hi && c->d.nl > 0 && c->d.t0 + c->d.nl <= c->d.T &&
                         count == array_count_host(c->d, id) + c->d.V && count <= c->stage_count;
    if (id < 0 || id >= DOTS_N_ARRAYS || !host || (count != array_count_host(c->d, id) && !with_hi)) { set_error("upload: bad array id or element count"); return DOTS_ERR_ARGUMENT; }
    if ((rc = need_zmid(c, E_UPLOAD, id != DOTS_Z_MID))) return rc;
    DOTS_HIP(hipMemcpyAsync(c->stage, host, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_to_device_layout(c, id, c->arr(id), c->stage))) return rc;
    if (with_hi) {
        hipLaunchKernelGGL(k_slab_phi_hi, dim3((c->d.V + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, c->d, c->stage + (int64_t)c->d.nl * c->d.V, c->d.phi_hi);
        DOTS_HIP(hipGetLastError());
    }
    DOTS_HIP(hipStreamSynchronize(c->stream));
    if (id == DOTS_Z_MID) c->carried.zmid = ZMID_STORED;      // (the upload is what z_mid's storage now holds)
    state_changed(c->carried);
    return 0;
}
int dots_download(dots_ctx *c, int id, double *host, int64_t count) {
    int rc = admit(c, E_DOWNLOAD);
    if (rc) return rc;
    if (id < 0 || id >= DOTS_N_ARRAYS || !host || count != array_count_host(c->d, id)) { set_error("download: bad array id or element count"); return DOTS_ERR_ARGUMENT; }
    if ((rc = need_zmid(c, E_DOWNLOAD, id == DOTS_Z_MID))) return rc;
    if ((rc = launch_from_device_layout(c, id, c->arr(id), c->stage))) return rc;
    DOTS_HIP(hipMemcpyAsync(host, c->stage, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    DOTS_HIP(hipStreamSynchronize(c->stream));
    c->d2h_bytes += (int64_t)sizeof(double) * count;
    return 0;
}

int64_t dots_slab_elems(dots_ctx *c, int which) {
    if (!c || c->shard_stride == 0) return -1;
    const int64_t nnode = (int64_t)c->d.V << c->d.tp_shift;
    switch (which) {
        case DOTS_SLAB_VERTEX_HALO: return c->d.V;
        case DOTS_SLAB_B_CHUNK: return nnode;
        case DOTS_SLAB_X_CHUNK: return nnode + c->d.V;
        case DOTS_SLAB_TRIANGLE_HALO: return (int64_t)3 * c->d.F;
        default: return -1;
    }
}

int dots_slab_set_buffers(dots_ctx *c, const dots_slab_buffers *b) {
    int rc = admit(c, E_SLAB_SET_BUFFERS);
    if (rc) return rc;
    if (c->shard_stride == 0) { set_error("slab_set_buffers: context is not a time slab"); return DOTS_ERR_STATE; }
    if (!b || !b->send_x || !b->send_nsq || !b->recv_x || !b->recv_nsq || !b->b_send || !b->b_recv || !b->x_send || !b->x_recv ||
        !b->send_mu || !b->send_b || !b->recv_mu || !b->recv_b) {
        set_error("slab_set_buffers: null buffer");
        return DOTS_ERR_ARGUMENT;
    }
    DOTS_HIP(hipStreamSynchronize(c->stream));
    c->slab = *b;
    Dev &d = c->d;
    const int rank = c->shard_begin / c->shard_stride;
    d.cg_b = b->b_send;                         // the right-hand side of this slab is written where the all-gather reads it
    d.X_lo = b->recv_x;
    d.nsq_hi = b->recv_nsq;
    d.mu_lo = b->recv_mu;
    d.B_hi = b->recv_b;
    // the previous slab appended its last interval's cone multipliers to its chunk of the SOLUTION all-gather (they are needed by
    // steps 2+3, after it: the right-hand-side all-gather can then start before the projection has run)
    d.lamc_lo = (rank > 0 && d.nl > 0) ? b->x_recv + (int64_t)(rank - 1) * c->slab_x_chunk + ((int64_t)d.V << d.tp_shift) : b->recv_x;
    c->pcg.cg_x = b->x_send;                    // the solver's view: the mode-space solution is written where the second all-gather reads it
    // the PCG's warm start (its own previous solution) and the buffers' padding start from zero
    DOTS_HIP(hipMemsetAsync(b->x_send, 0, sizeof(double) * (size_t)c->slab_x_chunk, c->stream));
    DOTS_HIP(hipMemsetAsync(b->b_send, 0, sizeof(double) * (size_t)c->slab_b_chunk, c->stream));
    DOTS_HIP(hipStreamSynchronize(c->stream));
    c->slab_stage = 0;
    return 0;
}

int dots_slab_stage(dots_ctx *c, int stage, dots_step_stats *stats) {
    int rc = admit(c, E_SLAB_STAGE);
    if (rc) return rc;
    if (c->shard_stride == 0) { set_error("slab_stage: context is not a time slab"); return DOTS_ERR_STATE; }
    if (!c->slab.b_send) { set_error("slab_stage: no exchange buffers (dots_slab_set_buffers)"); return DOTS_ERR_STATE; }
    if (stage < 0 || stage > 6) { set_error("slab_stage: unknown stage"); return DOTS_ERR_ARGUMENT; }
    // order: 0, 1, 2, 3 -- or with stage 1 in two halves: 0, 6, 5, 2, 3 (slab_stage = the next stage expected; 5: the projection is due)
    const bool in_order = stage == 4 || stage == c->slab_stage || (stage == 6 && c->slab_stage == 1);
    if (!in_order) { set_error("slab_stage: stages must be called in the order 0, 1, 2, 3 (or 0, 6, 5, 2, 3)"); return DOTS_ERR_STATE; }
    if (stage == 4 && c->slab_stage != 0) { set_error("slab_stage: the KKT halos are packed between iterations"); return DOTS_ERR_STATE; }
    if (!stats) {
        hipEvent_t *tv = stage != 4 ? time_slot(c, 1 + stage) : nullptr;
        rc = tv ? (int)hipEventRecord(tv[0], c->stream) : 0;
        if (!rc) rc = slab_stage(c, stage);
        if (!rc && tv && hipEventRecord(tv[1], c->stream) != hipSuccess) rc = DOTS_ERR_HIP;
        if (rc) {      // (the slot goes back to the ring: see run_iteration)
            if (tv) c->t_count -= 1;
            if (rc > 0) { set_error("slab_stage: hipEventRecord failed"); rc = DOTS_ERR_HIP; }
            return rc;
        }
    } else {
        DOTS_HIP(hipEventRecord(c->ev[0], c->stream));
        if ((rc = slab_stage(c, stage))) return rc;
        DOTS_HIP(hipEventRecord(c->ev[1], c->stream));
        DOTS_HIP(hipEventSynchronize(c->ev[1]));
        float t;
        DOTS_HIP(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
        memset(stats, 0, sizeof *stats);
        book_stage(*stats, stage, t);
        if (stage == 2) stats->cg_iterations = stats->cg_last_iterations = c->last_cg_iters;
    }
    if (stage <= 3) c->slab_stage = (stage + 1) & 3;
    else if (stage == 6) c->slab_stage = 5;
    else if (stage == 5) c->slab_stage = 2;
    return 0;
}

int dots_stream_wait(dots_ctx *c, void *other_stream, int ctx_waits) {
    int rc = admit(c, E_STREAM_WAIT);
    if (rc) return rc;
    hipStream_t other = (hipStream_t)other_stream;       // nullptr = the legacy default stream
    if (ctx_waits) {
        DOTS_HIP(hipEventRecord(c->ev[10], other));
        DOTS_HIP(hipStreamWaitEvent(c->stream, c->ev[10], 0));
    } else {
        DOTS_HIP(hipEventRecord(c->ev[11], c->stream));
        DOTS_HIP(hipStreamWaitEvent(other, c->ev[11], 0));
    }
    return 0;
}

int dots_step(dots_ctx *c, int n_iters, dots_step_stats *stats) {
    int rc = admit(c, E_STEP);
    if (rc) return rc;
    c->batched = 0;
    if (n_iters < 0) { set_error("n_iters < 0"); return DOTS_ERR_ARGUMENT; }
    if (c->shard_stride != 0) { set_error("dots_step on a time slab: use dots_slab_stage"); return DOTS_ERR_STATE; }
    if ((rc = modal_needs_factor(c, "dots_step"))) return rc;
    dots_step_stats local;
    memset(&local, 0, sizeof local);
    for (int i = 0; i < n_iters; ++i)
        if ((rc = run_iteration(c, stats ? &local : nullptr))) return rc;
    if (stats) *stats = local;
    return 0;
}

int dots_step_flags(dots_ctx *c, uint32_t flags) {
    int rc = admit(c, E_STEP_FLAGS);
    if (rc) return rc;
    if (flags & ~(uint32_t)(DOTS_STEP_SKIP_Z_MID | DOTS_STEP_PALM | DOTS_STEP_RHS_AHEAD | DOTS_STEP_TIMED | DOTS_STEP_CARRY | DOTS_STEP_KKT_SUMS)) { set_error("step_flags: unknown flag"); return DOTS_ERR_ARGUMENT; }
    if ((flags & DOTS_STEP_RHS_AHEAD) && (flags & DOTS_STEP_PALM)) { set_error("step_flags: DOTS_STEP_RHS_AHEAD cannot be combined with DOTS_STEP_PALM (its step 0 changes what the right-hand side reads)"); return DOTS_ERR_ARGUMENT; }
    c->carried.rhs_ahead_armed = ((flags & DOTS_STEP_RHS_AHEAD) && rhs_writes_modes(c)) ? 1 : 0;      // (a hint: ignored without the direct solver / on a time slab)
    if ((flags & DOTS_STEP_SKIP_Z_MID) && (flags & DOTS_STEP_PALM)) { set_error("step_flags: DOTS_STEP_PALM reads z_mid, it cannot be combined with DOTS_STEP_SKIP_Z_MID"); return DOTS_ERR_ARGUMENT; }
    c->step_skip_zmid = (flags & DOTS_STEP_SKIP_Z_MID) ? 1 : 0;
    c->step_palm = (flags & DOTS_STEP_PALM) ? 1 : 0;
    c->step_timed = (flags & DOTS_STEP_TIMED) ? 1 : 0;
    c->step_carry = ((flags & DOTS_STEP_CARRY) && !(flags & DOTS_STEP_PALM)) ? 1 : 0;      // (a hint, like DOTS_STEP_RHS_AHEAD)
    c->step_kkt = ((flags & DOTS_STEP_KKT_SUMS) && !(flags & DOTS_STEP_SKIP_Z_MID)) ? 1 : 0;  // (a hint as well)
    return 0;
}

int dots_step_times(dots_ctx *c, dots_step_stats *out, int capacity, int wait, int *n_out) {
    int rc = admit(c, E_STEP_TIMES);
    if (rc) return rc;
    if (!out || !n_out || capacity < 0) { set_error("step_times: bad argument"); return DOTS_ERR_ARGUMENT; }
    int n = 0;
    while (n < capacity && c->t_count > 0) {
        hipEvent_t *tv = c->tev[c->t_head];
        const int kind = c->tkind[c->t_head];
        const bool whole = kind == 0 || kind == TKIND_FUSED;
        hipEvent_t last = tv[whole ? 5 : 1];
        if (wait) DOTS_HIP(hipEventSynchronize(last));
        else {
            const hipError_t q = hipEventQuery(last);
            if (q == hipErrorNotReady) break;
            DOTS_HIP(q);
        }
        dots_step_stats &st = out[n];
        memset(&st, 0, sizeof st);
        float t;
        if (whole) {
            // Every phase is bracketed by two events, and an event costs stream time itself: the gap between the two events
            // recorded back to back behind the last kernel (4, 5) is that cost, measured in this very iteration; it is taken off
            // every phase so that the sampled times estimate what the UNTIMED iterations of the kind take.
            float gap, p[4];
            DOTS_HIP(hipEventElapsedTime(&gap, tv[4], tv[5]));
            for (int i = 0; i < 4; ++i) {
                DOTS_HIP(hipEventElapsedTime(&p[i], tv[i], tv[i + 1]));
                p[i] = p[i] > gap ? p[i] - gap : 0.0f;
            }
            if (kind == TKIND_FUSED) {      // one launch for the right-hand side and the projection: half each, as a slab's stage 1
                st.ms_rhs = st.ms_soc = 0.5 * p[0];
            } else {
                st.ms_rhs = p[0];
                st.ms_soc = p[2];
            }
            st.ms_laplacian = p[1];
            st.ms_q_lambda_multiplier = p[3];
            st.ms_total = (double)p[0] + p[1] + (kind == TKIND_FUSED ? 0.0 : (double)p[2]) + p[3];
            st.alm_iterations = 1;
        } else {
            const int stage = kind - 1;
            DOTS_HIP(hipEventElapsedTime(&t, tv[0], tv[1]));
            book_stage(st, stage, t);
        }
        c->t_head = (c->t_head + 1) % Ctx::TIME_SLOTS;
        c->t_count -= 1;
        ++n;
    }
    *n_out = n;
    return 0;
}

int dots_run_phase(dots_ctx *c, int phase, dots_step_stats *stats) {
    int rc = admit(c, E_RUN_PHASE);
    if (rc) return rc;
    if (c->shard_stride != 0) { set_error("run_phase works on whole arrays: not available on a time slab"); return DOTS_ERR_STATE; }
    dots_step_stats local;
    memset(&local, 0, sizeof local);
    if ((rc = need_zmid(c, E_RUN_PHASE, phase == DOTS_PHASE_Q_LAMBDA))) return rc;
    switch (phase) {
        case DOTS_PHASE_LAPLACIAN:
            if ((rc = modal_needs_factor(c, "run_phase(LAPLACIAN)"))) return rc;
            if ((rc = launch_rhs(c))) return rc;
            if ((rc = cg_solve(c, &local))) return rc;
            break;
        case DOTS_PHASE_SOC_PROJECTION: rc = launch_soc_projection(c); c->carried.zmid = ZMID_STORED; break;
        case DOTS_PHASE_Q_LAMBDA_MULT: rc = launch_q_lambda_mult(c); break;
        case DOTS_PHASE_Q_LAMBDA: rc = launch_q_lambda_only(c); break;
        default: set_error("unknown phase"); return DOTS_ERR_ARGUMENT;
    }
    if (rc) return rc;
    DOTS_HIP(hipStreamSynchronize(c->stream));
    if (stats) *stats = local;
    return 0;
}

// What the three KKT entry points share behind admit: the mask check, the refusal of an unspecified z_mid, on a time slab the refusal
// of stale halos (dots_kkt: of the slab itself), and z_mid rebuilt where the stand-alone kernels read it.  An empty mask passes.
static int kkt_prelude(Ctx *c, Entry e, uint32_t mask, const double *out) {
    const char *who = ADMISSION[e].name;
    if (!out || (mask >> DOTS_N_KKT)) { set_error(std::string(who) + ": bad mask or null output"); return DOTS_ERR_ARGUMENT; }
    if (!mask) return 0;
    const bool prim_z = mask & (1u << DOTS_KKT_PRIM_Z);
    int rc;
    if (prim_z && (rc = refuse_unspecified_zmid(c->carried, e))) return rc;
    if (c->shard_stride != 0 && e == E_KKT) { set_error("kkt on a time slab: use dots_kkt_sums / dots_kkt_combine around the caller's all-reduce"); return DOTS_ERR_STATE; }
    if (c->shard_stride != 0 && !c->carried.kkt_halo_fresh && (mask & ((1u << DOTS_KKT_DUAL_ALPHA) | (1u << DOTS_KKT_COMP_RHO_FQ) | (1u << DOTS_KKT_COMP_M_RHO_B)))) {
        set_error(std::string(who) + ": the KKT halos are stale (dots_slab_stage 4 + exchange first)");
        return DOTS_ERR_STATE;
    }
    return need_zmid(c, e, prim_z && !kkt_takes_fused(c, mask));
}

int dots_kkt(dots_ctx *c, uint32_t mask, double *out) {
    int rc = admit(c, E_KKT);
    if (rc || (rc = kkt_prelude(c, E_KKT, mask, out)) || !mask) return rc;
    return kkt_evaluate(c, mask, out);
}
int dots_kkt_sums(dots_ctx *c, uint32_t mask, double *sums) {
    int rc = admit(c, E_KKT_SUMS);
    if (rc) return rc;
    static_assert(DOTS_KKT_N_SUMS == MAX_SUMS, "header and kernels disagree on the number of KKT sums");
    for (int i = 0; sums && !(mask >> DOTS_N_KKT) && i < DOTS_KKT_N_SUMS; ++i) sums[i] = 0.0;      // (also when the call is then refused)
    if ((rc = kkt_prelude(c, E_KKT_SUMS, mask, sums)) || !mask) return rc;
    return kkt_sums(c, mask, sums);
}
int dots_kkt_sums_device(dots_ctx *c, uint32_t mask, double *device_sums) {
    int rc = admit(c, E_KKT_SUMS_DEVICE);
    if (rc || (rc = kkt_prelude(c, E_KKT_SUMS_DEVICE, mask, device_sums))) return rc;
    return kkt_sums_device(c, mask, device_sums);
}
int dots_kkt_combine(dots_ctx *c, uint32_t mask, const double *sums, double *out) {
    int rc = admit(c, E_KKT_COMBINE);
    if (rc) return rc;
    if (!sums || !out || (mask >> DOTS_N_KKT)) { set_error("kkt_combine: bad argument"); return DOTS_ERR_ARGUMENT; }
    return kkt_combine(c, mask, sums, out);
}
int dots_objective_sums(dots_ctx *c, double *sums) {
    int rc = admit(c, E_OBJECTIVE_SUMS);
    if (rc) return rc;
    if (!sums) { set_error("null output"); return DOTS_ERR_ARGUMENT; }
    return objective_sums(c, sums);
}
int dots_objective_combine(dots_ctx *c, const double *sums, double *out) {
    int rc = admit(c, E_OBJECTIVE_COMBINE);
    if (rc) return rc;
    if (!sums || !out) { set_error("null argument"); return DOTS_ERR_ARGUMENT; }
    return objective_combine(c, sums, out);
}

int dots_objective(dots_ctx *c, double *out) {
    int rc = admit(c, E_OBJECTIVE);
    if (rc) return rc;
    if (!out) { set_error("null output"); return DOTS_ERR_ARGUMENT; }
    if (c->shard_stride != 0) { set_error("objective on a time slab: use dots_objective_sums / dots_objective_combine"); return DOTS_ERR_STATE; }
    return objective_evaluate(c, out);
}

int dots_adjust_penalty(dots_ctx *c, double factor) {
    const bool anticipated = c && c->carried.rhs_ahead == 3 && factor == c->ahead_dv;      // (penalty_decision_ahead; admission drops the launch ahead)
    int rc = admit(c, E_ADJUST_PENALTY);      // (carries out a division that is still pending)
    if (rc) return rc;
    if (!(factor > 0)) { set_error("factor must be positive"); return DOTS_ERR_ARGUMENT; }
    state_changed(c->carried);
    // one GPU, direct solver: the next iteration's kernels apply the division as they read (run_iteration); any other access to
    // the arrays carries it out first (admission.h: DUALS)
    if (c->lazy_div && c->shard_stride == 0 && carry_possible(c)) {
        c->carried.pending_div = factor;
        if (anticipated) c->carried.rhs_ahead = 4;      // ... kept if dots_set_params now brings the anticipated penalty
        return 0;
    }
    return launch_adjust_penalty(c, factor);
}
int dots_scale_z(dots_ctx *c, double z_mul, double beta_mul, double sz_new) {
    int rc = admit(c, E_SCALE_Z);
    if (rc) return rc;
    state_changed(c->carried);
    if ((rc = need_zmid(c, E_SCALE_Z))) return rc;
    return launch_scale_z(c, z_mul, beta_mul, sz_new);
}
int dots_scale_arrays(dots_ctx *c, uint32_t mask, double factor) {
    int rc = admit(c, E_SCALE_ARRAYS);
    if (rc) return rc;
    if (mask >> DOTS_N_ARRAYS) { set_error("bad array mask"); return DOTS_ERR_ARGUMENT; }
    state_changed(c->carried);
    if ((rc = need_zmid(c, E_SCALE_ARRAYS))) return rc;
    for (int id = 0; id < DOTS_N_ARRAYS; ++id)
        if ((mask >> id) & 1u)
            if ((rc = launch_scale_array(c, id, factor))) return rc;
    return 0;
}
int dots_norm_square(dots_ctx *c, int id, int part, double *out) {
    int rc = admit(c, E_NORM_SQUARE);
    if (rc) return rc;
    if (id < 0 || id >= DOTS_N_ARRAYS || !out || part < 0 || part > 2) { set_error("norm_square: bad argument"); return DOTS_ERR_ARGUMENT; }
    if ((rc = need_zmid(c, E_NORM_SQUARE, id == DOTS_Z_MID))) return rc;
    return norm_square(c, id, part, out);
}

int dots_apply_operator(dots_ctx *c, int op, double scale, const double *in, int64_t n_in, double *out, int64_t n_out) {
    int rc = admit(c, E_APPLY_OPERATOR);
    if (rc) return rc;
    // (input array class, output array class) per operator, expressed through state arrays of the same shape
    int in_id, out_id;
    switch (op) {
        case DOTS_OP_GRAD_TIME: in_id = DOTS_PHI; out_id = DOTS_A; break;
        case DOTS_OP_DIV_TIME: case DOTS_OP_TIME_AVG_ADJOINT: in_id = DOTS_A; out_id = DOTS_PHI; break;
        case DOTS_OP_GRAD_SPACE: in_id = DOTS_PHI; out_id = DOTS_B; break;
        case DOTS_OP_DIV_SPACE: in_id = DOTS_B; out_id = DOTS_PHI; break;
        case DOTS_OP_DECOUPLE: in_id = DOTS_B; out_id = DOTS_Z_MID; break;
        case DOTS_OP_DECOUPLE_ADJOINT: in_id = DOTS_Z_MID; out_id = DOTS_B; break;
        case DOTS_OP_LAPLACIAN_APPLY: in_id = DOTS_PHI; out_id = DOTS_PHI; break;
        default: set_error("unknown operator"); return DOTS_ERR_ARGUMENT;
    }
    if (!in || !out || n_in != array_count_host(c->d, in_id) || n_out != array_count_host(c->d, out_id)) {
        set_error("apply_operator: bad element counts");
        return DOTS_ERR_ARGUMENT;
    }
    // scratch: device-layout input and output live in two temporary buffers
    DevicePool tmp(c->device);
    double *din = nullptr, *dout = nullptr;
    auto enqueue = [&]() -> int {
        int r;
        if ((r = tmp.alloc(&din, array_count_device(c->d, in_id), c->stream, false))) return r;
        if ((r = tmp.alloc(&dout, array_count_device(c->d, out_id), c->stream))) return r;
        DOTS_HIP(hipMemcpyAsync(c->stage, in, sizeof(double) * (size_t)n_in, hipMemcpyHostToDevice, c->stream));
        if ((r = launch_to_device_layout(c, in_id, din, c->stage))) return r;
        if ((r = op == DOTS_OP_LAPLACIAN_APPLY ? cg_apply_operator(c, din, dout) : launch_operator(c, op, scale, din, dout))) return r;
        if ((r = launch_from_device_layout(c, out_id, dout, c->stage))) return r;
        DOTS_HIP(hipMemcpyAsync(out, c->stage, sizeof(double) * (size_t)n_out, hipMemcpyDeviceToHost, c->stream));
        return 0;
    };
    rc = enqueue();      // (every path out of the call waits for the stream before the buffers go)
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (rc) return rc;
    DOTS_HIP(es);
    return 0;
}

int dots_mg_setup(dots_ctx *c, const dots_mg_desc *m) {
    int rc = admit(c, E_MG_SETUP);
    if (rc) return rc;
    if (!m || m->n_levels < 2 || m->n_levels > 10 || !m->levels || !m->coarse_inverse) { set_error("mg_setup: bad description"); return DOTS_ERR_ARGUMENT; }
    if (c->lap_solver != DOTS_LAP_MODAL_PCG) { set_error("multigrid needs the modal solver"); return DOTS_ERR_ARGUMENT; }
    const bool windowed = c->pcg_windows && c->shard_stride == 0 && pcg_ncol(c) > CgScalOffsets::NCMAX;      // one coarse inverse per window of 256 modes
    if (pcg_ncol(c) > CgScalOffsets::NCMAX && !windowed) { set_error("mg_setup: the modal PCG takes T + 1 <= 256; above, use the direct solver (dots_front_setup)"); return DOTS_ERR_STATE; }
    if (m->levels[0].n != c->d.V || m->n_cols != pcg_ncol(c)) { set_error("mg_setup: level 0 / mode count mismatch"); return DOTS_ERR_ARGUMENT; }
    DOTS_HIP(hipStreamSynchronize(c->stream));
    c->cg_graphs_release();
    mg_release(c);
    // level vectors and the coarse inverse use the PCG view's pitch; windowed: a window's (256 columns), the vectors reused by every window
    const Dev pv = pcg_view(c), d = windowed ? pcg_window_view(pv, 0) : pv;
    MgDev g{};
    g.nlev = m->n_levels;
    g.omega = m->omega;
    for (int l = 0; l < m->n_levels; ++l) {
        const dots_mg_level &h = m->levels[l];
        MgLevelDev &L = g.lv[l];
        L.n = h.n;
        L.nc = h.n_coarse;
        if (l + 1 < m->n_levels && (h.n_coarse != m->levels[l + 1].n || !h.p_rowptr || !h.r_rowptr)) { set_error("mg_setup: inconsistent level sizes"); mg_release(c); return DOTS_ERR_ARGUMENT; }
        // index sanity (a wrong index would fault on the device)
        if (l > 0) {
            if (!h.rowptr || !h.col || !h.val_k || !h.val_m || !h.diag_k || !h.diag_m) { set_error("mg_setup: null level array"); mg_release(c); return DOTS_ERR_ARGUMENT; }
            for (int j = 0; j < h.nnz; ++j) if (h.col[j] < 0 || h.col[j] >= h.n) { set_error("mg_setup: column index out of range"); mg_release(c); return DOTS_ERR_ARGUMENT; }
            if (h.rowptr[h.n] != h.nnz) { set_error("mg_setup: rowptr/nnz mismatch"); mg_release(c); return DOTS_ERR_ARGUMENT; }
        }
        if (l + 1 < m->n_levels) {
            if (h.p_rowptr[h.n] != h.p_nnz || h.r_rowptr[h.n_coarse] != h.p_nnz) { set_error("mg_setup: P/R size mismatch"); mg_release(c); return DOTS_ERR_ARGUMENT; }
            for (int j = 0; j < h.p_nnz; ++j)
                if (h.p_col[j] < 0 || h.p_col[j] >= h.n_coarse || h.r_col[j] < 0 || h.r_col[j] >= h.n) { set_error("mg_setup: P/R index out of range"); mg_release(c); return DOTS_ERR_ARGUMENT; }
        }
#define MUP(field, src, n) if ((rc = c->mg_pool.upload(&L.field, src, (int64_t)(n), c->stream))) { mg_release(c); return rc; }
        if (l == 0) {
            L.rp = d.rowptr; L.col = d.col; L.vK = d.val; L.vM = nullptr; L.dK = d.kdiag; L.dM = d.mass_v;
        } else {
            MUP(rp, h.rowptr, h.n + 1); MUP(col, h.col, h.nnz); MUP(vK, h.val_k, h.nnz); MUP(vM, h.val_m, h.nnz);
            MUP(dK, h.diag_k, h.n); MUP(dM, h.diag_m, h.n);
        }
        if (l + 1 < m->n_levels) {
            MUP(p_rp, h.p_rowptr, h.n + 1); MUP(p_col, h.p_col, h.p_nnz); MUP(p_val, h.p_val, h.p_nnz);
            MUP(r_rp, h.r_rowptr, h.n_coarse + 1); MUP(r_col, h.r_col, h.p_nnz); MUP(r_val, h.r_val, h.p_nnz);
            if (!h.ap_rowptr || !h.ap_col || !h.ap_val_k || !h.ap_val_m || !h.ap_val_p || h.ap_rowptr[h.n] != h.ap_nnz) { set_error("mg_setup: bad A*P arrays"); mg_release(c); return DOTS_ERR_ARGUMENT; }
            for (int j = 0; j < h.ap_nnz; ++j) if (h.ap_col[j] < 0 || h.ap_col[j] >= h.n_coarse) { set_error("mg_setup: A*P index out of range"); mg_release(c); return DOTS_ERR_ARGUMENT; }
            MUP(ap_rp, h.ap_rowptr, h.n + 1); MUP(ap_col, h.ap_col, h.ap_nnz); MUP(ap_vK, h.ap_val_k, h.ap_nnz); MUP(ap_vM, h.ap_val_m, h.ap_nnz); MUP(ap_vP, h.ap_val_p, h.ap_nnz);
        }
#undef MUP
        // level vectors; level 0 works on the PCG's own r, z and Ap buffers
        if (l > 0) {
            const int64_t nv = (int64_t)h.n << d.tp_shift;
            const double *tmp = nullptr;
            double **vecs[3] = {&L.b, &L.bt, &L.t};
            for (auto v : vecs) {
                if ((rc = c->mg_pool.upload<double>(&tmp, nullptr, nv, c->stream))) { mg_release(c); return rc; }
                *v = const_cast<double *>(tmp);
            }
        }
    }
    // coarse inverse: host [nL][nL][n_cols] -> device [nL][nL][TP]
    // (windowed: block w = the modes [256 w, 256 w + 256), [nL][nL][256] each, one after the other)
    const int nL = m->levels[m->n_levels - 1].n;
    const int n_win = windowed ? pcg_window_count(pv) : 1;
    const size_t block = (size_t)nL * nL * d.TP;
    std::vector<double> inv(block * n_win, 0.0);
    for (int64_t ij = 0; ij < (int64_t)nL * nL; ++ij)
        for (int k = 0; k < m->n_cols; ++k) inv[(size_t)(k / d.TP) * block + (size_t)ij * d.TP + k % d.TP] = m->coarse_inverse[(size_t)ij * m->n_cols + k];
    if ((rc = c->mg_pool.upload(&g.coarse_inv, inv, c->stream))) { mg_release(c); return rc; }
    // mg_release() reset c->mg; the level pointers were written into the local copy
    for (int l = 0; l < g.nlev; ++l) c->mg.lv[l] = g.lv[l];
    c->mg.nlev = g.nlev;
    c->mg.omega = g.omega;
    c->mg.coarse_inv = g.coarse_inv;
    c->mg.coarse_win_stride = windowed ? (int64_t)block : 0;
    return 0;
}

int dots_mg_enable(dots_ctx *c, int on) {
    int rc = admit(c, E_MG_ENABLE);
    if (rc) return rc;
    c->use_mg = on ? 1 : 0;
    if (!c->use_mg) c->mg_path = 0;      // Jacobi from here on: the last cycle's launches are no longer this context's
    return 0;
}

// One V-cycle on a caller's residual (tests and diagnosis; the product path never calls it): the launches are cg_mg_apply's, i.e. mg_vcycle with
// the PCG's own tiling.  The PCG vectors, partial rows and flags it writes are scratch between solves (kernels_cg.hip: cg_mg_apply).
int dots_mg_apply(dots_ctx *c, const double *r, double *z, double *rz, const int32_t *frozen) {
    int rc = admit(c, E_MG_APPLY);
    if (rc) return rc;
    if (c->lap_solver != DOTS_LAP_MODAL_PCG) { set_error("mg_apply: the V-cycle belongs to the modal solver"); return DOTS_ERR_STATE; }
    if (c->shard_stride != 0) { set_error("mg_apply: not on a time slab"); return DOTS_ERR_STATE; }
    if (pcg_ncol(c) > CgScalOffsets::NCMAX) { set_error("mg_apply: one V-cycle on all modes takes T + 1 <= 256 (a windowed context cycles inside its solves only)"); return DOTS_ERR_STATE; }
    if (c->mg.nlev < 2) { set_error("mg_apply: no multigrid hierarchy on this context (dots_mg_setup)"); return DOTS_ERR_STATE; }
    if (!r || !z || !rz) { set_error("mg_apply: null array"); return DOTS_ERR_ARGUMENT; }
    const Dev &g = c->d;      // (not a time slab: the PCG view is d)
    const int64_t nh = array_count_host(c->d, DOTS_PHI);      // [n_modes][V], the layout of phi
    for (int k = 0; k < FLAG_TOTAL; ++k) c->h_flags[k] = (k < g.cg_ncol && frozen && frozen[k]) ? 1 : 0;
    DOTS_HIP(hipMemcpyAsync(g.flags, c->h_flags, sizeof(int) * FLAG_TOTAL, hipMemcpyHostToDevice, c->stream));
    DOTS_HIP(hipMemcpyAsync(c->stage, r, sizeof(double) * (size_t)nh, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_to_device_layout(c, DOTS_PHI, g.cg_r, c->stage))) return rc;
    if ((rc = cg_mg_apply(c, rz))) return rc;
    if ((rc = launch_from_device_layout(c, DOTS_PHI, g.cg_z, c->stage))) return rc;
    DOTS_HIP(hipMemcpyAsync(z, c->stage, sizeof(double) * (size_t)nh, hipMemcpyDeviceToHost, c->stream));
    DOTS_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// DOTS_STEP_CARRY: the per-corner gathers steps 2+3 leave for the next right-hand side / projection (one GPU, pitch <= 128);
// they belong to the direct solver's iteration and are released with the factor (per context: a sharer of a factor has its own)
static int front_carry_alloc(Ctx *c) {
    int rc;
    if (c->d.TP <= 128 && c->d.nl > 0) {      // (one GPU or a time slab with nodes)
        const int64_t rows = (int64_t)3 * c->d.F;
        const double *sq = nullptr, *g = nullptr, *lo = nullptr, *e = nullptr;
        DevicePool &own = c->front_own;
        if ((rc = own.upload<double>(&sq, nullptr, (2 * rows) << c->d.tp_shift, c->stream)) || (rc = own.upload<double>(&g, nullptr, rows << c->d.tp_shift, c->stream)) ||
            (rc = own.upload<double>(&lo, nullptr, rows, c->stream)) || (c->shard_stride == 0 && (rc = own.upload<double>(&e, nullptr, rows << c->d.tp_shift, c->stream)))) {
            front_release(c);
            return rc;
        }
        c->d.cn_sq = const_cast<double *>(sq);
        c->d.cn_g = const_cast<double *>(g);
        c->d.cn_lo = const_cast<double *>(lo);
        c->d.cn_e = const_cast<double *>(e);
    }
    return 0;
}

// a context with its own direct solver on one GPU: what the batched calls take
static bool front_batchable(const Ctx *c) {
    return c->use_front && c->front.n_nodes > 0 && c->shard_stride == 0 && c->lap_solver == DOTS_LAP_MODAL_PCG;
}

// c's stream waits for what is enqueued on `other`'s stream so far
static int batch_wait(Ctx *c, Ctx *other) {
    if (c == other) return 0;
    if (!other->ev_batch) DOTS_HIP(hipEventCreateWithFlags(&other->ev_batch, hipEventDisableTiming));
    DOTS_HIP(hipEventRecord(other->ev_batch, other->stream));
    DOTS_HIP(hipStreamWaitEvent(c->stream, other->ev_batch, 0));
    return 0;
}

// The members of a batched call and what front_solve_many reads and writes per member: right-hand side, intermediate, solution (modes)
struct BatchMembers {
    std::vector<Ctx *> cv;
    std::vector<const double *> bh;
    std::vector<double *> ys, xs;
};

// cs[0 .. n) as the members of the batched call `e`: each is admitted as its row says, holds a direct solver on one GPU and the factor
// of cs[0], and is listed once.
// `one_message` (dots_bench_many): the two factor checks under one text and status, no search for a context listed twice.
static int batch_members(Entry e, dots_ctx *const *cs, int n, BatchMembers &out, bool one_message = false) {
    const std::string w(ADMISSION[e].name);
    int rc;
    for (int k = 0; k < n; ++k) {
        if ((rc = admit(cs[k], e))) return rc;
        const bool holds = front_batchable(cs[k]), shares = holds && cs[k]->front.F == cs[0]->front.F;
        if (one_message && !shares) { set_error(w + ": the contexts do not share one factor"); return DOTS_ERR_STATE; }
        if (!holds) { set_error(w + ": every context needs an installed or shared factor on one GPU (no PCG, no time slab)"); return DOTS_ERR_STATE; }
        if (!shares) { set_error(w + ": the contexts do not share one factor (dots_front_share)"); return DOTS_ERR_ARGUMENT; }
        for (int j = 0; j < k && !one_message; ++j)
            if (cs[j] == cs[k]) { set_error(w + ": a context is listed twice"); return DOTS_ERR_ARGUMENT; }
    }
    out.cv.assign(cs, cs + n);
    for (Ctx *c : out.cv) { out.bh.push_back(c->d.cg_p0); out.ys.push_back(c->d.cg_z); out.xs.push_back(c->d.cg_x); }      // (front_batchable: one GPU, the PCG view is d)
    return 0;
}

int dots_front_setup(dots_ctx *c, const dots_front_desc *desc) {
    int rc = admit(c, E_FRONT_SETUP);
    if (rc) return rc;
    if (c->lap_solver != DOTS_LAP_MODAL_PCG) { set_error("the direct solve needs the modal solver"); return DOTS_ERR_ARGUMENT; }
    c->d.cn_sq = c->d.cn_g = c->d.cn_lo = c->d.cn_e = nullptr;
    if ((rc = front_setup(c, desc))) return rc;
    // DOTS_STEP_CARRY: the per-corner gathers steps 2+3 leave for the next right-hand side / projection (one GPU, pitch <= 128);
    // they belong to the direct solver's iteration and are released with the factor
    {   // beta_mid streamed around the caches (ql_lane<BMNT>): where factor + the state an iteration touches do not fit the Infinity Cache but the
        // factor is small enough for a good part of it to stay there between the sweeps once beta_mid no longer pushes it out.  Measured, hint against
        // none (profiles/studies/r04_nontemporal.txt): knot -2.5 % (everything fits), knot63 / sphere10k / a 10k torus +9 %, tori of 20k / 40k / 60k vertices
        // +3.3 / +3.7 / +5.0 %, 80k +0.3 %, 100k -0.5 %; T = 63: 20k +2.3 %, 40k +0.1...1.5 %; T = 127: 20k -0.2...+1.7 %, 65k -2 %
        // (the sweeps of the last four touch 0.92-3.1 GB): on up to 0.9 GB
        const double mall = 256.0 * 1048576.0, F8 = 8.0 * (double)c->d.F * (double)c->d.TP, V8 = 8.0 * (double)c->d.V * (double)c->d.TP;
        const double touched = 33.0 * F8 + 12.0 * V8;      // beta_mid, B, E, the carried sums; the vertex arrays
        int nt = -1;
        if (!env_int("DOTS_BM_NT", 0, 1, &nt)) { front_release(c); return DOTS_ERR_ARGUMENT; }
        const double factor = 0.5 * c->sched.bytes;      // what the sweeps touch: every block is read by both sweeps (the zero blocks of merged nodes are never read)
        c->sched.bm_nt = nt >= 0 ? nt : (factor < 0.9e9 && factor + touched > mall ? 1 : 0);
    }
    return front_carry_alloc(c);
}

int dots_front_share(dots_ctx *c, dots_ctx *owner) {
    int rc = admit(c, E_FRONT_SHARE);
    if (rc) return rc;
    if ((rc = admit(owner, E_FRONT_SHARE_OWNER))) return rc;
    if (owner == c) { set_error("front_share: a context cannot share its own factor"); return DOTS_ERR_ARGUMENT; }
    if (owner->front.n_nodes == 0) { set_error("front_share: the owner has no factor installed"); return DOTS_ERR_STATE; }
    if (owner->shard_stride != 0 || c->shard_stride != 0) { set_error("front_share: time slabs cannot share a factor"); return DOTS_ERR_STATE; }
    if (c->lap_solver != DOTS_LAP_MODAL_PCG) { set_error("the direct solve needs the modal solver"); return DOTS_ERR_ARGUMENT; }
    char buf[256] = {0};
    const Dev &a = c->d, &b = owner->d;
    if (c->device != owner->device) snprintf(buf, sizeof buf, "device %d, the owner's %d", c->device, owner->device);
    else if (a.V != b.V || a.F != b.F || a.T != b.T) snprintf(buf, sizeof buf, "V, F, T = %d, %d, %d, the owner's %d, %d, %d", a.V, a.F, a.T, b.V, b.F, b.T);
    else if (c->nnz != owner->nnz) snprintf(buf, sizeof buf, "%d Laplacian entries, the owner's %d", c->nnz, owner->nnz);
    else if (c->prm.eps != owner->sched.eps) snprintf(buf, sizeof buf, "eps %.17g, the owner's factor was built with %.17g", c->prm.eps, owner->sched.eps);
    else if (a.TP != b.TP || a.cg_ncol != b.cg_ncol) snprintf(buf, sizeof buf, "mode pitch %d, the owner's %d", a.TP, b.TP);      // (neither is a time slab)
    else if (c->lap_hash != owner->lap_hash) snprintf(buf, sizeof buf, "another mesh or vertex numbering (the Laplacian or the vertex masses differ)");
    if (buf[0]) { set_error(std::string("front_share: the factor does not fit this context: ") + buf); return DOTS_ERR_ARGUMENT; }
    // what every sharer reads is the owner's store; the update planes and the carried gathers are the sharer's own
    c->d.cn_sq = c->d.cn_g = c->d.cn_lo = c->d.cn_e = nullptr;
    front_release(c);
    c->front = owner->front;
    c->front.W = nullptr;
    c->sched = owner->sched;
    const double *w = nullptr;
    if ((rc = c->front_own.upload<double>(&w, nullptr, owner->sched.w_rows << c->d.tp_shift, c->stream))) { front_release(c); return rc; }
    c->front.W = const_cast<double *>(w);
    c->front_store = owner->front_store;
    c->front_record = owner->front_record;      // (dots_move_vertices_many refreshes the store from whichever holder is listed first)
    c->use_front = 1;
    return front_carry_alloc(c);
}

int dots_laplacian_solve_many(dots_ctx *const *cs, int n, const double *const *host_in, double *const *host_out) {
    if (!cs || n < 1 || !host_in || !host_out) { set_error("laplacian_solve_many: bad arguments"); return DOTS_ERR_ARGUMENT; }
    for (int k = 0; k < n; ++k)
        if (!host_in[k] || !host_out[k]) { set_error("laplacian_solve_many: null array"); return DOTS_ERR_ARGUMENT; }
    BatchMembers m;
    int rc = batch_members(E_LAPLACIAN_SOLVE_MANY, cs, n, m);
    if (rc) return rc;
    const int64_t cnt = array_count_device(cs[0]->d, DOTS_PHI), nh = array_count_host(cs[0]->d, DOTS_PHI);
    std::vector<double *> din((size_t)n, nullptr), dout((size_t)n, nullptr);
    DevicePool tmp(cs[0]->device);
    auto enqueue = [&]() -> int {
        int r;
        // per member, on its own stream: the input in device layout and its forward time transform (as step 1 forms them)
        for (int k = 0; k < n; ++k) {
            Ctx *c = cs[k];
            if ((r = tmp.alloc(&din[k], cnt, c->stream, false)) || (r = tmp.alloc(&dout[k], cnt, c->stream, false))) return r;
            DOTS_HIP(hipMemcpyAsync(c->stage, host_in[k], sizeof(double) * (size_t)nh, hipMemcpyHostToDevice, c->stream));
            if ((r = launch_to_device_layout(c, DOTS_PHI, din[k], c->stage))) return r;
            modes_forward(c, din[k], c->d.cg_p0, true);
        }
        // the sweeps of all members on the first member's stream, then each member's inverse transform on its own
        for (int k = 1; k < n; ++k)
            if ((r = batch_wait(cs[0], cs[k]))) return r;
        if ((r = front_solve_many(m.cv.data(), n, m.bh.data(), m.ys.data(), m.xs.data()))) return r;
        for (int k = 0; k < n; ++k) {
            Ctx *c = cs[k];
            if ((r = batch_wait(c, cs[0]))) return r;
            if ((r = modes_inverse(c, c->d.cg_x, dout[k], true))) return r;
            if ((r = launch_from_device_layout(c, DOTS_PHI, dout[k], c->stage))) return r;
            DOTS_HIP(hipMemcpyAsync(host_out[k], c->stage, sizeof(double) * (size_t)nh, hipMemcpyDeviceToHost, c->stream));
        }
        return 0;
    };
    rc = enqueue();
    for (int k = 0; k < n; ++k) (void)hipStreamSynchronize(cs[k]->stream);      // (every member's, before the buffers go)
    if (rc) return rc;
    DOTS_HIP(hipGetLastError());
    return 0;
}

int dots_step_many(dots_ctx *const *cs, int n, dots_step_stats *stats) {
    if (!cs || n < 1) { set_error("step_many: bad arguments"); return DOTS_ERR_ARGUMENT; }
    BatchMembers m;
    int rc = batch_members(E_STEP_MANY, cs, n, m);      // (the iteration consumes the flags and a pending division itself)
    if (rc) return rc;
    Ctx *c0 = cs[0];
    const std::vector<Ctx *> &cv = m.cv;
    std::vector<IterPlan> plan((size_t)n);
    const bool timed = stats != nullptr;
    hipEvent_t *ev = c0->ev;      // (stats: the batch's phases on the first member's stream)
    if (timed) {
        for (int k = 1; k < n; ++k) if ((rc = batch_wait(c0, cv[k]))) return rc;
        DOTS_HIP(hipEventRecord(ev[0], c0->stream));
        for (int k = 1; k < n; ++k) if ((rc = batch_wait(cv[k], c0))) return rc;
    }
    // each member on its own stream: the first half of its iteration and the forward time transform of its right-hand side
    for (int k = 0; k < n; ++k) {
        Ctx *c = cv[k];
        c->carried.rhs_ahead_armed = 0;      // (DOTS_STEP_RHS_AHEAD is ignored in a batch; a launch ahead already enqueued is still taken)
        c->batched = 1;
        IterPlan &p = plan[(size_t)k];
        if ((rc = iteration_before(c, false, p, nullptr))) return rc;
        if (!rhs_writes_modes(c)) modes_forward(c, c->d.cg_b, c->d.cg_p0, true);
        c->last_cg_iters = 0;
    }
    for (int k = 1; k < n; ++k) if ((rc = batch_wait(c0, cv[k]))) return rc;
    if (timed) DOTS_HIP(hipEventRecord(ev[1], c0->stream));
    if ((rc = front_solve_many(m.cv.data(), n, m.bh.data(), m.ys.data(), m.xs.data()))) return rc;
    if (timed) DOTS_HIP(hipEventRecord(ev[2], c0->stream));
    // each member behind the sweeps: inverse transform (unless its projection takes it), projection, steps 2+3
    for (int k = 0; k < n; ++k) {
        Ctx *c = cv[k];
        if ((rc = batch_wait(c, c0))) return rc;
        if (!plan[(size_t)k].fuse && (rc = modes_inverse(c, c->d.cg_x, c->d.phi, true))) return rc;
        if ((rc = iteration_after(c, plan[(size_t)k], nullptr))) return rc;
    }
    DOTS_HIP(hipGetLastError());
    if (timed) {
        for (int k = 1; k < n; ++k) if ((rc = batch_wait(c0, cv[k]))) return rc;
        DOTS_HIP(hipEventRecord(ev[3], c0->stream));
        DOTS_HIP(hipEventSynchronize(ev[3]));
        memset(stats, 0, sizeof *stats);
        float t;
        DOTS_HIP(hipEventElapsedTime(&t, ev[0], ev[1])); stats->ms_rhs = t;
        DOTS_HIP(hipEventElapsedTime(&t, ev[1], ev[2])); stats->ms_laplacian = t;
        DOTS_HIP(hipEventElapsedTime(&t, ev[2], ev[3])); stats->ms_q_lambda_multiplier = t;      // (projection included)
        DOTS_HIP(hipEventElapsedTime(&t, ev[0], ev[3])); stats->ms_total = t;
        stats->alm_iterations = n;
    }
    return 0;
}

int dots_bench_many(dots_ctx *const *cs, int n, int reps, double *ms) {
    if (!cs || n < 1 || reps < 1 || !ms) { set_error("bench_many: bad arguments"); return DOTS_ERR_ARGUMENT; }
    BatchMembers m;
    int rc = batch_members(E_BENCH_MANY, cs, n, m, true);
    if (rc) return rc;
    const std::vector<Ctx *> &cv = m.cv;
    Ctx *c0 = cv[0];
    for (int k = 1; k < n; ++k) if ((rc = batch_wait(c0, cv[k]))) return rc;
    for (int i = 0; i < 2; ++i) if ((rc = front_solve_many(m.cv.data(), n, m.bh.data(), m.ys.data(), m.xs.data()))) return rc;
    DOTS_HIP(hipEventRecord(c0->ev[6], c0->stream));
    for (int i = 0; i < reps; ++i) if ((rc = front_solve_many(m.cv.data(), n, m.bh.data(), m.ys.data(), m.xs.data()))) return rc;
    DOTS_HIP(hipEventRecord(c0->ev[7], c0->stream));
    DOTS_HIP(hipEventSynchronize(c0->ev[7]));
    float t;
    DOTS_HIP(hipEventElapsedTime(&t, c0->ev[6], c0->ev[7]));
    *ms = t / reps;
    for (int k = 1; k < n; ++k) if ((rc = batch_wait(cv[k], c0))) return rc;
    return 0;
}

// ---- carrying the state from one context to another (dots_prolong_time, dots_prolong_space, dots_transfer_space, dots_carry_spacetime) --
// What the four entry points share.  An entry point calls carry_guard, validates its descriptor -- a bad argument leaves both contexts
// untouched --, lists its tables in a CarryTables record and calls carry_state.  carry_state brings the source up to date, prepares the
// destination, puts the tables one after another into one device buffer (doubles first keeps them aligned) and, with both streams
// ordered, calls launch_carry with the device's copy of the record for each of the twelve arrays.  The order is the protocol: the
// destination's stream waits for what the source has enqueued, whatever the source does next -- its release included -- comes after the
// reads, and the buffer is freed after the synchronise, also when a launch failed.  `what`: the tables' noun in the messages.
static int carry_guard(const std::string &who, const dots_ctx *dst, const dots_ctx *src, const void *desc) {
    if (!dst || !src || !desc) { set_error(who + ": null argument"); return DOTS_ERR_ARGUMENT; }
    if (dst == src) { set_error(who + ": source and destination are one context"); return DOTS_ERR_ARGUMENT; }
    if (dst->shard_stride != 0 || src->shard_stride != 0) { set_error(who + ": not available on time slabs"); return DOTS_ERR_STATE; }
    if (dst->device != src->device) { set_error(who + ": the contexts are on different devices"); return DOTS_ERR_STATE; }
    return 0;
}

// the two carriers in space: both levels have one time grid, no table is missing, and the tables are those of the destination's mesh
static int carry_space_shapes(const char *who, const char *what, const Dev &dd, const Dev &ds, bool null_table, int n_vertices, int n_triangles) {
    char buf[200];
    if (dd.T != ds.T) snprintf(buf, sizeof buf, "%s: n_time = %d, the source's %d: both levels have one time grid", who, dd.T, ds.T);
    else if (null_table) snprintf(buf, sizeof buf, "%s: null %s", who, what);
    else if (n_vertices != dd.V || n_triangles != dd.F)
        snprintf(buf, sizeof buf, "%s: %ss of %d vertices and %d triangles, the destination has %d and %d", who, what, n_vertices, n_triangles, dd.V, dd.F);
    else return 0;
    set_error(buf);
    return DOTS_ERR_ARGUMENT;
}

// every time-table entry names two source time points of the row it reads
static int check_time_tables(const char *who, const CarryTables &t, const Dev &dd, const Dev &ds) {
    const int nn = dd.T + 1, ni = dd.T;
    for (int i = 0; i < nn + ni; ++i) {
        const bool node = i < nn;
        const int j = node ? t.node_j[i] : t.interval_j[i - nn];
        const double w = node ? t.node_w[i] : t.interval_w[i - nn];
        const int top = std::max((node ? ds.T + 1 : ds.T) - 2, 0);
        if (j < 0 || j > top || !(w >= 0.0 && w <= 1.0)) {
            char buf[240];
            snprintf(buf, sizeof buf, "%s: %s table entry %d (j = %d, w = %g) out of range (0 <= j <= %d, 0 <= w <= 1)", who, node ? "node" : "interval",
                     node ? i : i - nn, j, w, top);
            set_error(buf);
            return DOTS_ERR_ARGUMENT;
        }
    }
    return 0;
}

static size_t carry_rows_per_vertex(int mode) { return mode == CARRY_SAME ? 1 : (mode == CARRY_NESTED ? 2 : 3); }

// every index that was passed names a row / a corner of the source; every weight is a finite number >= 0.  vname, fname: what the
// entry point's descriptor calls the vertex and the triangle table
static int check_space_tables(const std::string &who, const char *vname, const char *fname, const CarryTables &t, const Dev &dd, const Dev &ds) {
    const size_t nv = carry_rows_per_vertex(t.mode) * (size_t)dd.V, nf = (size_t)dd.F;
    for (size_t i = 0; t.vsrc && i < nv; ++i) {
        if (t.vsrc[i] < 0 || t.vsrc[i] >= ds.V) { set_error(who + ": " + vname + " entry out of range"); return DOTS_ERR_ARGUMENT; }
        if (t.vw && !(t.vw[i] >= 0.0 && std::isfinite(t.vw[i]))) { set_error(who + ": a weight that is negative or not finite"); return DOTS_ERR_ARGUMENT; }
    }
    for (size_t i = 0; t.fsrc && i < nf; ++i)
        if (t.fsrc[i] < 0 || t.fsrc[i] >= ds.F) { set_error(who + ": " + fname + " entry out of range"); return DOTS_ERR_ARGUMENT; }
    for (size_t i = 0; t.csrc && i < 3 * nf; ++i)
        if (t.csrc[i] < 0 || t.csrc[i] > 2) { set_error(who + ": csrc entry outside 0 .. 2"); return DOTS_ERR_ARGUMENT; }
    return 0;
}

static int carry_state(Entry e_src, Entry e_dst, const char *what, dots_ctx *dst, dots_ctx *src, const double *factor, double *ms, const CarryTables &host) {
    const std::string who = ADMISSION[e_dst].name;
    int rc = admit(src, e_src);      // (a pending penalty division is carried out, as for a download)
    if (rc || (rc = need_zmid(src, e_src)) || (rc = admit(dst, e_dst))) return rc;
    dst->carried.pending_div = 0.0;      // (every array a pending division would have touched is replaced)
    const size_t nn = (size_t)dst->d.T + 1, ni = (size_t)dst->d.T, V = (size_t)dst->d.V, F = (size_t)dst->d.F, per = carry_rows_per_vertex(host.mode);
    const void *from[8] = {host.node_w, host.interval_w, host.vw, host.node_j, host.interval_j, host.vsrc, host.fsrc, host.csrc};
    const size_t size[8] = {sizeof(double) * nn, sizeof(double) * ni, sizeof(double) * 3 * V, sizeof(int32_t) * nn,
                            sizeof(int32_t) * ni, sizeof(int32_t) * per * V, sizeof(int32_t) * F, sizeof(int32_t) * 3 * F};
    size_t bytes = 0;
    for (int k = 0; k < 8; ++k) bytes += from[k] ? size[k] : 0;
    char *buf = nullptr, *at[8];
    DevicePool tmp(dst->device);      // (freed behind the stream synchronisation below)
    if ((rc = tmp.alloc(&buf, (int64_t)bytes, dst->stream, false))) return rc;
    hipError_t e = hipSuccess;
    bytes = 0;
    for (int k = 0; k < 8; ++k) {
        at[k] = from[k] ? buf + bytes : nullptr;      // (a table that was not passed stays null)
        if (e == hipSuccess && from[k]) e = hipMemcpyAsync(at[k], from[k], size[k], hipMemcpyHostToDevice, dst->stream);
        bytes += from[k] ? size[k] : 0;
    }
    const CarryTables dev{(const int32_t *)at[3], (const int32_t *)at[4], (const double *)at[0], (const double *)at[1], (const int32_t *)at[5],
                          (const double *)at[2], (const int32_t *)at[6], (const int32_t *)at[7], host.mode};
    if (e != hipSuccess) rc = hip_fail(e, (who + ": " + what + "s").c_str(), __FILE__, __LINE__);
    // the destination's stream waits for what the source has enqueued (its last step, the division, z_mid)
    if (!rc) rc = batch_wait(dst, src);
    if (!rc && (e = hipEventRecord(dst->ev[0], dst->stream)) != hipSuccess) rc = hip_fail(e, "hipEventRecord", __FILE__, __LINE__);
    const int group[DOTS_N_ARRAYS] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3};      // recorver_scaled_solution (solver_socp.py:397-405)
    for (int id = 0; id < DOTS_N_ARRAYS && !rc; ++id) rc = launch_carry(dst, src, id, dev, factor[group[id]], who.c_str());
    if (!rc && (e = hipEventRecord(dst->ev[1], dst->stream)) != hipSuccess) rc = hip_fail(e, "hipEventRecord", __FILE__, __LINE__);
    if (!rc) rc = batch_wait(src, dst);      // (whatever the source does next -- its release included -- comes after the reads)
    e = hipStreamSynchronize(dst->stream);
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
    if (rc) return rc;
    dst->carried.zmid = ZMID_STORED;      // (z_mid's storage holds the carried z_mid)
    state_changed(dst->carried);
    if (ms) {
        float t = 0.f;
        DOTS_HIP(hipEventElapsedTime(&t, dst->ev[0], dst->ev[1]));
        *ms = t;
    }
    return 0;
}

int dots_prolong_time(dots_ctx *dst, dots_ctx *src, const dots_prolong_desc *desc) {
    const char *who = "prolong_time";
    int rc = carry_guard(who, dst, src, desc);
    if (rc) return rc;
    const Dev &dd = dst->d, &ds = src->d;
    if (dd.V != ds.V || dd.F != ds.F) {
        char buf[160];
        snprintf(buf, sizeof buf, "prolong_time: V, F = %d, %d, the source's %d, %d: another mesh", dd.V, dd.F, ds.V, ds.F);
        set_error(buf);
        return DOTS_ERR_ARGUMENT;
    }
    if (!desc->node_j || !desc->node_w || !desc->interval_j || !desc->interval_w) { set_error("prolong_time: null table"); return DOTS_ERR_ARGUMENT; }
    const CarryTables t{desc->node_j, desc->interval_j, desc->node_w, desc->interval_w, desc->vmap, nullptr, desc->fmap, nullptr, CARRY_SAME};
    if ((rc = check_time_tables(who, t, dd, ds)) || (rc = check_space_tables(who, "vmap", "fmap", t, dd, ds))) return rc;
    return carry_state(E_PROLONG_TIME_SRC, E_PROLONG_TIME, "table", dst, src, desc->factor, desc->ms, t);
}

int dots_prolong_space(dots_ctx *dst, dots_ctx *src, const dots_prolong_space_desc *desc) {
    const char *who = "prolong_space";
    int rc = carry_guard(who, dst, src, desc);
    if (rc) return rc;
    const Dev &dd = dst->d, &ds = src->d;
    if ((rc = carry_space_shapes(who, "row map", dd, ds, !desc->vmap || !desc->fmap, desc->n_vertices, desc->n_triangles))) return rc;
    const CarryTables t{nullptr, nullptr, nullptr, nullptr, desc->vmap, nullptr, desc->fmap, nullptr, CARRY_NESTED};
    if ((rc = check_space_tables(who, "vmap", "fmap", t, dd, ds))) return rc;
    return carry_state(E_PROLONG_SPACE_SRC, E_PROLONG_SPACE, "row map", dst, src, desc->factor, desc->ms, t);
}

int dots_transfer_space(dots_ctx *dst, dots_ctx *src, const dots_transfer_space_desc *desc) {
    const char *who = "transfer_space";
    int rc = carry_guard(who, dst, src, desc);
    if (rc) return rc;
    const Dev &dd = dst->d, &ds = src->d;
    if ((rc = carry_space_shapes(who, "table", dd, ds, !desc->vsrc || !desc->vw || !desc->fsrc || !desc->csrc, desc->n_vertices, desc->n_triangles))) return rc;
    const CarryTables t{nullptr, nullptr, nullptr, nullptr, desc->vsrc, desc->vw, desc->fsrc, desc->csrc, CARRY_LOCATED};
    if ((rc = check_space_tables(who, "vsrc", "fsrc", t, dd, ds))) return rc;
    return carry_state(E_TRANSFER_SPACE_SRC, E_TRANSFER_SPACE, "table", dst, src, desc->factor, desc->ms, t);
}

int dots_carry_spacetime(dots_ctx *dst, dots_ctx *src, const dots_carry_spacetime_desc *desc) {
    const char *who = "carry_spacetime";
    int rc = carry_guard(who, dst, src, desc);
    if (rc) return rc;
    const Dev &dd = dst->d, &ds = src->d;
    char buf[240];
    if (dd.T == ds.T) {
        snprintf(buf, sizeof buf, "carry_spacetime: both contexts have n_time = %d: on one time grid the carriers in space (dots_prolong_space, "
                                  "dots_transfer_space) are the definition", dd.T);
        set_error(buf);
        return DOTS_ERR_ARGUMENT;
    }
    if (!desc->node_j || !desc->node_w || !desc->interval_j || !desc->interval_w || !desc->vsrc || !desc->fsrc) { set_error("carry_spacetime: null table"); return DOTS_ERR_ARGUMENT; }
    if (desc->n_vertices != dd.V || desc->n_triangles != dd.F) {
        snprintf(buf, sizeof buf, "carry_spacetime: tables of %d vertices and %d triangles, the destination has %d and %d", desc->n_vertices, desc->n_triangles, dd.V, dd.F);
        set_error(buf);
        return DOTS_ERR_ARGUMENT;
    }
    const CarryTables t{desc->node_j, desc->interval_j, desc->node_w, desc->interval_w, desc->vsrc, desc->vw, desc->fsrc, desc->csrc,
                        desc->vw ? CARRY_LOCATED : CARRY_NESTED};
    if ((rc = check_time_tables(who, t, dd, ds)) || (rc = check_space_tables(who, "vsrc", "fsrc", t, dd, ds))) return rc;
    return carry_state(E_CARRY_SPACETIME_SRC, E_CARRY_SPACETIME, "table", dst, src, desc->factor, desc->ms, t);
}

// ---- dots_restart: new end masses on a live context (include/dots_socp_hip.h) ------------------------------------------------------
int dots_restart(dots_ctx *c, const dots_restart_desc *desc) {
    if (!c || !desc || !desc->mu0 || !desc->mu1) { set_error("restart: null argument"); return DOTS_ERR_ARGUMENT; }
    if (desc->mode != DOTS_RESTART_COLD && desc->mode != DOTS_RESTART_WARM) { set_error("restart: unknown mode"); return DOTS_ERR_ARGUMENT; }
    const bool warm = desc->mode == DOTS_RESTART_WARM, on_device = desc->device_pointers != 0;
    if (c->shard_stride != 0) { set_error("restart: not available on a time slab"); return DOTS_ERR_STATE; }
    const int V = c->d.V;
    if (!on_device)
        for (int v = 0; v < V; ++v)
            if (!std::isfinite(desc->mu0[v]) || !std::isfinite(desc->mu1[v])) { set_error("restart: an end mass that is not finite"); return DOTS_ERR_ARGUMENT; }
    if (warm) {
        for (double f : desc->factors)
            if (!(std::isfinite(f) && f > 0.0)) { set_error("restart: a factor that is not finite and positive"); return DOTS_ERR_ARGUMENT; }
        if (int rc = refuse_unspecified_zmid(c->carried, E_RESTART)) return rc;
    }
    // the launch ahead, an armed penalty decision, the carried gathers, the fused sums and the step path go; the division stays for below
    int rc = admit(c, E_RESTART);
    if (rc) return rc;
    Dev &d = c->d;
    DOTS_HIP(hipEventRecord(c->ev[0], c->stream));
    if (warm) {      // what dots_download does before it reads, then the recovery factors in place
        if ((rc = flush_division(c)) || (rc = need_zmid(c, E_RESTART)) || (rc = launch_restart_scale(c, desc->factors, nullptr))) return rc;
    } else {
        c->carried.pending_div = 0.0;      // (it would have divided arrays that are zero from here on)
        if (c->carried.zmid == ZMID_DEFERRED) c->carried.zmid = ZMID_STORED;      // (nothing to rebuild it for)
        if ((rc = launch_restart_scale(c, nullptr, nullptr))) return rc;      // (one launch: a memset per array costs the host milliseconds on the large ones)
    }
    // what is derived from the state or left over from the old run's launches, as a new context has it: zero
    const size_t node_bytes = sizeof(double) * ((size_t)V << d.tp_shift);
    double *const node_arrays[] = {d.lamc, c->zf_alt, c->ze_alt, c->lamc_alt, d.cg_b, d.cg_r, d.cg_z, d.cg_p0, d.cg_p1, d.cg_Ap, d.cg_x};
    for (double *p : node_arrays)
        if (p) DOTS_HIP(hipMemsetAsync(p, 0, node_bytes, c->stream));
    // (B_alt keeps its bytes: it is read only while z_mid is deferred, and the step that sets it has written all of it)
    DOTS_HIP(hipMemsetAsync(d.scal, 0, sizeof(double) * CgScalOffsets::TOTAL, c->stream));
    DOTS_HIP(hipMemsetAsync(d.flags, 0, sizeof(int) * FLAG_TOTAL, c->stream));
    DOTS_HIP(hipMemsetAsync(c->kkt_counter, 0, 2 * sizeof(int), c->stream));
    // boundary data: the masses where the kernels read them, norm_boundary as dots_create forms it
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    DOTS_HIP(hipMemcpyAsync(const_cast<double *>(d.mu0), desc->mu0, sizeof(double) * (size_t)V, kind, c->stream));
    DOTS_HIP(hipMemcpyAsync(const_cast<double *>(d.mu1), desc->mu1, sizeof(double) * (size_t)V, kind, c->stream));
    double nb = 0.0;
    if (on_device) { if ((rc = restart_boundary_sum(c, d.mu0, d.mu1, &nb))) return rc; }
    else nb = boundary_sum(desc->mu0, desc->mu1, c->mass_host->data(), V);
    DOTS_HIP(hipEventRecord(c->ev[1], c->stream));
    DOTS_HIP(hipStreamSynchronize(c->stream));      // (host arrays are borrowed for the call only; the ring's events and the mailbox are idle from here)
    fresh_run_params(c);      // (tau, eps, cg_tol, cg_max_iter stay)
    c->prm.norm_d = c->norm_d0;
    c->prm.norm_boundary = boundary_norm(nb, d.T);
    // host bookkeeping of the old run
    c->carried.zmid = ZMID_STORED;
    c->carried.needs_restart = 0;      // (after dots_move_vertices: the run that starts here is one on the new surface)
    c->zmid_dv = c->zmid_sz = 0.0;
    c->ahead_dv = c->ahead_r = c->carried.ahead_div = 0.0;
    state_changed(c->carried);
    c->step_timed = c->step_skip_zmid = c->step_palm = c->step_kkt = c->step_carry = 0;
    c->batched = 0;
    c->t_head = c->t_count = 0;
    c->last_cg_iters = 0;
    c->cgc.last_iters = 0;
    for (auto &k : c->cgw) k.last_iters = 0;
    c->pcg_windows_ran = 0;
    c->mail_seq = 0;
    for (int i = 0; i < MAX_SUMS + 8; ++i) c->h_mail[i] = 0.0;
    if (desc->ms) {
        float t = 0.f;
        DOTS_HIP(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
        *desc->ms = t;
    }
    return 0;
}

// ---- dots_move_vertices, dots_move_vertices_many: other vertex positions on live contexts (include/dots_socp_hip.h) -----------------
// cs[0 .. n) move together.  Every check runs for every member before any member changes; the positions are validated once, into the
// scratch of cs[0]; then each member does on its own stream what a move does to one context, all take the host constants of one
// download, and the factor they hold is refreshed once, on cs[0]'s stream, with every stream idle before and after.  `many`: the list
// is the caller's (dots_move_vertices_many) and must be the whole set of holders of the store; otherwise cs is one context, which
// must hold its store alone.
static int move_holders(dots_ctx *const *cs, int n, const dots_move_desc *desc, bool many) {
    dots_ctx *c0 = cs[0];
    const int V = c0->d.V, F = c0->d.F, nnz = c0->nnz;
    for (int k = 0; k < n; ++k) {
        const Ctx *c = cs[k];
        if (c->shard_stride != 0) { set_error("move_vertices: not available on a time slab"); return DOTS_ERR_STATE; }
        if (c->lap_solver != DOTS_LAP_MODAL_PCG) { set_error("move_vertices: the context is not modal (DOTS_LAP_MODAL_PCG)"); return DOTS_ERR_STATE; }
        if (c->mg.nlev >= 2) { set_error("move_vertices: a multigrid hierarchy is installed (its coarse operators belong to the old surface)"); return DOTS_ERR_STATE; }
    }
    if (!many && c0->front_store && c0->front_store.use_count() > 1) {
        set_error("move_vertices: the factor store is shared (dots_front_share): a sharer cannot move it, and an owner not under its sharers");
        return DOTS_ERR_STATE;
    }
    if (many) {
        bool whole = c0->front_store ? (long)n == c0->front_store.use_count() : n == 1;
        for (int k = 1; k < n; ++k) {
            whole = whole && cs[k]->front_store == c0->front_store;
            for (int j = 0; j < k; ++j) whole = whole && cs[j] != cs[k];
        }
        if (!whole) {
            set_error("move_vertices_many: the list is not the set of holders of one factor store (every context that shares it, each once)");
            return DOTS_ERR_STATE;
        }
        // (one store: one mesh, Laplacian and vertex numbering, dots_front_share; the scratch of cs[0] also serves the triangle tables of all)
        for (int k = 1; k < n; ++k)
            if (cs[k]->tri_hash != c0->tri_hash || cs[k]->d.F != F) {
                set_error("move_vertices_many: the members number their triangles or corner lists differently");
                return DOTS_ERR_STATE;
            }
    }
    const bool on_device = desc->device_pointers != 0;
    if (!on_device)
        for (int64_t i = 0; i < (int64_t)3 * V; ++i)
            if (!std::isfinite(desc->vertices[i])) { set_error("move_vertices: a coordinate that is not finite"); return DOTS_ERR_ARGUMENT; }
    hipError_t e0 = hipSetDevice(c0->device);
    if (e0 != hipSuccess) return hip_fail(e0, "hipSetDevice", __FILE__, __LINE__);
    int rc;
    // scratch in the staging buffer: [area F | hat 9 F | mass V | flag | xyz 3 V], every part on a 16-byte boundary
    auto even = [](int64_t n) { return (n + 1) & ~(int64_t)1; };
    const int64_t o_hat = even(F), o_mass = o_hat + even((int64_t)9 * F), o_flag = o_mass + even(V), o_xyz = o_flag + 2, total = o_xyz + (int64_t)3 * V;
    for (int k = 0; k < n; ++k) {
        if ((rc = front_refresh_check(cs[k]))) return rc;
        if (total > cs[k]->stage_count) { set_error("move_vertices: the scratch tables do not fit the staging buffer on this mesh"); return DOTS_ERR_STATE; }
    }
    // what dots_download does before it reads, with the OLD geometry (z_mid is rebuilt from tables that are about to change); the launch
    // ahead, an armed penalty decision, the carried gathers and the fused sums go
    const Entry e = many ? E_MOVE_VERTICES_MANY : E_MOVE_VERTICES;
    for (int k = 0; k < n; ++k)
        if ((rc = admit(cs[k], e)) || (rc = need_zmid(cs[k], e))) return rc;
    GeomScratch s{c0->stage, c0->stage + o_hat, c0->stage + o_mass, reinterpret_cast<int *>(c0->stage + o_flag)};
    const double *xyz = desc->vertices;
    if (!on_device) {
        DOTS_HIP(hipMemcpyAsync(c0->stage + o_xyz, desc->vertices, sizeof(double) * (size_t)3 * V, hipMemcpyHostToDevice, c0->stream));
        xyz = c0->stage + o_xyz;
    }
    DOTS_HIP(hipEventRecord(c0->ev[0], c0->stream));
    if ((rc = launch_geometry_validate(c0, xyz, s))) return rc;
    DOTS_HIP(hipEventRecord(c0->ev[1], c0->stream));
    int flag = 0;
    DOTS_HIP(hipMemcpyAsync(&flag, s.flag, sizeof(int), hipMemcpyDeviceToHost, c0->stream));
    DOTS_HIP(hipStreamSynchronize(c0->stream));      // (host positions are borrowed for the call only)
    if (flag) {
        set_error("move_vertices: a coordinate that is not finite, a triangle whose area is not positive or a vertex whose mass is not positive; the context keeps its geometry");
        return DOTS_ERR_ARGUMENT;
    }
    // from here on the contexts are on the new surface: each member's tables from the one scratch (complete: the host has waited for
    // it), behind the flush on its own stream; the host constants of the run (run_constants: sequential sums over the tables) from one download
    std::vector<double> area((size_t)F), val((size_t)nnz);
    std::vector<std::vector<double>> mu((size_t)2 * n, std::vector<double>((size_t)V));
    auto mass = std::make_shared<std::vector<double>>((size_t)V);      // (a new vector: whoever shares the old one keeps it)
    for (int k = 0; k < n; ++k) {
        dots_ctx *c = cs[k];
        const Dev &d = c->d;
        DOTS_HIP(hipEventRecord(c->ev[2], c->stream));
        if ((rc = launch_geometry_commit(c, s))) return rc;
        DOTS_HIP(hipEventRecord(c->ev[3], c->stream));
        c->carried.needs_restart = 1;
        state_changed(c->carried);
        if (k == 0) {
            DOTS_HIP(hipMemcpyAsync(area.data(), d.area_f, sizeof(double) * (size_t)F, hipMemcpyDeviceToHost, c->stream));
            DOTS_HIP(hipMemcpyAsync(mass->data(), d.mass_v, sizeof(double) * (size_t)V, hipMemcpyDeviceToHost, c->stream));
            DOTS_HIP(hipMemcpyAsync(val.data(), d.val, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost, c->stream));
            c->d2h_bytes += (int64_t)sizeof(double) * ((int64_t)F + (int64_t)V + nnz);
        }
        DOTS_HIP(hipMemcpyAsync(mu[(size_t)2 * k].data(), d.mu0, sizeof(double) * (size_t)V, hipMemcpyDeviceToHost, c->stream));
        DOTS_HIP(hipMemcpyAsync(mu[(size_t)2 * k + 1].data(), d.mu1, sizeof(double) * (size_t)V, hipMemcpyDeviceToHost, c->stream));
        c->d2h_bytes += (int64_t)sizeof(double) * 2 * (int64_t)V;
    }
    for (int k = 0; k < n; ++k) DOTS_HIP(hipStreamSynchronize(cs[k]->stream));      // (no member has anything in flight when the refresh starts)
    const std::vector<Ctx *> cv(cs, cs + n);
    std::vector<const double *> ends;
    for (const std::vector<double> &m : mu) ends.push_back(m.data());
    run_constants(cv.data(), n, mass, area.data(), val.data(), ends.data());
    // the factor the members hold, from K + (sigma_a + eps) M of the new tables, into the allocations it has: once
    DOTS_HIP(hipEventRecord(c0->ev[6], c0->stream));
    if (c0->front.n_nodes > 0 && (rc = front_refresh(c0))) {
        (void)hipStreamSynchronize(c0->stream);
        const std::string why = g_last_error;
        for (int k = 0; k < n; ++k) {
            dots_ctx *c = cs[k];
            c->d.cn_sq = c->d.cn_g = c->d.cn_lo = c->d.cn_e = nullptr;
            front_release(c);      // (a PCG context from here on, as after a failed dots_front_setup)
        }
        set_error(why);
        return rc;
    }
    DOTS_HIP(hipEventRecord(c0->ev[7], c0->stream));
    for (int k = 0; k < n; ++k) DOTS_HIP(hipStreamSynchronize(cs[k]->stream));
    if (desc->ms) {
        float a = 0.f, f = 0.f, w = 0.f;
        DOTS_HIP(hipEventElapsedTime(&a, c0->ev[0], c0->ev[1]));
        DOTS_HIP(hipEventElapsedTime(&f, c0->ev[6], c0->ev[7]));
        DOTS_HIP(hipEventElapsedTime(&w, c0->ev[0], c0->ev[7]));
        double assembly = a;
        for (int k = 0; k < n; ++k) {
            float b = 0.f;
            DOTS_HIP(hipEventElapsedTime(&b, cs[k]->ev[2], cs[k]->ev[3]));
            assembly += b;
        }
        desc->ms[0] = assembly;
        desc->ms[1] = f;
        desc->ms[2] = w;
    }
    return 0;
}

int dots_move_vertices(dots_ctx *c, const dots_move_desc *desc) {
    if (!c || !desc || !desc->vertices) { set_error("move_vertices: null argument"); return DOTS_ERR_ARGUMENT; }
    return move_holders(&c, 1, desc, false);
}

int dots_move_vertices_many(dots_ctx *const *ctxs, int n, const dots_move_desc *desc) {
    if (!ctxs || n < 1 || !desc || !desc->vertices) { set_error("move_vertices_many: null argument"); return DOTS_ERR_ARGUMENT; }
    for (int k = 0; k < n; ++k)
        if (!ctxs[k]) { set_error("move_vertices_many: null context"); return DOTS_ERR_ARGUMENT; }
    return move_holders(ctxs, n, desc, true);
}

int dots_geometry_copy(dots_ctx *c, const dots_geometry_tables *out) {
    int rc = admit(c, E_GEOMETRY_COPY);      // (reads tables only: neither the state nor the parameters)
    if (rc) return rc;
    if (!out) { set_error("geometry_copy: null argument"); return DOTS_ERR_ARGUMENT; }
    const Dev &d = c->d;
    const int64_t V = d.V, F = d.F;
    const struct { double *host; const double *dev; int64_t n; } parts[] = {
        {out->area_tri, d.area_f, F}, {out->hat_grad, d.hat, 9 * F}, {out->mass_vert, d.mass_v, V}, {out->lap_val, d.val, (int64_t)c->nnz},
        {out->kdiag, d.kdiag, V}, {out->corner_scale, d.c_D, 3 * F}, {out->corner_grad_area, d.c_gA, 9 * F}};
    DOTS_HIP(hipStreamSynchronize(c->stream));
    for (const auto &p : parts)
        if (p.host) DOTS_HIP(hipMemcpyAsync(p.host, p.dev, sizeof(double) * (size_t)p.n, hipMemcpyDeviceToHost, c->stream));
    DOTS_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- dots_readout ---------------------------------------------------------------------------------------------------------
// the inverse of the device numbering, the copy stream, the chunk events and the host memory of the layer sums: once per context
static int readout_prepare(Ctx *c) {
    if (c->readout_ready) return 0;
    const Dev &d = c->d;
    for (int pass = 0; pass < 2; ++pass) {
        const int *perm = pass ? d.perm_f : d.perm_v;
        const int n = pass ? d.F : d.V;
        if (!perm) continue;
        std::vector<int> p((size_t)n), inv((size_t)n);
        DOTS_HIP(hipMemcpyAsync(p.data(), perm, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        DOTS_HIP(hipStreamSynchronize(c->stream));
        for (int i = 0; i < n; ++i) {
            if (p[i] < 0 || p[i] >= n) { set_error("readout: the device numbering is not a permutation"); return DOTS_ERR_STATE; }
            inv[p[i]] = i;
        }
        const int *dev = nullptr;
        int rc = dev_upload(c, &dev, inv.data(), n);
        if (rc) return rc;
        (pass ? c->inv_perm_f : c->inv_perm_v) = const_cast<int *>(dev);
    }
    if (!c->copy_stream) DOTS_HIP(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (auto &ev : c->ro_ev) if (!ev) DOTS_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    for (auto &ev : c->ring_ev) if (!ev) DOTS_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    int rc = 0;
    if (!c->h_ro_sums && (rc = c->pinned.alloc(&c->h_ro_sums, 2 * 1024, hipHostMallocCoherent | hipHostMallocMapped))) return rc;
    c->readout_ready = 1;
    return 0;
}

// Device -> host copies of dots_readout on the copy stream, each behind the event of the launch that formed its layers: straight into the
// caller's memory, or (DOTS_READOUT_PINNED=<KB per slot>) through two pinned slots that the host empties while the next piece is on its way
struct ReadoutCopier {
    Ctx *c;
    size_t SLOT;                 // bytes per slot
    char *pend_host[2] = {nullptr, nullptr};
    size_t pend_n[2] = {0, 0};
    int k = 0;
    int drain(int slot) {
        if (!pend_host[slot]) return 0;
        DOTS_HIP(hipEventSynchronize(c->ring_ev[slot]));
        memcpy(pend_host[slot], c->h_ring + slot * SLOT, pend_n[slot]);
        pend_host[slot] = nullptr;
        return 0;
    }
    int copy(double *host, const double *dev, size_t bytes, hipEvent_t after) {
        DOTS_HIP(hipStreamWaitEvent(c->copy_stream, after, 0));
        c->d2h_bytes += (int64_t)bytes;
        if (!c->readout_pinned) {
            DOTS_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->copy_stream));
            return 0;
        }
        for (size_t off = 0; off < bytes; off += SLOT, ++k) {
            const int slot = k & 1;
            const size_t n = std::min(SLOT, bytes - off);
            int rc = drain(slot);
            if (rc) return rc;
            DOTS_HIP(hipMemcpyAsync(c->h_ring + slot * SLOT, (const char *)dev + off, n, hipMemcpyDeviceToHost, c->copy_stream));
            DOTS_HIP(hipEventRecord(c->ring_ev[slot], c->copy_stream));
            pend_host[slot] = (char *)host + off;
            pend_n[slot] = n;
        }
        return 0;
    }
    int finish() {
        int rc = drain(k & 1);      // (the older of the two slots first)
        if (!rc) rc = drain((k + 1) & 1);
        if (rc) return rc;
        return 0;
    }
};

int dots_readout(dots_ctx *c, const dots_readout_desc *desc) {
    if (!c) { set_error("null context"); return DOTS_ERR_ARGUMENT; }
    if (!desc) { set_error("readout: null description"); return DOTS_ERR_ARGUMENT; }
    if (c->shard_stride != 0) { set_error("readout: not available on time slabs"); return DOTS_ERR_STATE; }
    const Dev &d = c->d;
    const bool sums = desc->layer_mass || desc->layer_negative;
    const bool want_mu = desc->mu || sums;
    if (!want_mu && !desc->E) { set_error("readout: nothing requested (mu, E and the layer sums are all NULL)"); return DOTS_ERR_ARGUMENT; }
    const int centred = desc->centred ? 1 : 0;
    if (centred && (!desc->mu0 || !desc->mu1)) { set_error("readout: the centred output needs mu0 and mu1"); return DOTS_ERR_ARGUMENT; }
    if (centred && d.T < 1) { set_error("readout: no layers to centre"); return DOTS_ERR_ARGUMENT; }
    int rc = admit(c, E_READOUT);      // (a pending penalty division is carried out, as for a download; z_mid is not needed)
    if (rc) return rc;
    if ((rc = readout_prepare(c))) return rc;
    const size_t slot = (size_t)c->readout_pinned << 10;
    if (slot && !c->h_ring && (rc = c->pinned.alloc(&c->h_ring, 2 * slot, hipHostMallocDefault))) return rc;
    // the staging buffer: [E | mu | w_vertex | mu0 | mu1 | w_triangle | partial sums], every part on a 16-byte boundary
    const int layers = d.T + centred, n_wg = readout_workgroups(c);
    auto even = [](int64_t n) { return (n + 1) & ~(int64_t)1; };
    const int64_t V = d.V, F = d.F;
    const int64_t n_E = desc->E ? (int64_t)(d.T + 1) * 3 * F : 0, n_mu = want_mu ? (int64_t)layers * V : 0;
    const int64_t o_mu = even(n_E), o_wv = o_mu + even(n_mu), o_m0 = o_wv + even(V), o_m1 = o_m0 + even(V), o_wt = o_m1 + even(V);
    const int64_t o_part = o_wt + even(F), total = o_part + (sums ? (int64_t)layers * 2 * n_wg : 0);
    if (total > c->stage_count) {      // (18 F pitch doubles: reached only by a mesh with more than ~ 14 vertices per triangle)
        set_error("readout: mu, E and their weights do not fit the staging buffer (sized for z_mid) on this mesh; use dots_download");
        return DOTS_ERR_STATE;
    }
    double *st = c->stage;
    // what is enqueued; every path out of the call waits for both streams first (the uploads read the caller's arrays)
    auto enqueue = [&]() -> int {
        const double *wv = nullptr, *wt = nullptr, *m0 = nullptr, *m1 = nullptr;
        if (want_mu && desc->w_vertex) { DOTS_HIP(hipMemcpyAsync(st + o_wv, desc->w_vertex, sizeof(double) * (size_t)V, hipMemcpyHostToDevice, c->stream)); wv = st + o_wv; }
        if (want_mu && centred) {
            DOTS_HIP(hipMemcpyAsync(st + o_m0, desc->mu0, sizeof(double) * (size_t)V, hipMemcpyHostToDevice, c->stream));
            DOTS_HIP(hipMemcpyAsync(st + o_m1, desc->mu1, sizeof(double) * (size_t)V, hipMemcpyHostToDevice, c->stream));
            m0 = st + o_m0;
            m1 = st + o_m1;
        }
        if (desc->E && desc->w_triangle) { DOTS_HIP(hipMemcpyAsync(st + o_wt, desc->w_triangle, sizeof(double) * (size_t)F, hipMemcpyHostToDevice, c->stream)); wt = st + o_wt; }
        int n_ch_mu = 0, n_ch_E = 0, r = 0;
        DOTS_HIP(hipEventRecord(c->ev[0], c->stream));
        if (want_mu && (r = launch_readout(c, false, st + o_mu, c->inv_perm_v, wv, m0, m1, centred, desc->factor, sums ? st + o_part : nullptr, c->ro_ev, &n_ch_mu))) return r;
        if (desc->E && (r = launch_readout(c, true, st, c->inv_perm_f, wt, nullptr, nullptr, 0, desc->factor, nullptr, c->ro_ev + 4, &n_ch_E))) return r;
        if (sums && (r = launch_readout_fold(c, st + o_part, layers, n_wg, c->h_ro_sums))) return r;
        DOTS_HIP(hipEventRecord(c->ev[1], c->stream));
        // every chunk of layers is copied as soon as its launch has finished, while the later launches run
        ReadoutCopier cp{c, slot};
        for (int k = 0; k < n_ch_mu && desc->mu; ++k) {
            const int64_t l0 = (int64_t)k * 256, l1 = std::min<int64_t>(l0 + 256, layers);
            if ((r = cp.copy(desc->mu + l0 * V, st + o_mu + l0 * V, sizeof(double) * (size_t)((l1 - l0) * V), c->ro_ev[k]))) return r;
        }
        for (int k = 0; k < n_ch_E; ++k) {
            const int64_t l0 = (int64_t)k * 256, l1 = std::min<int64_t>(l0 + 256, d.T + 1);
            if ((r = cp.copy(desc->E + l0 * 3 * F, st + l0 * 3 * F, sizeof(double) * (size_t)((l1 - l0) * 3 * F), c->ro_ev[4 + k]))) return r;
        }
        return cp.finish();
    };
    rc = enqueue();
    const hipError_t e1 = hipStreamSynchronize(c->copy_stream), e2 = hipStreamSynchronize(c->stream);
    if (!rc && e1 != hipSuccess) rc = hip_fail(e1, "hipStreamSynchronize", __FILE__, __LINE__);
    if (!rc && e2 != hipSuccess) rc = hip_fail(e2, "hipStreamSynchronize", __FILE__, __LINE__);
    if (rc) return rc;
    for (int l = 0; l < layers && sums; ++l) {      // (written by the fold kernel itself: no copy)
        if (desc->layer_mass) desc->layer_mass[l] = c->h_ro_sums[2 * l];
        if (desc->layer_negative) desc->layer_negative[l] = c->h_ro_sums[2 * l + 1];
    }
    if (desc->ms) {
        float t = 0.f;
        DOTS_HIP(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
        *desc->ms = t;
    }
    return 0;
}

// ---- dots_flow_map --------------------------------------------------------------------------------------------------------
// the context's triangles and the inverse of its triangle numbering on the host, once per context: what the caller's tables are
// checked against and translated with
static int flow_prepare(Ctx *c) {
    if (c->flow) return 0;
    const Dev &d = c->d;
    auto fh = std::make_shared<FlowHost>();
    fh->tri.resize((size_t)d.F * 3);
    DOTS_HIP(hipMemcpyAsync(fh->tri.data(), d.tri, sizeof(int) * (size_t)d.F * 3, hipMemcpyDeviceToHost, c->stream));
    std::vector<int> perm;
    if (d.perm_f) {
        perm.resize((size_t)d.F);
        DOTS_HIP(hipMemcpyAsync(perm.data(), d.perm_f, sizeof(int) * (size_t)d.F, hipMemcpyDeviceToHost, c->stream));
    }
    DOTS_HIP(hipStreamSynchronize(c->stream));
    if (d.perm_f) {
        fh->inv_f.assign((size_t)d.F, -1);
        for (int i = 0; i < d.F; ++i) {
            if (perm[i] < 0 || perm[i] >= d.F || fh->inv_f[perm[i]] >= 0) { set_error("flow_map: the device numbering is not a permutation"); return DOTS_ERR_STATE; }
            fh->inv_f[perm[i]] = i;
        }
    }
    preload_flow_kernels();
    c->flow = fh;
    return 0;
}

// What dots_flow_map, dots_flow_push, dots_flow_trace and dots_flow_slide ask for, as one record: the embedded description, and what is
// optional beside it.  Without nodes the trace is the whole horizon, node 0 to node n_time.
struct FlowRequest {
    Entry entry;                                     // the entry point: its admission row, its name in the messages
    const dots_flow_map_desc *map;
    const dots_flow_push_desc *push = nullptr;       // the deposit fields (its `map` is not read), or null: no deposits
    bool nodes = false;                              // node_from and node_to are the caller's, and are checked
    int node_from = 0, node_to = 0;
    double *action = nullptr;                        // host out [n_particles], or null
    bool slide = false;                              // the sliding mode; `slides` is then required
    int32_t *slides = nullptr, *steps = nullptr;     // host out [n_particles]; steps may be null
};
// The request of a trace description; `deposits` holds its deposit fields as dots_flow_push takes them.
static FlowRequest flow_trace_request(Entry entry, const dots_flow_trace_desc &t, dots_flow_push_desc &deposits) {
    deposits = dots_flow_push_desc{};
    deposits.mass = t.mass; deposits.n_attributes = t.n_attributes; deposits.all_layers = t.all_layers; deposits.attributes = t.attributes;
    deposits.scale_exponent = t.scale_exponent; deposits.mass_at = t.mass_at; deposits.attr_at = t.attr_at; deposits.dropped = t.dropped;
    deposits.ms = t.ms;
    FlowRequest r{entry, &t.map};
    if (t.mass) r.push = &deposits;
    r.nodes = true; r.node_from = t.node_from; r.node_to = t.node_to; r.action = t.action;
    return r;
}
// The one call path of the four entry points: the checks of the request, the caller's starts and neighbour table in the device
// numbering (host preparation), the allocation of the call, the launch and the copies back.
static int flow_run(dots_ctx *c, const FlowRequest &req) {
    const dots_flow_map_desc *desc = req.map;
    const dots_flow_push_desc *push = req.push;
    const std::string w = std::string(ADMISSION[req.entry].name) + ": ";
    if (c->shard_stride != 0) { set_error(w + "not available on time slabs"); return DOTS_ERR_STATE; }
    const Dev &d = c->d;
    if (req.slide && !req.slides) { set_error(w + "null pointer (slides is required)"); return DOTS_ERR_ARGUMENT; }
    if (req.nodes) {
        if (req.node_from < 0 || req.node_from > d.T || req.node_to < 0 || req.node_to > d.T) { set_error(w + "a time node outside 0 .. n_time"); return DOTS_ERR_ARGUMENT; }
        if (req.node_from == req.node_to) { set_error(w + "node_from equals node_to: no interval to trace"); return DOTS_ERR_ARGUMENT; }
    }
    const bool outputs = desc->triangle && desc->weights && desc->status && desc->rested && desc->crossings;
    if (!desc->start_triangle || !desc->start_weights || !desc->neighbours || (!push && !outputs)) {
        set_error(w + (push ? "null pointer (start_triangle, start_weights and neighbours are required)"
                            : "null pointer (start_triangle, start_weights, neighbours and the five outputs are required)"));
        return DOTS_ERR_ARGUMENT;
    }
    const int A = push ? push->n_attributes : 0;
    if (push) {
        if (!push->mass || !push->scale_exponent || !push->mass_at) { set_error(w + "null pointer (mass, scale_exponent and mass_at are required)"); return DOTS_ERR_ARGUMENT; }
        if (A < 0 || A > FLOW_PUSH_CHANNELS - 1) { set_error(w + "n_attributes outside 0 .. 4"); return DOTS_ERR_ARGUMENT; }
        if (A > 0 && (!push->attributes || !push->attr_at)) { set_error(w + "attributes and attr_at are required with n_attributes > 0"); return DOTS_ERR_ARGUMENT; }
        for (int ch = 0; ch <= A; ++ch)
            if (push->scale_exponent[ch] < -1000 || push->scale_exponent[ch] > 1000) { set_error(w + "a scale exponent outside -1000 .. 1000"); return DOTS_ERR_ARGUMENT; }
    }
    if (desc->n_particles < 1) { set_error(w + "n_particles < 1"); return DOTS_ERR_ARGUMENT; }
    if (desc->max_crossings < 1 || desc->max_crossings > 255) { set_error(w + "max_crossings outside 1 .. 255"); return DOTS_ERR_ARGUMENT; }
    if (std::isnan(desc->floor)) { set_error(w + "the floor is not a number"); return DOTS_ERR_ARGUMENT; }
    if (d.F >= FLOW_MAX_TRIANGLES) { set_error(w + "more than 2^27 triangles"); return DOTS_ERR_ARGUMENT; }
    hipError_t e0 = hipSetDevice(c->device);
    if (e0 != hipSuccess) return hip_fail(e0, "hipSetDevice", __FILE__, __LINE__);
    int rc = flow_prepare(c);
    if (rc) return rc;
    const FlowHost &fh = *c->flow;
    const int P = desc->n_particles, F = d.F, T = d.T;
    const int node_from = req.nodes ? req.node_from : 0, node_to = req.nodes ? req.node_to : T;
    const int n_turns = std::abs(node_to - node_from);      // intervals traversed
    auto to_dev = [&](int f) { return fh.inv_f.empty() ? f : fh.inv_f[f]; };
    // the starts, in the device numbering
    std::vector<int> h_start((size_t)P);
    for (int p = 0; p < P; ++p) {
        const int f = desc->start_triangle[p];
        if (f < 0 || f >= F) { set_error(w + "a start triangle out of range"); return DOTS_ERR_ARGUMENT; }
        h_start[p] = to_dev(f);
    }
    for (size_t i = 0; i < (size_t)P * 3; ++i)
        if (!(desc->start_weights[i] >= 0.0 && std::isfinite(desc->start_weights[i]))) {
            set_error(w + "a weight that is negative or not finite");
            return DOTS_ERR_ARGUMENT;
        }
    // the neighbour table, in the device numbering, every entry with the corners of the neighbour that name the two shared vertices
    std::vector<int> h_nbr((size_t)F * 3);
    for (int f = 0; f < F; ++f) {
        const int fd = to_dev(f);
        for (int k = 0; k < 3; ++k) {
            const int g = desc->neighbours[(size_t)f * 3 + k];
            if (g < -1 || g >= F) { set_error(w + "a neighbour index out of range"); return DOTS_ERR_ARGUMENT; }
            if (g < 0) { h_nbr[(size_t)fd * 3 + k] = -1; continue; }
            const int gd = to_dev(g);
            const int va = fh.tri[(size_t)fd * 3 + (k + 1) % 3], vb = fh.tri[(size_t)fd * 3 + (k + 2) % 3];
            int ca = -1, cb = -1;
            for (int m = 0; m < 3; ++m) {
                if (fh.tri[(size_t)gd * 3 + m] == va) ca = m;
                if (fh.tri[(size_t)gd * 3 + m] == vb) cb = m;
            }
            if (g == f || ca < 0 || cb < 0 || ca == cb) { set_error(w + "a neighbour entry that does not share the edge opposite its corner"); return DOTS_ERR_ARGUMENT; }
            h_nbr[(size_t)fd * 3 + k] = flow_pack_neighbour(gd, ca, cb);
        }
    }
    // what the particles carry: finite, and small enough for the caller's exponents -- sum_p |g| max(1, (w0 + w1) + w2) 2^k_c <= 2^61
    FlowPush q{};
    FlowPushFinish fin{};
    if (push) {
        for (int ch = 0; ch <= A; ++ch) {
            double sum = 0.0;
            for (int p = 0; p < P; ++p) {
                const double g = ch == 0 ? push->mass[p] : push->mass[p] * push->attributes[(size_t)(ch - 1) * P + p];
                if (!std::isfinite(g)) { set_error(w + (ch == 0 ? "a mass that is not finite" : "a mass times an attribute that is not finite")); return DOTS_ERR_ARGUMENT; }
                const double *sw = desc->start_weights + (size_t)p * 3;
                const double wsum = (sw[0] + sw[1]) + sw[2];
                sum += std::fabs(g) * (1.0 > wsum ? 1.0 : wsum);
            }
            q.k[ch] = push->scale_exponent[ch];
            fin.unscale[ch] = std::ldexp(1.0, -push->scale_exponent[ch]);
            if (!(sum * std::ldexp(1.0, q.k[ch]) <= 0x1p61)) { set_error(w + "a scale exponent too large for what the particles carry (flow.push_scales chooses one)"); return DOTS_ERR_ARGUMENT; }
        }
    }
    if ((rc = admit(c, req.entry))) return rc;      // (a pending penalty division is carried out, as for a download; z_mid is not needed)
    if (push && (rc = readout_prepare(c))) return rc;      // (the inverse of the vertex numbering is the read-out's)
    // one allocation for the call: [start_w | o_w | w_at | mass | attr | pushed | action] doubles, [acc | dropped] 64-bit words, then
    // [start | nbr | o_tri | status | rested | crossings | slides | steps | tri_at] ints (the five counters in a row: FlowSlide::o_counts)
    const size_t layers = (size_t)n_turns + 1;
    const size_t n_wat = desc->weights_at ? layers * P * 3 : 0, n_tat = desc->triangles_at ? layers * P : 0;
    const size_t L = push ? (push->all_layers ? layers : 1) : 0;
    const size_t n_acc = push ? (size_t)(A + 1) * L * (size_t)d.V : 0, n_carry = push ? (size_t)(A + 1) * P : 0;
    const size_t n_act = req.action ? (size_t)P : 0;
    const size_t n_slides = req.slide ? (size_t)P : 0, n_steps = n_slides;      // (the kernel counts the steps in any case; copied on request)
    const size_t n_dbl = (size_t)P * 3 * 2 + n_wat + n_carry + n_acc + n_act, n_u64 = push ? n_acc + 1 : 0,
                 n_int = (size_t)P * 5 + (size_t)F * 3 + n_tat + n_slides + n_steps;
    char *buf = nullptr;
    DevicePool tmp(c->device);      // (every path out of the call below waits for the stream first)
    if (tmp.alloc(&buf, (int64_t)(sizeof(double) * (n_dbl + n_u64) + sizeof(int) * n_int), c->stream, false)) {
        (void)hipGetLastError();
        set_error(w + (push ? "out of device memory for the particle tables and the accumulators" : "out of device memory for the particle tables"));
        return DOTS_ERR_MEMORY;
    }
    double *b_sw = (double *)buf, *b_ow = b_sw + (size_t)P * 3, *b_wat = b_ow + (size_t)P * 3, *b_mass = b_wat + n_wat, *b_attr = b_mass + (push ? P : 0),
           *b_pushed = b_mass + n_carry, *b_act = b_pushed + n_acc;
    unsigned long long *b_acc = (unsigned long long *)(b_act + n_act);
    int *b_start = (int *)(b_acc + n_u64), *b_nbr = b_start + P, *b_otri = b_nbr + (size_t)F * 3, *b_status = b_otri + P, *b_rested = b_status + P,
        *b_cross = b_rested + P, *b_slides = b_cross + P, *b_steps = b_slides + n_slides, *b_tat = b_steps + n_steps;
    auto enqueue = [&]() -> int {
        DOTS_HIP(hipMemcpyAsync(b_sw, desc->start_weights, sizeof(double) * (size_t)P * 3, hipMemcpyHostToDevice, c->stream));
        DOTS_HIP(hipMemcpyAsync(b_start, h_start.data(), sizeof(int) * (size_t)P, hipMemcpyHostToDevice, c->stream));
        DOTS_HIP(hipMemcpyAsync(b_nbr, h_nbr.data(), sizeof(int) * (size_t)F * 3, hipMemcpyHostToDevice, c->stream));
        if (push) {
            DOTS_HIP(hipMemcpyAsync(b_mass, push->mass, sizeof(double) * (size_t)P, hipMemcpyHostToDevice, c->stream));
            if (A) DOTS_HIP(hipMemcpyAsync(b_attr, push->attributes, sizeof(double) * (size_t)A * P, hipMemcpyHostToDevice, c->stream));
        }
        FlowArgs a{};
        a.mu = d.mu; a.E = d.E; a.tri = d.tri; a.hat = d.hat; a.nbr = b_nbr; a.perm_f = d.perm_f;
        a.start_tri = b_start; a.start_w = b_sw;
        a.o_tri = b_otri; a.o_status = b_status; a.o_rested = b_rested; a.o_cross = b_cross; a.o_w = b_ow;
        a.tri_at = desc->triangles_at ? b_tat : nullptr;
        a.w_at = desc->weights_at ? b_wat : nullptr;
        a.floor = desc->floor;
        a.h = 1.0 / (double)T;
        a.P = P; a.T = n_turns; a.tp_shift = d.tp_shift; a.max_crossings = desc->max_crossings;
        const bool forward = node_to > node_from;      // forward: the intervals node_from + i; backward: node_from - 1 - i
        const FlowSpan sp{n_act ? b_act : nullptr, forward ? node_from : node_from - 1, forward ? 1 : -1};
        const FlowSlide sl{d.area_f, b_status};
        DOTS_HIP(hipEventRecord(c->ev[0], c->stream));
        if (push) {      // (the milliseconds hold the zeroing, the trace with its deposits and the conversion)
            q.acc = b_acc; q.mass = b_mass; q.attr = b_attr;
            q.A = A; q.L = (int)L; q.V = d.V;
            DOTS_HIP(hipMemsetAsync(b_acc, 0, sizeof(unsigned long long) * n_u64, c->stream));
            fin.acc = b_acc; fin.inv = c->inv_perm_v; fin.out = b_pushed; fin.A = A; fin.L = (int)L; fin.V = d.V;
        }
        int r = launch_flow(c, a, sp, push ? &q : nullptr, req.slide ? &sl : nullptr);
        if (!r && push) r = launch_flow_push_finish(c, fin);
        if (r) return r;
        DOTS_HIP(hipEventRecord(c->ev[1], c->stream));
        // only the outputs cross to the host
        if (desc->weights) DOTS_HIP(hipMemcpyAsync(desc->weights, b_ow, sizeof(double) * (size_t)P * 3, hipMemcpyDeviceToHost, c->stream));
        int32_t *outs[4] = {desc->triangle, desc->status, desc->rested, desc->crossings};
        const int *srcs[4] = {b_otri, b_status, b_rested, b_cross};
        for (int i = 0; i < 4; ++i)
            if (outs[i]) DOTS_HIP(hipMemcpyAsync(outs[i], srcs[i], sizeof(int) * (size_t)P, hipMemcpyDeviceToHost, c->stream));
        if (desc->weights_at) DOTS_HIP(hipMemcpyAsync(desc->weights_at, b_wat, sizeof(double) * n_wat, hipMemcpyDeviceToHost, c->stream));
        if (desc->triangles_at) DOTS_HIP(hipMemcpyAsync(desc->triangles_at, b_tat, sizeof(int) * n_tat, hipMemcpyDeviceToHost, c->stream));
        if (n_act) DOTS_HIP(hipMemcpyAsync(req.action, b_act, sizeof(double) * n_act, hipMemcpyDeviceToHost, c->stream));
        if (n_slides) DOTS_HIP(hipMemcpyAsync(req.slides, b_slides, sizeof(int) * n_slides, hipMemcpyDeviceToHost, c->stream));
        if (req.slide && req.steps) DOTS_HIP(hipMemcpyAsync(req.steps, b_steps, sizeof(int) * n_steps, hipMemcpyDeviceToHost, c->stream));
        if (push) {
            const size_t n_layer = L * (size_t)d.V;
            DOTS_HIP(hipMemcpyAsync(push->mass_at, b_pushed, sizeof(double) * n_layer, hipMemcpyDeviceToHost, c->stream));
            if (A) DOTS_HIP(hipMemcpyAsync(push->attr_at, b_pushed + n_layer, sizeof(double) * n_layer * A, hipMemcpyDeviceToHost, c->stream));
            if (push->dropped) DOTS_HIP(hipMemcpyAsync(push->dropped, b_acc + n_acc, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        }
        return 0;
    };
    rc = enqueue();      // (every path out of the call waits for the stream first: the copies use the caller's and this call's arrays)
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (!rc && es != hipSuccess) rc = hip_fail(es, "hipStreamSynchronize", __FILE__, __LINE__);
    if (!rc && (desc->ms || (push && push->ms))) {
        float t = 0.f;
        const hipError_t et = hipEventElapsedTime(&t, c->ev[0], c->ev[1]);
        if (et != hipSuccess) rc = hip_fail(et, "hipEventElapsedTime", __FILE__, __LINE__);
        if (desc->ms) *desc->ms = t;
        if (push && push->ms) *push->ms = t;
    }
    if (rc) return rc;
    size_t bytes = sizeof(double) * (n_wat + n_act) + sizeof(int) * (n_tat + n_slides + (req.slide && req.steps ? n_steps : 0)) + (desc->weights ? sizeof(double) * (size_t)P * 3 : 0);
    for (const int32_t *o : {desc->triangle, desc->status, desc->rested, desc->crossings}) bytes += o ? sizeof(int) * (size_t)P : 0;
    if (push) bytes += sizeof(double) * n_acc + (push->dropped ? sizeof(int64_t) : 0);
    c->d2h_bytes += (int64_t)bytes;
    return 0;
}

int dots_flow_map(dots_ctx *c, const dots_flow_map_desc *desc) {
    if (!c) { set_error("null context"); return DOTS_ERR_ARGUMENT; }
    if (!desc) { set_error("flow_map: null description"); return DOTS_ERR_ARGUMENT; }
    return flow_run(c, FlowRequest{E_FLOW_MAP, desc});
}

int dots_flow_push(dots_ctx *c, const dots_flow_push_desc *desc) {
    if (!c) { set_error("null context"); return DOTS_ERR_ARGUMENT; }
    if (!desc) { set_error("flow_push: null description"); return DOTS_ERR_ARGUMENT; }
    return flow_run(c, FlowRequest{E_FLOW_PUSH, &desc->map, desc});
}

int dots_flow_trace(dots_ctx *c, const dots_flow_trace_desc *desc) {
    if (!c) { set_error("null context"); return DOTS_ERR_ARGUMENT; }
    if (!desc) { set_error("flow_trace: null description"); return DOTS_ERR_ARGUMENT; }
    dots_flow_push_desc deposits;
    return flow_run(c, flow_trace_request(E_FLOW_TRACE, *desc, deposits));
}

int dots_flow_slide(dots_ctx *c, const dots_flow_slide_desc *desc) {
    if (!c) { set_error("null context"); return DOTS_ERR_ARGUMENT; }
    if (!desc) { set_error("flow_slide: null description"); return DOTS_ERR_ARGUMENT; }
    dots_flow_push_desc deposits;
    FlowRequest req = flow_trace_request(E_FLOW_SLIDE, desc->trace, deposits);
    req.slide = true; req.slides = desc->slides; req.steps = desc->steps;
    return flow_run(c, req);
}

// ---- dots_sensitivity -----------------------------------------------------------------------------------------------------
int dots_sensitivity(dots_ctx *c, const dots_sensitivity_desc *desc) {
    if (!c) { set_error("null context"); return DOTS_ERR_ARGUMENT; }
    if (!desc) { set_error("sensitivity: null description"); return DOTS_ERR_ARGUMENT; }
    if (c->shard_stride != 0) { set_error("sensitivity: not available on time slabs"); return DOTS_ERR_STATE; }
    if (!desc->phi0 && !desc->phiT && !desc->stress) { set_error("sensitivity: nothing requested (phi0, phiT and stress are all NULL)"); return DOTS_ERR_ARGUMENT; }
    if (!std::isfinite(desc->factor_phi) || !std::isfinite(desc->factor_mu)) { set_error("sensitivity: a factor that is not finite"); return DOTS_ERR_ARGUMENT; }
    const bool on_device = desc->device_pointers != 0;
    if (on_device && ((uintptr_t)desc->stress & 15)) { set_error("sensitivity: the device stress pointer is not on a 16-byte boundary"); return DOTS_ERR_ARGUMENT; }
    const Dev &d = c->d;
    int rc = admit(c, E_SENSITIVITY);      // (a pending penalty division is carried out, as for a download; z_mid is not needed)
    if (rc) return rc;
    if ((rc = readout_prepare(c))) return rc;      // (the inverses of the device numbering are the read-out's)
    // the staging buffer: [stress | phi0 | phiT | mass], every part on a 16-byte boundary
    auto even = [](int64_t n) { return (n + 1) & ~(int64_t)1; };
    const int64_t V = d.V, F = d.F;
    const int64_t n_s = desc->stress && !on_device ? 18 * F : 0, n_p = on_device ? 0 : even(V);
    const int64_t o_p0 = n_s, o_pT = o_p0 + n_p, o_mass = o_pT + n_p, total = o_mass + (desc->mass_vertex ? V : 0);
    if (total > c->stage_count) { set_error("sensitivity: the outputs do not fit the staging buffer on this mesh"); return DOTS_ERR_STATE; }
    double *st = c->stage;
    auto enqueue = [&]() -> int {
        SensArgs a{};
        a.phi = d.phi; a.mu = d.mu; a.tri = d.tri;
        a.inv_v = c->inv_perm_v; a.inv_f = c->inv_perm_f; a.perm_v = d.perm_v;
        a.mass_dev = d.mass_v;
        if (desc->mass_vertex && desc->stress) {
            DOTS_HIP(hipMemcpyAsync(st + o_mass, desc->mass_vertex, sizeof(double) * (size_t)V, hipMemcpyHostToDevice, c->stream));
            a.mass = st + o_mass;
        }
        a.phi0 = !desc->phi0 ? nullptr : (on_device ? desc->phi0 : st + o_p0);
        a.phiT = !desc->phiT ? nullptr : (on_device ? desc->phiT : st + o_pT);
        a.stress = !desc->stress ? nullptr : (on_device ? desc->stress : st);
        a.factor_phi = desc->factor_phi; a.factor_mu = desc->factor_mu;
        a.V = d.V; a.F = d.F; a.T = d.T; a.tp_shift = d.tp_shift;
        DOTS_HIP(hipEventRecord(c->ev[0], c->stream));
        int r = launch_sensitivity(c, a);
        if (r) return r;
        DOTS_HIP(hipEventRecord(c->ev[1], c->stream));
        if (!on_device) {      // only the outputs cross to the host
            if (desc->phi0) DOTS_HIP(hipMemcpyAsync(desc->phi0, st + o_p0, sizeof(double) * (size_t)V, hipMemcpyDeviceToHost, c->stream));
            if (desc->phiT) DOTS_HIP(hipMemcpyAsync(desc->phiT, st + o_pT, sizeof(double) * (size_t)V, hipMemcpyDeviceToHost, c->stream));
            if (desc->stress) DOTS_HIP(hipMemcpyAsync(desc->stress, st, sizeof(double) * (size_t)(18 * F), hipMemcpyDeviceToHost, c->stream));
        }
        return 0;
    };
    rc = enqueue();      // (every path out of the call waits for the stream first: the copies use the caller's arrays)
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (!rc && es != hipSuccess) rc = hip_fail(es, "hipStreamSynchronize", __FILE__, __LINE__);
    if (rc) return rc;
    if (desc->ms) {
        float t = 0.f;
        DOTS_HIP(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
        *desc->ms = t;
    }
    if (!on_device) c->d2h_bytes += (int64_t)sizeof(double) * ((desc->phi0 ? V : 0) + (desc->phiT ? V : 0) + (desc->stress ? 18 * F : 0));
    return 0;
}

// ---- dots_barycenter_update: takes no context (include/dots_socp_hip.h) ----------------------------------------------------------
static int64_t bary_scratch(int64_t V, int64_t *o_mean, int64_t *o_part, int64_t *o_out) {
    const int G = barycenter_workgroups((int)V);
    *o_mean = (V + 1) & ~(int64_t)1;
    *o_part = *o_mean + BARY_MAX_N;
    *o_out = *o_part + 6 * (int64_t)G;
    return *o_out + 4;
}

int64_t dots_barycenter_scratch(int32_t n_vertices) {
    int64_t a, b, c;
    return n_vertices < 1 ? -1 : bary_scratch(n_vertices, &a, &b, &c);
}

int dots_barycenter_update(const dots_barycenter_desc *desc) {
    if (!desc || !desc->phi0 || !desc->weights || !desc->nu || !desc->scalars || !desc->scratch) { set_error("barycenter_update: null argument"); return DOTS_ERR_ARGUMENT; }
    if (desc->n < 1 || desc->n > BARY_MAX_N) { set_error("barycenter_update: n must be 1 .. 16"); return DOTS_ERR_ARGUMENT; }
    if (desc->n_vertices < 1) { set_error("barycenter_update: n_vertices must be positive"); return DOTS_ERR_ARGUMENT; }
    for (int k = 0; k < desc->n; ++k) {
        if (!desc->phi0[k]) { set_error("barycenter_update: a null potential"); return DOTS_ERR_ARGUMENT; }
        if (!std::isfinite(desc->weights[k])) { set_error("barycenter_update: a weight that is not finite"); return DOTS_ERR_ARGUMENT; }
    }
    if (!std::isfinite(desc->eta) || !std::isfinite(desc->mass)) { set_error("barycenter_update: eta and mass must be finite"); return DOTS_ERR_ARGUMENT; }
    const int64_t V = desc->n_vertices;
    if (desc->vertex_row && !desc->nu_device_order) { set_error("barycenter_update: vertex_row without nu_device_order"); return DOTS_ERR_ARGUMENT; }
    int64_t o_mean, o_part, o_out;
    const int64_t total = bary_scratch(V, &o_mean, &o_part, &o_out);
    auto overlap = [](const double *a, int64_t na, const double *b, int64_t nb) { return a < b + nb && b < a + na; };
    if ((desc->nu_device_order && overlap(desc->nu_device_order, V, desc->nu, V)) || overlap(desc->scratch, total, desc->nu, V)
        || (desc->nu_device_order && overlap(desc->scratch, total, desc->nu_device_order, V))) {
        set_error("barycenter_update: nu, nu_device_order and scratch overlap");
        return DOTS_ERR_ARGUMENT;
    }
    DOTS_HIP(hipSetDevice(desc->device));
    hipStream_t stream = static_cast<hipStream_t>(desc->stream);
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto enqueue = [&]() -> int {
        BaryArgs a{};
        for (int k = 0; k < desc->n; ++k) {
            a.phi[k] = desc->phi0[k];
            a.w[k] = desc->weights[k];
        }
        a.eta = desc->eta; a.mass = desc->mass;
        a.nu = desc->nu; a.nu_dev = desc->nu_device_order; a.inv_v = desc->vertex_row;
        a.y = desc->scratch; a.mean = desc->scratch + o_mean; a.part = desc->scratch + o_part; a.out = desc->scratch + o_out;
        a.n = desc->n; a.V = (int)V; a.G = barycenter_workgroups((int)V);
        if (desc->ms) {
            DOTS_HIP(hipEventCreate(&ev[0]));
            DOTS_HIP(hipEventCreate(&ev[1]));
            DOTS_HIP(hipEventRecord(ev[0], stream));
        }
        int r = launch_barycenter(stream, a);
        if (r) return r;
        if (desc->ms) DOTS_HIP(hipEventRecord(ev[1], stream));
        // (pageable host memory: the copy is complete when the stream is idle, which the call waits for below)
        DOTS_HIP(hipMemcpyAsync(desc->scalars, a.out, 4 * sizeof(double), hipMemcpyDeviceToHost, stream));
        return 0;
    };
    int rc = enqueue();      // (every path out of the call waits for the stream first: the kernels use the caller's arrays)
    const hipError_t es = hipStreamSynchronize(stream);
    if (!rc && es != hipSuccess) rc = hip_fail(es, "hipStreamSynchronize", __FILE__, __LINE__);
    if (!rc && desc->ms) {
        float t = 0.f;
        const hipError_t et = hipEventElapsedTime(&t, ev[0], ev[1]);
        if (et != hipSuccess) rc = hip_fail(et, "hipEventElapsedTime", __FILE__, __LINE__);
        *desc->ms = t;
    }
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

// ---- dots_tangent_*: linearised transport; the calls take no context (include/dots_socp_hip.h) ------------------------------------------
static bool tangent_overlap(const void *a, int64_t bytes_a, const void *b, int64_t bytes_b) {
    const char *p = static_cast<const char *>(a), *q = static_cast<const char *>(b);
    return p < q + bytes_b && q < p + bytes_a;
}

// The launches of `enqueue` on the descriptor's device and stream, timed if asked for; `after` (may be empty) enqueues what follows
// the timed part.  Every path out waits for the stream first: the kernels use the caller's arrays.
using TangentWork = std::function<int(hipStream_t)>;
static int tangent_run(const dots_tangent_desc *desc, const TangentWork &enqueue, const TangentWork &after) {
    DOTS_HIP(hipSetDevice(desc->device));
    hipStream_t stream = static_cast<hipStream_t>(desc->stream);
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto all = [&]() -> int {
        if (desc->ms) {
            DOTS_HIP(hipEventCreate(&ev[0]));
            DOTS_HIP(hipEventCreate(&ev[1]));
            DOTS_HIP(hipEventRecord(ev[0], stream));
        }
        int r = enqueue(stream);
        if (r) return r;
        if (desc->ms) DOTS_HIP(hipEventRecord(ev[1], stream));
        return after(stream);
    };
    int rc = all();
    const hipError_t es = hipStreamSynchronize(stream);
    if (!rc && es != hipSuccess) rc = hip_fail(es, "hipStreamSynchronize", __FILE__, __LINE__);
    if (!rc && desc->ms) {
        float t = 0.f;
        const hipError_t et = hipEventElapsedTime(&t, ev[0], ev[1]);
        if (et != hipSuccess) rc = hip_fail(et, "hipEventElapsedTime", __FILE__, __LINE__);
        *desc->ms = t;
    }
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

static bool tangent_sizes_ok(const dots_tangent_desc *desc, const char *who) {
    if (!desc) { set_error(std::string(who) + ": null argument"); return false; }
    if (desc->n_vertices < 1 || desc->n_triangles < 1) { set_error(std::string(who) + ": n_vertices and n_triangles must be positive"); return false; }
    return true;
}

int dots_tangent_velocities(const dots_tangent_desc *desc, int32_t n, const double *const *phi0, double *velocities) {
    const char *who = "tangent_velocities";
    if (!tangent_sizes_ok(desc, who)) return DOTS_ERR_ARGUMENT;
    if (!desc->triangles || !desc->hat_grad || !phi0 || !velocities) { set_error("tangent_velocities: null argument"); return DOTS_ERR_ARGUMENT; }
    if (n < 1) { set_error("tangent_velocities: n must be at least 1"); return DOTS_ERR_ARGUMENT; }
    const int64_t V = desc->n_vertices, F = desc->n_triangles, out_bytes = (int64_t)n * F * 24;
    if (tangent_overlap(velocities, out_bytes, desc->triangles, F * 12) || tangent_overlap(velocities, out_bytes, desc->hat_grad, F * 72)) {
        set_error("tangent_velocities: velocities overlaps the mesh tables");
        return DOTS_ERR_ARGUMENT;
    }
    for (int k = 0; k < n; ++k) {
        if (!phi0[k]) { set_error("tangent_velocities: a null potential"); return DOTS_ERR_ARGUMENT; }
        if (tangent_overlap(velocities, out_bytes, phi0[k], V * 8)) { set_error("tangent_velocities: velocities overlaps a potential"); return DOTS_ERR_ARGUMENT; }
    }
    return tangent_run(desc, [&](hipStream_t stream) -> int {
        for (int at = 0; at < n; at += TANGENT_VEL_N) {
            TangentVelArgs a{};
            a.n = std::min(n - at, TANGENT_VEL_N);
            for (int k = 0; k < a.n; ++k) a.phi[k] = phi0[at + k];
            a.tri = desc->triangles; a.hat = desc->hat_grad; a.F = (int)F;
            a.out = velocities + (int64_t)at * F * 3;
            int r = launch_tangent_velocities(stream, a);
            if (r) return r;
        }
        return 0;
    }, [](hipStream_t) -> int { return 0; });
}

int dots_tangent_weights(const dots_tangent_desc *desc, const double *sigma, double *w) {
    const char *who = "tangent_weights";
    if (!tangent_sizes_ok(desc, who)) return DOTS_ERR_ARGUMENT;
    if (!desc->triangles || !desc->area_tri || !desc->mass_vert || !sigma || !w) { set_error("tangent_weights: null argument"); return DOTS_ERR_ARGUMENT; }
    const int64_t V = desc->n_vertices, F = desc->n_triangles;
    if (tangent_overlap(w, F * 8, sigma, V * 8) || tangent_overlap(w, F * 8, desc->triangles, F * 12) || tangent_overlap(w, F * 8, desc->area_tri, F * 8)
        || tangent_overlap(w, F * 8, desc->mass_vert, V * 8)) {
        set_error("tangent_weights: w overlaps an input");
        return DOTS_ERR_ARGUMENT;
    }
    return tangent_run(desc, [&](hipStream_t stream) -> int {
        return launch_tangent_weights(stream, desc->triangles, sigma, desc->mass_vert, desc->area_tri, w, (int)F);
    }, [](hipStream_t) -> int { return 0; });
}

int64_t dots_tangent_gram_scratch(int32_t na, int32_t nb, int32_t n_triangles) {
    if (na < 1 || nb < 1 || na > TANGENT_MAX_N || nb > TANGENT_MAX_N || n_triangles < 1) return -1;
    return (2 * (int64_t)tangent_chunks(n_triangles) + 1) * na * nb;      // the partial pairs, then G
}

int dots_tangent_gram(const dots_tangent_desc *desc, int32_t na, const double *A, int32_t nb, const double *B, const double *w, double *scratch, double *G) {
    const char *who = "tangent_gram";
    if (!tangent_sizes_ok(desc, who)) return DOTS_ERR_ARGUMENT;
    if (!A || !w || !scratch || !G) { set_error("tangent_gram: null argument"); return DOTS_ERR_ARGUMENT; }
    const int64_t F = desc->n_triangles, total = dots_tangent_gram_scratch(na, nb, (int32_t)F);
    if (total < 0) { set_error("tangent_gram: na and nb must be 1 .. 4096"); return DOTS_ERR_ARGUMENT; }
    if (!B && nb != na) { set_error("tangent_gram: B = NULL means B = A: nb must equal na"); return DOTS_ERR_ARGUMENT; }
    if (tangent_overlap(scratch, total * 8, A, (int64_t)na * F * 24) || (B && tangent_overlap(scratch, total * 8, B, (int64_t)nb * F * 24))
        || tangent_overlap(scratch, total * 8, w, F * 8)) {
        set_error("tangent_gram: scratch overlaps an input");
        return DOTS_ERR_ARGUMENT;
    }
    TangentGramArgs a{};
    a.A = A; a.B = B ? B : A; a.w = w;
    a.na = na; a.nb = nb; a.F = (int)F; a.C = tangent_chunks((int)F);
    a.part = scratch; a.G = scratch + 2 * (int64_t)a.C * na * nb;
    return tangent_run(desc, [&](hipStream_t stream) -> int { return launch_tangent_gram(stream, a); }, [&](hipStream_t stream) -> int {
        // (pageable host memory: the copy is complete when the stream is idle, which the call waits for)
        DOTS_HIP(hipMemcpyAsync(G, a.G, sizeof(double) * (size_t)na * nb, hipMemcpyDeviceToHost, stream));
        return 0;
    });
}

int dots_front_enable(dots_ctx *c, int on) {
    int rc = admit(c, E_FRONT_ENABLE);
    if (rc) return rc;
    if (on && c->front.n_nodes == 0) { set_error("front_enable: no factor installed"); return DOTS_ERR_STATE; }
    c->use_front = on ? 1 : 0;
    return 0;
}

int dots_pcg_windows(dots_ctx *c, int on) {
    int rc = admit(c, E_PCG_WINDOWS);
    if (rc) return rc;
    if (c->lap_solver != DOTS_LAP_MODAL_PCG) { set_error("pcg_windows: the windows belong to the modal solver (DOTS_LAP_MODAL_PCG)"); return DOTS_ERR_STATE; }
    if (c->shard_stride != 0) { set_error("pcg_windows: not on a time slab"); return DOTS_ERR_STATE; }
    on = on ? 1 : 0;
    if (on == c->pcg_windows) return 0;
    // a hierarchy installed under the other setting has the other layout (level vectors and coarse inverse per window): it goes, with the graphs
    if (c->d.cg_ncol > CgScalOffsets::NCMAX) {
        DOTS_HIP(hipStreamSynchronize(c->stream));
        c->cg_graphs_release();
        mg_release(c);
    }
    c->pcg_windows = on;
    c->pcg_windows_ran = 0;
    return 0;
}

int dots_front_launches(dots_ctx *c) {
    if (admit(c, E_FRONT_LAUNCHES) || c->front.n_nodes == 0) return -1;
    return 2 * c->sched.n_bands - (c->sched.top_inverse ? 1 : 0);
}

int dots_front_info(dots_ctx *c, double *out) {
    int rc = admit(c, E_FRONT_INFO);
    if (rc) return rc;
    if (!out || c->front.n_nodes == 0) { set_error("front_info: no factor installed"); return DOTS_ERR_STATE; }
    out[0] = c->sched.bytes_unmerged;
    out[1] = c->sched.bytes;
    out[2] = (double)c->sched.heights;
    out[3] = (double)c->sched.n_bands;
    return 0;
}

int dots_front_pitch(dots_ctx *c) {
    if (admit(c, E_FRONT_PITCH)) return -1;
    return c->d.TP;      // (the PCG view's pitch is d's)
}

int64_t dots_debug_counter(dots_ctx *c, int which) {
    if (!c) return -1;
    switch (which) {
        case 0: return c->mail_fallbacks;
        case 1: return (int64_t)c->mail_seq;
        case 2: return c->penalty_ahead_started;
        case 3: return c->penalty_ahead_confirmed;
        case 4: return c->front.n_leaves;      // leaves the sweeps handle as explicit local inverses (0: band kernels)
        case 5: return c->front.leaf_bd ? 1 : 0;      // ... with their coupling in per-row records (0: read from the CSR)
        case 6: return c->sched.bm_nt;                      // beta_mid streamed around the caches by steps 2+3 (the rule of dots_front_setup, or DOTS_BM_NT)
        case 7: return c->front_many_launches;        // sweep launches the last front_solve_many on this (first) context enqueued
        case 8: return c->front_many_split;           // ... of those, launches with fewer rhs than their chunk (many_launch halved: LDS or 1024-thread cap)
        case 9: return c->d2h_bytes;                  // bytes dots_download, dots_readout, dots_flow_map, dots_flow_push, dots_flow_trace, dots_flow_slide and dots_sensitivity have copied device -> host
        case 10: return c->front_own.size() + (c->front_store ? c->front_store->size() : 0);      // device allocations of the factor this context holds, its own and the store it shares (0 after front_release: also after a failed dots_front_setup)
        case 11: return c->mg_path;                   // MG_PATH_* bits of the last V-cycle enqueued (dots_dev.h)
        case 12: return c->carried.step_path;                 // STEP_PATH_* bits of the last iteration's launches (dots_dev.h)
        case 13: return c->cg_path;                   // CG_PATH_* bits and tiling of the last PCG launches (dots_dev.h)
        case 14: return c->pcg_windows_ran;           // low byte: windows the last PCG solve ran (0: none yet, or unwindowed); bit 8: the windowed transforms ran
        case 15: return c->carried.deep_path;                 // DEEP_PATH_* of the last right-hand side and inverse transform (dots_dev.h)
        default: return -1;
    }
}

int dots_bench_kernel(dots_ctx *c, int which, int reps, double *ms, double *bytes) {
    int rc = admit(c, E_BENCH_KERNEL);
    if (rc) return rc;
    if (reps < 1 || !ms || !bytes) { set_error("bench: bad argument"); return DOTS_ERR_ARGUMENT; }
    if (which == 5) {      // dots_restart's in-place rescaling with every factor 1: the state keeps its values
        if (c->shard_stride != 0) { set_error("bench: the rescaling of dots_restart does not run on a time slab"); return DOTS_ERR_STATE; }
        if ((rc = need_zmid(c, E_BENCH_KERNEL))) return rc;
        const double one[4] = {1.0, 1.0, 1.0, 1.0};
        for (int i = 0; i < 2; ++i) if ((rc = launch_restart_scale(c, one, bytes))) return rc;
        DOTS_HIP(hipEventRecord(c->ev[6], c->stream));
        for (int i = 0; i < reps; ++i) if ((rc = launch_restart_scale(c, one, bytes))) return rc;
        DOTS_HIP(hipEventRecord(c->ev[7], c->stream));
        DOTS_HIP(hipEventSynchronize(c->ev[7]));
        float t = 0.f;
        DOTS_HIP(hipEventElapsedTime(&t, c->ev[6], c->ev[7]));
        *ms = (double)t / reps;
        return 0;
    }
    return cg_bench(c, which, reps, ms, bytes);
}

}  // extern "C"

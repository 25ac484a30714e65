// ALM element-wise / gather kernels for gfx950: second-order-cone projection, right-hand side
// of the phi step, the fused (q, lambda_c) + multiplier update, scaling tools, layout conversion.
// All HBM-bound fp64; one thread per (row, time) element, rows = vertices or (triangle, xyz).
#include "modes_dev.h"
#include "kkt_slots.h"

#include <algorithm>
#include <cassert>

namespace dots {

// ------------------------------------------------------------------------------------------
// Step 1-2  second-order-cone projection      (reference: solver_socp.py:988-1042)
//
// Cone of (t, v):  z_fst >= || ( z_end, D[k,f] * z_mid[t, s, k, f, c]  over the corners (f,k) of v ) ||.
// The reference does this with two 0/1 incidence SpMVs and >= 9 passes over 18*T*F-sized arrays;
// here one thread owns (v, t): it walks the vertex's corner list once to accumulate the squared
// norm, forms lambda, and walks it again to write z_mid of its own corners (no atomics: every
// corner belongs to exactly one vertex).  beta_mid is read from HBM once, the second walk hits L2.
// ------------------------------------------------------------------------------------------
// ONLY_MULTIPLIER: the iteration driver (dots_step) does not need z_mid in memory: it stores the cone
// multiplier lambda[v][t] (T*V values instead of 18*T*F) and steps 2+3 rebuild z_mid = lambda/D * pre-image on
// the fly from beta_mid and B, which they read anyway: the second corner walk and 18*T*F stores disappear here,
// 18*T*F loads disappear there.
// The squared norm is accumulated in two halves, s = 0 (entries of node t) and s = 1 (entries of node t + 1), each over
// the corner list in order: when node t + 1 belongs to the next time slab that rank forms the s = 1 half from its own
// B and beta_mid (soc_half_of_first_node) and this one reads it from the halo -- bit for bit the same sum.
// two consecutive time columns of a row (16-byte aligned: even column, pitch a power of two)

// A corner's share of a sum over xyz is formed FIRST, as (x + y) + z, and the shares are then added in corner-list order: the
// kernels that gather these terms from memory and the steps-2+3 kernel that forms them from its registers for the next
// iteration (DOTS_STEP_CARRY: cn_sq, cn_g below) then produce the same sums bit for bit (-ffp-contract=off: no fused multiply-adds).
__device__ __forceinline__ double sum3(double x, double y, double z) { return (x + y) + z; }
constexpr int CARRY_BATCH = 2;      // corners whose carried rows a lane loads before it adds them (closed surfaces: valence ~ 6)
// one pre-image entry of the cone's middle block squared: (D (sB B - beta_mid))^2, sBB = sB * B already rounded
__device__ __forceinline__ double soc_w2(double D, double sBB, double bm) {
    const double w = D * (sBB - bm);
    return w * w;
}
// z_mid from the cone multiplier: z = (lambda / D) * (D * (sz/sqrt3 * B - beta_mid)), sBB = sz/sqrt3 * B already rounded.  The one place where it is
// written: the full projection stores it, steps 2+3 (ql_lane, ZMODE >= 1) and k_rebuild_zmid rebuild it from the stored multiplier.
__device__ __forceinline__ double zmid_of(double lam, double D, double sBB, double bm) { return (lam / D) * (D * (sBB - bm)); }

__device__ __forceinline__ double soc_half(const Dev &d, int v, int t, int s, double sB) {
    double acc = 0.0;
    for (int j = d.cptr[v]; j < d.cptr[v + 1]; ++j) {
        const int fk = d.cidx[j];
        const int f = fk / 3;
        const double D = d.c_D[j];
        double q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = soc_w2(D, sB * d.B[idxF(d, f, c, t + s)], d.bm[idxM(d, fk, s, c, t)]);
        acc += sum3(q[0], q[1], q[2]);
    }
    return acc;
}

// CARRIED: the corners' shares were stored by the last steps-2+3 launch in corner-LIST order (a vertex's rows are contiguous), ROWS rows per
// corner, the column that of the lane's interval or node: no index chain, neither B, E nor beta_mid is touched.  The rows of the corners
// j0 .. j1 - 1 at the N columns p points to, added in list order into acc[row][column]: BATCH corners' loads in flight, rows clamped to the list.
// What lies past the list is dropped by a select, not a branch: behind a branch the compiler moved the later corners' loads too (k_rhs_modes2<true>: the
// projection's four loads of a pass went out two and two, torus100k 691 -> 676 it/s).
template <int N, int BATCH, int ROWS>
__device__ __forceinline__ void carried_gather(const Dev &d, const double *__restrict__ p, int j0, int j1, double (&acc)[ROWS][N]) {
    for (int j = j0; j < j1; j += BATCH) {
        DN<N> q[BATCH][ROWS];
#pragma unroll
        for (int i = 0; i < BATCH; ++i) {
            const int64_t row = (int64_t)(ROWS * min(j + i, j1 - 1)) << d.tp_shift;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) q[i][r] = ldn_nt<N>(p + row + r * d.TP);
        }
#pragma unroll
        for (int i = 0; i < BATCH; ++i) {
            const bool in = j + i < j1;
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
#pragma unroll
                for (int u = 0; u < N; ++u) {
                    const double sum = acc[r][u] + q[i][r].v[u];
                    acc[r][u] = in ? sum : acc[r][u];
                }
        }
    }
}

// The multiplier of the cone from the two halves of the middle block's squared norm and the values of A, beta_fst, beta_end at the lane's N
// intervals; z_fst, z_end (and with ONLY_MULTIPLIER the multiplier) are stored -- as 16-byte words when both intervals of a pair exist.
template <int N, bool ONLY_MULTIPLIER>
__device__ __forceinline__ DN<N> soc_finish(const Dev &d, int iv, int t, double sz, double cd, const double (&acc)[2][N], const DN<N> &A, const DN<N> &bf, const DN<N> &be) {
    DN<N> zf, ze, lm;
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const double a = A.v[u];
        const double w_fst = cd - sz * a - bf.v[u];
        const double w_end = cd + sz * a - be.v[u];
        const double nrm = sqrt((acc[0][u] + acc[1][u]) + w_end * w_end);
        double lam = 0.5 * (1.0 + w_fst / nrm);          // 0/0 -> NaN when the pre-image is 0, as in the reference (:1018)
        if (lam == lam) lam = fmin(fmax(lam, 0.0), 1.0);  // np.clip keeps NaN; fmin/fmax would drop it
        zf.v[u] = (lam >= 1.0) ? w_fst : lam * nrm;
        ze.v[u] = lam * w_end;
        lm.v[u] = lam;
    }
    if (N == 2 && t + 1 < d.ni) {      // the second interval exists (T odd: not for the last pair)
        stn<N>(d.zf + iv, zf);
        stn<N>(d.ze + iv, ze);
        if (ONLY_MULTIPLIER) stn<N>(d.lamc + iv, lm);
    } else {
        d.zf[iv] = zf.v[0];
        d.ze[iv] = ze.v[0];
        if (ONLY_MULTIPLIER) d.lamc[iv] = lm.v[0];
    }
    return lm;
}

// The projection of the N consecutive intervals t .. t + N - 1 of a vertex by one lane.
// N = 1: 8-byte accesses; the only form of the full projection (z_mid stored) and on a time slab (the halo nsq_hi).
// N = 2 (t even, one GPU: every node is held here, multiplier only): B and the s = 0 entries of both intervals sit in one aligned 16-byte
// word per row, 15 loads per corner instead of 24; half the waves for the same bytes (see ql_lane).
// CARRIED: carried_gather over cn_sq[j][s][interval] (the s = 1 shares are stored in the column of their INTERVAL).
// DIV: a penalty update is pending (Carried::pending_div): the five dual arrays still hold their values BEFORE the division by
// `dv` (admm_tools / solver_socp.py:367-371) and every entry is divided as it is read -- the same IEEE division the stand-alone
// kernel (k_divide_five) performs, so nothing changes bit for bit; steps 2+3 of the same iteration write the arrays back divided.
template <int N, bool ONLY_MULTIPLIER, bool CARRIED = false, bool DIV = false>
__device__ __forceinline__ void soc_lane(const Dev &d, int v, int t, double sz, double cd, double dv = 1.0) {
    static_assert(N == 1 || ONLY_MULTIPLIER, "the full projection takes one interval per lane");
    const double sB = sz * INV_SQRT3;
    const int iv = idxV(d, v, t);
    const int j0 = d.cptr[v], j1 = d.cptr[v + 1];
    bool ex[N];      // the end node of interval t + u is held here (N = 1: not at a slab's last interval) and the interval exists (N = 2: T odd)
#pragma unroll
    for (int u = 0; u < N; ++u) ex[u] = N == 1 ? t + 1 < d.nl : (u == 0 || t + 1 < d.ni);
    double acc[2][N] = {};
    if (CARRIED) carried_gather<N, CARRY_BATCH, 2>(d, d.cn_sq + t, j0, j1, acc);
    for (int j = CARRIED ? j1 : j0; j < j1; ++j) {
        const int fk = d.cidx[j];
        const int f = fk / 3;
        const double D = d.c_D[j];
        double b[3][N + 1], m0[3][N], m1[3][N];      // B at the nodes t .. t + N; beta_mid's s = 0 and s = 1 entries of the lane's intervals
        // N = 2: every load of the corner first, what does not exist dropped by a select.  N = 1: B at node t + 1 and the s = 1 entries behind their
        // branch, after the s = 0 half: with a corner's twelve loads in flight k_rhs_modes_mfma<false, true> took 74 VGPRs instead of 72 (6 waves
        // per SIMD instead of 7) and k_soc_projection<true> 58 instead of 50.
        constexpr bool LATE = N == 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const DN<N> bt = ldn<N>(d.B + idxF(d, f, c, t)), mt = ldn<N>(d.bm + idxM(d, fk, 0, c, t));
            if (!LATE) b[c][N] = ex[N - 1] ? d.B[idxF(d, f, c, t + N)] : 0.0;
#pragma unroll
            for (int u = 0; u < N; ++u) {
                b[c][u] = bt.v[u];
                m0[c][u] = mt.v[u];
                if (!LATE) m1[c][u] = ex[u] ? d.bm[idxM(d, fk, 1, c, t + u)] : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < N; ++u) {
            double q[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c] = soc_w2(D, sB * b[c][u], DIV ? m0[c][u] / dv : m0[c][u]);
            acc[0][u] += sum3(q[0], q[1], q[2]);
            if (!ex[u]) continue;
            if (LATE) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { b[c][u + 1] = d.B[idxF(d, f, c, t + u + 1)]; m1[c][u] = d.bm[idxM(d, fk, 1, c, t + u)]; }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c] = soc_w2(D, sB * b[c][u + 1], DIV ? m1[c][u] / dv : m1[c][u]);
            acc[1][u] += sum3(q[0], q[1], q[2]);
        }
    }
    if constexpr (N == 1) { if (!ex[0]) acc[1][0] = d.nsq_hi[v]; }      // (time slab: node t + 1 belongs to the next slab, which formed this half)
    DN<N> bf = ldn<N>(d.bf + iv), be = ldn<N>(d.be + iv);
    if (DIV) {
#pragma unroll
        for (int u = 0; u < N; ++u) { bf.v[u] /= dv; be.v[u] /= dv; }
    }
    const DN<N> lam = soc_finish<N, ONLY_MULTIPLIER>(d, iv, t, sz, cd, acc, ldn<N>(d.A + iv), bf, be);
    if (ONLY_MULTIPLIER) return;
    for (int j = j0; j < j1; ++j) {      // (not reached on a time slab: the full projection needs every node of the interval here)
        const int fk = d.cidx[j];
        const int f = fk / 3;
        const double D = d.c_D[j];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int c = 0; c < 3; ++c) d.zm[idxM(d, fk, s, c, t)] = zmid_of(lam.v[0], D, sB * d.B[idxF(d, f, c, t + s)], d.bm[idxM(d, fk, s, c, t)]);
    }
}

template <bool ONLY_MULTIPLIER, bool CARRIED = false>
__global__ __launch_bounds__(BLOCK) void k_soc_projection(Dev d, double sz, double cd, int n_soc, int IC) {
    // Workgroups [n_soc, gridDim.x): the modes -> time transform of phi (independent of the projection, same launch)
    if ((int)blockIdx.x >= n_soc) {
        const int tile = xcd_tile(blockIdx.x - n_soc, d.n_vtiles);
        if (tile >= d.n_vtiles) return;
        modes_of_tile<false>(d, IC, tile * d.VT, NodeRows{d.cg_x, d.tp_shift}, d.phi);
        return;
    }
    // one element per thread: a workgroup takes a quarter of a tile (the corner walk is a chain of dependent
    // loads; four elements per thread would serialise four of them)
    // (block b and block b + G8 share a tile and an XCD: G8 is a multiple of 8)
    const int G8 = n_soc / (TILE_ELEMS / BLOCK);
    const int tile = xcd_tile(blockIdx.x % G8, d.n_vtiles);
    if (tile >= d.n_vtiles) return;
    const int v0 = tile * d.VT;
    for (int e = (blockIdx.x / G8) * BLOCK + threadIdx.x; e < TILE_ELEMS; e += TILE_ELEMS) {
        const int v = v0 + (e >> d.tp_shift), t = e & (d.TP - 1);
        if (v >= d.V || t >= d.ni) continue;
        soc_lane<1, ONLY_MULTIPLIER, CARRIED>(d, v, t, sz, cd);
    }
}

// ------------------------------------------------------------------------------------------
// Time slabs: what the neighbouring slabs need from this one (dots_slab_stage 0 and 4).
//   forward  (to the next slab, which starts at node t0 + nl):   X = A + lambda_c - mu (right-hand side at its first node) or
//            mu (KKT) of this slab's last interval nl - 1
//   backward (to the previous slab, which ends with interval t0 - 1): the s = 1 half of that interval's cone norms --
//            its entries are compared with B of THIS slab's first node and live in this slab's column 0 -- or B of the
//            first node (KKT: Comp(rho, f(q)))
// ------------------------------------------------------------------------------------------
template <bool CARRIED>
__global__ __launch_bounds__(BLOCK) void k_slab_pack_iteration(Dev d, double sz, double *__restrict__ send_x, double *__restrict__ send_nsq) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= d.V) return;
    if (d.t0 + d.nl <= d.T) {        // a next slab exists: interval nl - 1 is this slab's last and ends at its first node
        const int iv = idxV(d, v, d.nl - 1);
        send_x[v] = d.A[iv] + d.lam[iv] - d.mu[iv];
    }
    if (d.t0 > 0) {
        if (CARRIED) {               // the corners' shares were left by steps 2+3 (cn_lo: same values, same order of the sum)
            double acc = 0.0;
            for (int j = d.cptr[v]; j < d.cptr[v + 1]; ++j) acc += d.cn_lo[j];
            send_nsq[v] = acc;
        } else {
            send_nsq[v] = soc_half(d, v, -1, 1, sz * INV_SQRT3);
        }
    }
}
__global__ __launch_bounds__(BLOCK) void k_slab_pack_kkt(Dev d, double *__restrict__ send_mu, double *__restrict__ send_b) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < d.V && d.t0 + d.nl <= d.T) send_mu[i] = d.mu[idxV(d, i, d.nl - 1)];
    if (i < 3 * d.F && d.t0 > 0) send_b[i] = d.B[(int64_t)i << d.tp_shift];
}
int launch_slab_pack_iteration(Ctx *c) {
    if (c->d.nl == 0) return 0;
    with_constant<true, false>(c->carried.carry_valid != 0, [&](auto CARRIED) {
        hipLaunchKernelGGL(k_slab_pack_iteration<CARRIED>, dim3((c->d.V + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, c->d, c->prm.scale_z, c->slab.send_x, c->slab.send_nsq);
    });
    DOTS_HIP(hipGetLastError());
    return 0;
}
int launch_slab_pack_kkt(Ctx *c) {
    if (c->d.nl == 0) return 0;
    const int n = std::max(c->d.V, 3 * c->d.F);
    hipLaunchKernelGGL(k_slab_pack_kkt, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, c->d, c->slab.send_mu, c->slab.send_b);
    DOTS_HIP(hipGetLastError());
    return 0;
}

int launch_soc_projection(Ctx *c, int zmid_mode, bool with_inverse) {
    const int n_soc = xcd_grid(c->d.n_vtiles) * (TILE_ELEMS / BLOCK);
    const int n_inv = with_inverse ? xcd_grid(c->d.n_vtiles) : 0;
    const size_t lds = with_inverse ? time_modes_tile_lds(c->d) : 0;
    const int IC = time_modes_chunk(c->d);
    // 0: the full projection (z_mid stored), 1: the multiplier only, 2: the multiplier from the carried shares
    with_constant<0, 1, 2>(!zmid_mode ? 0 : (c->carried.carry_valid ? 2 : 1), [&](auto V) {
        hipLaunchKernelGGL((k_soc_projection<V != 0, V == 2>), dim3(n_soc + n_inv), dim3(BLOCK), lds, c->stream, c->d, c->prm.scale_z, c->prm.const_d, n_soc, IC);
    });
    DOTS_HIP(hipGetLastError());
    c->carried.step_path = (c->carried.step_path & ~STEP_PATH_SOC_RIDER) | STEP_PATH_SOC_ALONE;
    return 0;
}

// ------------------------------------------------------------------------------------------
// Step 1-1 right-hand side                    (reference: solver_socp.py:976-986, :886-921)
//   rhs = div_t((A + lambda_c - mu) * mass) + div_x((B - E) * area) - boundary - eps * mass * phi
// The PCG solves K phi = b with K = -Laplacian (SPD-semidefinite), so b = -rhs is stored.
// div_x is a gather over the vertex's corner list (no scatter, no atomics).  Each workgroup also
// emits the partial sum of b (mean removal for the singular eps = 0 operator).
// ------------------------------------------------------------------------------------------
// div_t((A + lambda_c - mu) mass) at the lane's N nodes: xp = that product of interval t - 1 (0 when there is none); A, L, M = A, lambda_c, mu of
// the lane's intervals, in its columns
template <int N>
__device__ __forceinline__ void rhs_div_time(const Dev &d, int t, double m, double xp, const DN<N> &A, const DN<N> &L, const DN<N> &M, double (&dt)[N]) {
    const double ih = 1.0 / d.h;
    double x[N + 1];
    x[0] = xp;
#pragma unroll
    for (int u = 0; u < N; ++u) {
        x[u + 1] = t + u < d.ni ? (A.v[u] + L.v[u] - M.v[u]) * m : 0.0;
        dt[u] = (x[u + 1] - x[u]) * ih;
    }
}
// The right-hand side at the lane's N nodes t .. t + N - 1 from its parts: dt (rhs_div_time), P = phi in the lane's columns, ds = the nodes'
// div_x((B - E) area), mu0[i] / mu1[i] = the vertex's boundary masses, read behind their branch, by the lanes of node 0 / T only (the deep form has
// them in registers and passes their addresses; handing them over by value put the loads before the branch and ten instructions into k_rhs_modes2).
template <int N>
__device__ __forceinline__ void rhs_finish(const Dev &d, int t, double r, double eps, double m, const double (&dt)[N], const DN<N> &P, const double (&ds)[1][N],
                                           const double *mu0, const double *mu1, int i, double (&out)[N]) {
    const int t0 = N == 1 ? d.t0 : 0;      // (two nodes per lane run on one GPU; t is even then: its second node is never node 0)
#pragma unroll
    for (int u = 0; u < N; ++u) {
        double rhs = dt[u];
        rhs -= ds[0][u];
        if (t0 + t + u == 0) rhs += mu0[i] / (r * d.h);       // first_node
        if (t0 + t + u == d.T) rhs -= mu1[i] / (r * d.h);     // last_node
        rhs -= eps * m * P.v[u];
        out[u] = -rhs;
    }
}

// The right-hand side at the N consecutive nodes t .. t + N - 1 of a vertex by one lane.  N = 1: 8-byte accesses; on a time slab interval t0 - 1
// lives in the previous slab (the halo X_lo).  N = 2 (t even, one GPU): the vertex arrays, B and E of both nodes in one 16-byte word per row.
// CARRIED: the corners' shares of div_x((B - E) area) were stored by the last steps-2+3 launch (cn_g[j][node]).  DIV: see soc_lane.
template <int N, bool CARRIED = false, bool DIV = false>
__device__ __forceinline__ void rhs_lane(const Dev &d, int v, int t, double r, double eps, double (&out)[N], double dv = 1.0) {
    const int iv = idxV(d, v, t);
    const double m = d.mass_v[v];
    DN<N> P;
    double dt[N], ds[1][N] = {};
    if constexpr (N == 1) {
        // One node per lane keeps its own head: the interval's loads behind `t < ni`, interval t first, then t - 1, phi loaded after the walk.  Through
        // the two-node head below (every load first, interval t - 1 first) the one-node kernels held 2 to 6 VGPRs more -- k_rhs<true> 42 against 36,
        // k_rhs<false> 52 / 48, k_rhs_modes 54 / 50, k_rhs_modes_mfma<false, true> 74 / 72 = 6 waves per SIMD against 7 -- and the slab iteration at
        // torus100k ran at 517 it/s against 525-531 (profiles/elementwise_lanes).
        const double ih = 1.0 / d.h;
        double xt = 0.0, xm = 0.0;
        if (t < d.ni) xt = (d.A[iv] + d.lam[iv] - (DIV ? d.mu[iv] / dv : d.mu[iv])) * m;
        if (t > 0) xm = (d.A[iv - 1] + d.lam[iv - 1] - (DIV ? d.mu[iv - 1] / dv : d.mu[iv - 1])) * m;
        else if (has_prev_interval(d, t)) xm = d.X_lo[v] * m;      // interval t0 - 1 lives in the previous time slab
        dt[0] = (xt - xm) * ih;
    } else {
        const DN<N> A = ldn<N>(d.A + iv), L = ldn<N>(d.lam + iv);
        P = ldn<N>(d.phi + iv);
        DN<N> M = ldn<N>(d.mu + iv);
        double xp = 0.0;
        if (t > 0) xp = (d.A[iv - 1] + d.lam[iv - 1] - (DIV ? d.mu[iv - 1] / dv : d.mu[iv - 1])) * m;
        if (DIV) {
#pragma unroll
            for (int u = 0; u < N; ++u) M.v[u] /= dv;
        }
        rhs_div_time<N>(d, t, m, xp, A, L, M, dt);
    }
    const int j0 = d.cptr[v], j1 = d.cptr[v + 1];
    if (CARRIED) carried_gather<N, CARRY_BATCH, 1>(d, d.cn_g + t, j0, j1, ds);
    for (int j = CARRIED ? j1 : j0; j < j1; ++j) {
        const int f = d.cidx[j] / 3;
        double g[N][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double ga = d.c_gA[j * 3 + c];
            const int64_t i = idxF(d, f, c, t);
            const DN<N> b = ldn<N>(d.B + i), e = ldn<N>(d.E + i);
#pragma unroll
            for (int u = 0; u < N; ++u) g[u][c] = ga * (b.v[u] - (DIV ? e.v[u] / dv : e.v[u]));
        }
#pragma unroll
        for (int u = 0; u < N; ++u) ds[0][u] += sum3(g[u][0], g[u][1], g[u][2]);
    }
    if constexpr (N == 1) P = ldn<N>(d.phi + iv);
    rhs_finish<N>(d, t, r, eps, m, dt, P, ds, d.mu0, d.mu1, v, out);
}
template <bool CARRIED = false, bool DIV = false>
__device__ __forceinline__ double rhs_value(const Dev &d, int v, int t, double r, double eps, double dv = 1.0) {
    double b[1];
    rhs_lane<1, CARRIED, DIV>(d, v, t, r, eps, b, dv);
    return b[0];
}

// Workgroups [n_rhs, gridDim.x) (when there are any): the cone projection, a quarter tile each, as in k_rhs_modes.
template <bool CARRIED>
__global__ __launch_bounds__(BLOCK) void k_rhs(Dev d, double r, double eps, int n_rhs, double sz, double cd) {
    __shared__ double lds[4];
    if ((int)blockIdx.x >= n_rhs) {
        const int G8 = (gridDim.x - n_rhs) / (TILE_ELEMS / BLOCK), b = blockIdx.x - n_rhs;
        const int st = xcd_tile(b % G8, d.n_vtiles);
        if (st >= d.n_vtiles) return;
        const int e = (b / G8) * BLOCK + threadIdx.x, v = st * d.VT + (e >> d.tp_shift), t = e & (d.TP - 1);
        if (v < d.V && t < d.ni) soc_lane<1, true, CARRIED>(d, v, t, sz, cd);
        return;
    }
    const int tile = xcd_tile(blockIdx.x, d.n_vtiles);
    double part[1] = {0.0};
    if (tile < d.n_vtiles) {
        const int v0 = tile * d.VT;
        for (int e = threadIdx.x; e < TILE_ELEMS; e += BLOCK) {
            const int v = v0 + (e >> d.tp_shift), t = e & (d.TP - 1);
            if (v >= d.V || t >= d.nl) continue;
            const double b = rhs_value<CARRIED>(d, v, t, r, eps);
            d.cg_b[idxV(d, v, t)] = b;
            part[0] += b;
        }
    }
    block_sum<1>(part, lds);
    if (threadIdx.x == 0) d.partials[blockIdx.x] = part[0];
}

// The same right-hand side followed at once by the time-mode transform of the tile (direct solver): b never goes
// to memory, the solver's input  bhat[v][a] = sum_t Q[t][a] b[v][t]  is written instead.
// 1024 threads: one right-hand-side value (a corner walk) per thread.
constexpr int RHS_NB = 1024;
// Workgroups [n_rhs, gridDim.x): the cone projection of a tile (it reads nothing this kernel or the solve writes
// and is as latency-bound as the corner walks here: one launch instead of two).
__global__ __launch_bounds__(RHS_NB) void k_rhs_modes(Dev d, double r, double eps, double *__restrict__ bhat, int IC, int n_rhs, double sz, double cd) {
    if ((int)blockIdx.x >= n_rhs) {
        const int st = xcd_tile(blockIdx.x - n_rhs, d.n_vtiles);
        if (st >= d.n_vtiles) return;
        const int e = threadIdx.x, v = st * d.VT + (e >> d.tp_shift), t = e & (d.TP - 1);
        if (v < d.V && t < d.ni) soc_lane<1, true>(d, v, t, sz, cd);
        return;
    }
    extern __shared__ double tm_lds[];
    const int n = d.T + 1, TP = d.TP, TPp = TP + 1;
    double *Qs = tm_lds;                 // [IC][TP]
    double *xs = tm_lds + IC * TP;       // [VT][TPp]
    const int tile = xcd_tile(blockIdx.x, d.n_vtiles);
    if (tile >= d.n_vtiles) return;
    const int v0 = tile * d.VT;
    stage_q_chunk<true, RHS_NB>(d, d.Q, Qs, 0, min(IC, n));      // ahead of the corner walks (as compiled not beside them: Q is waited for and written before the walks' loads are issued)
    for (int e = threadIdx.x; e < TILE_ELEMS; e += RHS_NB) {
        const int vl = e >> d.tp_shift, t = e & (TP - 1);
        xs[vl * TPp + t] = (v0 + vl < d.V && t < n) ? rhs_value(d, v0 + vl, t, r, eps) : 0.0;
    }
    modes_from_tile<true, RHS_NB>(d, d.Q, xs, Qs, IC, v0, bhat, -1, 0, 1 << 30, true);
}

// k_rhs_modes with two time columns per lane (one GPU, direct solver): 512 threads per tile.
constexpr int RHS_NB2 = RHS_NB / 2;
template <bool CARRIED, bool DIV = false>
__global__ __launch_bounds__(RHS_NB2) void k_rhs_modes2(Dev d, double r, double eps, double *__restrict__ bhat, int IC, int n_rhs, double sz, double cd, double dv) {
    const int e = 2 * threadIdx.x, vl = e >> d.tp_shift, t = e & (d.TP - 1);
    if ((int)blockIdx.x >= n_rhs) {
        const int st = xcd_tile(blockIdx.x - n_rhs, d.n_vtiles);
        if (st >= d.n_vtiles) return;
        const int v = st * d.VT + vl;
        if (v < d.V && t < d.ni) soc_lane<2, true, CARRIED, DIV>(d, v, t, sz, cd, dv);
        return;
    }
    extern __shared__ double tm_lds[];
    const int n = d.T + 1, TP = d.TP, TPp = TP + 1;
    double *Qs = tm_lds;                 // [IC][TP]
    double *xs = tm_lds + IC * TP;       // [VT][TPp]
    const int tile = xcd_tile(blockIdx.x, d.n_vtiles);
    if (tile >= d.n_vtiles) return;
    const int v0 = tile * d.VT;
    stage_q_chunk<true, RHS_NB2>(d, d.Q, Qs, 0, min(IC, n));      // ahead of the corner walks (as compiled not beside them: Q is waited for and written before the walks' loads are issued; k_rhs_modes2_deep overlaps them)
    for (int ee = e; ee < TILE_ELEMS; ee += 2 * RHS_NB2) {       // (one pass: TILE_ELEMS = 2 * RHS_NB2)
        const int vv = ee >> d.tp_shift, tt = ee & (TP - 1);
        const int v = v0 + vv;
        double b[2] = {0.0, 0.0};
        if (v < d.V && tt < n) rhs_lane<2, CARRIED, DIV>(d, v, tt, r, eps, b, dv);
        xs[vv * TPp + tt] = b[0];
        xs[vv * TPp + tt + 1] = tt + 1 < n ? b[1] : 0.0;
    }
    modes_from_tile<true, RHS_NB2>(d, d.Q, xs, Qs, IC, v0, bhat, -1, 0, 1 << 30, true);
}

// ---- k_rhs_modes2<true> with its loads in flight (pitch 8, 16 or 32) ----------------------------------------------------------------
// As compiled, the carried walks above wait for memory step after step: the vertex arrays, the values of interval t - 1 behind their
// branch, cptr, the carried rows CARRY_BATCH at a time, mu0 / mu1 behind theirs -- and the workgroup's barrier waits for the slowest
// lane.  Here a lane issues cptr together with everything that does not depend on it (addresses clamped instead of branches: every
// load is unconditional, what it must not use is dropped by a select), then ALL carried rows of its vertex: DEEP_BATCH corners per
// pass, rows clamped to the list, added in list order -- carried_gather with DEEP_BATCH; the rest is rhs_finish / soc_finish, as in rhs_lane<2, true> / soc_lane<2, true, true>.
// The rows in flight cost registers (occupancy): launch_rhs takes this form while a CU gets few workgroups (deep_launch_wins).
constexpr int DEEP_BATCH = 8;      // corners per pass (closed surfaces: valence ~ 6: one pass)
__device__ __forceinline__ void rhs_lane2_deep(const Dev &d, int v, int t, double r, double eps, double (&out)[2]) {
    const int iv = idxV(d, v, t), ip = t > 0 ? iv - 1 : iv;
    const int jc0 = d.cptr[v], jc1 = d.cptr[v + 1];
    const double m = d.mass_v[v];
    const D2 A = ld2(d.A + iv), L = ld2(d.lam + iv), P = ld2(d.phi + iv), M = ld2(d.mu + iv);
    const double Ap = d.A[ip], Lp = d.lam[ip], Mp = d.mu[ip];
    const double m0 = d.mu0[v], m1 = d.mu1[v];
    double dt[2], ds[1][2] = {};
    carried_gather<2, DEEP_BATCH, 1>(d, d.cn_g + t, jc0, jc1, ds);
    rhs_div_time<2>(d, t, m, t > 0 ? (Ap + Lp - Mp) * m : 0.0, A, L, M, dt);
    rhs_finish<2>(d, t, r, eps, m, dt, P, ds, &m0, &m1, 0, out);
}
__device__ __forceinline__ void soc_lane2_deep(const Dev &d, int v, int t, double sz, double cd) {
    const int iv = idxV(d, v, t);
    const int j0 = d.cptr[v], j1 = d.cptr[v + 1];
    const D2 A = ld2(d.A + iv), bf = ld2(d.bf + iv), be = ld2(d.be + iv);
    double acc[2][2] = {};
    carried_gather<2, DEEP_BATCH, 2>(d, d.cn_sq + t, j0, j1, acc);
    soc_finish<2, true>(d, iv, t, sz, cd, acc, A, bf, be);
}

// k_rhs_modes2<true> in that form: Q is loaded first and held in registers while the walk's loads are in flight, written to LDS with
// the tile, and the transform is modes_from_tile_fast.  Same grid, same tiles, same riders.
template <int TPC>
__global__ __launch_bounds__(RHS_NB2) void k_rhs_modes2_deep(Dev d, double r, double eps, double *__restrict__ bhat, int n_rhs, double sz, double cd) {
    const int e = 2 * threadIdx.x, vl = e / TPC, t = e & (TPC - 1);
    if ((int)blockIdx.x >= n_rhs) {
        const int st = xcd_tile(blockIdx.x - n_rhs, d.n_vtiles);
        if (st >= d.n_vtiles) return;
        const int v = st * d.VT + vl;
        if (v < d.V && t < d.ni) soc_lane2_deep(d, v, t, sz, cd);
        return;
    }
    extern __shared__ dots_d2v tm_lds_deep[];
    constexpr int XP = fast_tile_pitch(TPC);
    double *Qs = reinterpret_cast<double *>(tm_lds_deep);      // [TPC][TPC]
    double *xs = Qs + TPC * TPC;                                // [VT][XP]
    const int n = d.T + 1;
    const int tile = xcd_tile(blockIdx.x, d.n_vtiles);
    if (tile >= d.n_vtiles) return;
    const int v0 = tile * d.VT, v = v0 + vl;
    QStage<true, RHS_NB2, TPC> qs;
    qs.load(d, d.Q);
    double b[2] = {0.0, 0.0};
    if (v < d.V && t < n) rhs_lane2_deep(d, v, t, r, eps, b);
    qs.store(Qs);
    dots_d2v bb;
    bb.x = b[0];
    bb.y = t + 1 < n ? b[1] : 0.0;
    *reinterpret_cast<dots_d2v *>(xs + vl * XP + t) = bb;      // (t even, XP even: aligned)
    __syncthreads();
    modes_from_tile_fast<RHS_NB2, TPC>(d, xs, Qs, v0, bhat);
}

// T + 1 >= 64: 32 vertices per workgroup, the transform on the matrix cores.
template <bool CARRIED, bool DIV = false>
__global__ __launch_bounds__(RHS_NB) void k_rhs_modes_mfma(Dev d, double r, double eps, double *__restrict__ bhat, int n_rhs, int n_tiles, double sz, double cd, double dv) {
    if ((int)blockIdx.x >= n_rhs) {      // riders: the cone projection of a tile, as in k_rhs_modes
        const int st = xcd_tile(blockIdx.x - n_rhs, d.n_vtiles);
        if (st >= d.n_vtiles) return;
        const int e = threadIdx.x, v = st * d.VT + (e >> d.tp_shift), t = e & (d.TP - 1);
        if (v < d.V && t < d.ni) soc_lane<1, true, CARRIED, DIV>(d, v, t, sz, cd, dv);
        return;
    }
    extern __shared__ double xs_m[];                    // [TM_ROWS][TP + 1]
    const int n = d.T + 1, TP = d.TP, TPp = TP + 1;
    const int tile = xcd_tile(blockIdx.x, n_tiles);     // neighbouring tiles walk the same triangles: one XCD (one L2) for a run of them
    if (tile >= n_tiles) return;
    const int v0 = tile * TM_ROWS;
    for (int e = threadIdx.x; e < TM_ROWS * TP; e += RHS_NB) {
        const int vl = e >> d.tp_shift, t = e & (TP - 1);
        xs_m[vl * TPp + t] = (v0 + vl < d.V && t < n) ? rhs_value<CARRIED, DIV>(d, v0 + vl, t, r, eps, dv) : 0.0;
    }
    __syncthreads();
    modes_from_tile_mfma<RHS_NB / 64>(d, d.Qpad, xs_m, v0, bhat);
}

// The facts rhs_choice decides from (step_choice.h), for a launch with or without the riding projection and a division or none
static RhsFacts rhs_facts(const Ctx *c, bool with_soc, bool pending) {
    const int g = xcd_grid(c->d.n_vtiles);
    return RhsFacts{rhs_writes_modes(c), time_modes_mfma_ok(c->d), c->d.TP >= 4, c->carried.carry_valid != 0, deep_launch_wins(c, with_soc ? 2 * g : g), with_soc, pending};
}
// the right-hand-side (+ projection) launch that launch_rhs would pick can divide the dual arrays as it reads them
bool rhs_divides(const Ctx *c) { return rhs_choice(rhs_facts(c, true, true)).divides; }

int launch_rhs(Ctx *c, bool with_soc, double dv, const RhsAhead *ahead) {
    Dev d = c->d;
    double r = c->prm.r;
    if (ahead) { d.zf = ahead->zf; d.ze = ahead->ze; d.lamc = ahead->lamc; r = ahead->r; }
    r /= c->prm.boundary_scale;
    const int g = xcd_grid(d.n_vtiles);
    const double eps = c->prm.eps, sz = c->prm.scale_z, cd = c->prm.const_d;
    const RhsChoice ch = rhs_choice(rhs_facts(c, with_soc, dv != 0.0));
    if (ch.refused) { set_error("launch_rhs: a pending penalty division was handed to a right-hand-side launch that cannot apply it"); return DOTS_ERR_STATE; }
    const double dvk = ch.variant == RHS_DIVIDING ? dv : 1.0;
    switch (ch.kernel) {
        case RHS_MFMA: {      // (two time columns per lane measured here too: knot63 -1.5 %, torus65k_T127 +1.5 %: not kept)
            const int n_tiles = (d.V + TM_ROWS - 1) / TM_ROWS, n_rhs = xcd_grid(n_tiles);
            with_constant<RHS_CARRIED, RHS_DIVIDING, RHS_NEITHER>(ch.variant, [&](auto V) {
                hipLaunchKernelGGL((k_rhs_modes_mfma<V == RHS_CARRIED, V == RHS_DIVIDING>), dim3(n_rhs + (with_soc ? g : 0)), dim3(RHS_NB), sizeof(double) * TM_ROWS * (d.TP + 1), c->stream,
                                   d, r, eps, d.cg_p0, n_rhs, n_tiles, sz, cd, dvk);
            });
            break;
        }
        case RHS_MODES2_DEEP:
            with_constant<8, 16, 32>(d.TP, [&](auto TPC) {
                hipLaunchKernelGGL((k_rhs_modes2_deep<TPC>), dim3(with_soc ? 2 * g : g), dim3(RHS_NB2), time_modes_fast_lds(d), c->stream, d, r, eps, d.cg_p0, g, sz, cd);
            });
            break;
        case RHS_MODES2:      // two time columns per lane (16-byte accesses)
            with_constant<RHS_CARRIED, RHS_DIVIDING, RHS_NEITHER>(ch.variant, [&](auto V) {
                hipLaunchKernelGGL((k_rhs_modes2<V == RHS_CARRIED, V == RHS_DIVIDING>), dim3(with_soc ? 2 * g : g), dim3(RHS_NB2), time_modes_tile_lds(d), c->stream, d, r, eps, d.cg_p0,
                                   time_modes_chunk(d), g, sz, cd, dvk);
            });
            break;
        case RHS_MODES:
            hipLaunchKernelGGL(k_rhs_modes, dim3(with_soc ? 2 * g : g), dim3(RHS_NB), time_modes_tile_lds(d), c->stream, d, r, eps, d.cg_p0, time_modes_chunk(d), g, sz, cd);
            break;
        case RHS_PLAIN:       // (carried: a time slab of the direct solver's iteration)
            with_constant<true, false>(ch.variant == RHS_CARRIED, [&](auto CARRIED) {
                hipLaunchKernelGGL(k_rhs<CARRIED>, dim3(with_soc ? g + g * (TILE_ELEMS / BLOCK) : g), dim3(BLOCK), 0, c->stream, d, r, eps, g, sz, cd);
            });
            break;
    }
    DOTS_HIP(hipGetLastError());
    c->carried.step_path = ch.path;      // the first launch of an iteration: a new record (dots_debug_counter 12)
    c->carried.deep_path = ch.deep;      // (dots_debug_counter 15)
    return 0;
}

// ------------------------------------------------------------------------------------------
// Steps 2 + 3 fused                            (reference: solver_socp.py:709-722, :1044-1065)
// Vertex part, thread (v, t < T):
//     dphi = (phi[t+1] - phi[t]) / h
//     A = (dphi + mu)/a2 + (a1/a2)(z_end + beta_end - z_fst - beta_fst);  lambda_c = cr/(1+cr) (dphi + mu - A)
//     mu += tau (dphi - A - lambda_c);  beta_fst += tau (z_fst + sz A - d);  beta_end += tau (z_end - sz A - d)
// Triangle part, thread (f, c, t <= T):
//     gx = sum_k hat[f][k][c] phi[tri[f][k]][t]                       (grad_space, 3 coalesced row gathers)
//     B  = (gx + E + sz/sqrt3 * (sum_k (z_mid+beta_mid)[t][s=0] + sum_k (z_mid+beta_mid)[t-1][s=1])) / diag_b[t]
//     E += tau (gx - B)
//     beta_mid[t][0][k] += tau (z_mid - sz/sqrt3 B[t]);  beta_mid[t-1][1][k] += tau (z_mid - sz/sqrt3 B[t])
// Every beta_mid entry is attached to the node whose B it is compared with, so the thread that
// computes B[t] updates them without any exchange: z_mid and beta_mid are read once, beta_mid written once.
// ------------------------------------------------------------------------------------------
// QONLY: only the (q, lambda_c) closed form (the reference's "Step 0" of is_palm = True, solver_socp.py:668-672):
// A, B and lambda_c are written, no multiplier moves.
// The fused KKT sums of the vertex part (DOTS_STEP_KKT_SUMS): the slots of kkt_vertex_body that need nothing beyond this element
constexpr int KV_N = 10;
constexpr int KV_SLOT[KV_N] = {V_DPHI2, V_A2, V_LAM2, V_RESMU2, V_RFST2, V_REND2, V_MU2, V_AUX1_2, V_MUAUX1_2, V_CONG_RES2};
// ... and of the triangle part
constexpr int KF_N = 7;
constexpr int KF_SLOT[KF_N] = {F_DX2, F_B2, F_RESE2, F_E2, F_AUX2_2, F_EAUX2_2, F_RMID2};

// KKT: the vertex sums that need nothing beyond this element (the slots KV_SLOT), on the values it has just computed; sv is indexed by V_*
template <bool QONLY, int NB = BLOCK, bool KKT = false, bool DIV = false>
__device__ __forceinline__ void q_lambda_vertex_tile(const Dev &d, int tile, double sz, double cd, double cr, double tau, const KktArgs *ka = nullptr,
                                                     double *sv = nullptr, double dv = 1.0) {
    const int v0 = tile * d.VT;
    const double a1 = sz * (1.0 + cr);
    const double a2 = 1.0 + 2.0 * sz * a1;
    const double ia2 = 1.0 / a2, a12 = a1 / a2, cl = cr / (1.0 + cr), ih = 1.0 / d.h;
    for (int e = threadIdx.x; e < TILE_ELEMS; e += NB) {
        const int v = v0 + (e >> d.tp_shift), t = e & (d.TP - 1);
        if (v >= d.V || t >= d.ni) continue;
        const int iv = idxV(d, v, t);
        const double dphi = (next_node(d, d.phi, d.phi_hi, v, t) - d.phi[iv]) * ih;
        const double zf = d.zf[iv], ze = d.ze[iv];
        double mu = d.mu[iv], bf = d.bf[iv], be = d.be[iv];
        if (DIV) { mu /= dv; bf /= dv; be /= dv; }      // (a pending penalty update: see soc_lane)
        const double memo = dphi + mu;
        const double a = ia2 * memo + a12 * (ze + be - zf - bf);
        const double lc = cl * (memo - a);
        d.A[iv] = a;
        d.lam[iv] = lc;
        if (QONLY) continue;
        const double mun = mu + tau * (dphi - a - lc), bfn = bf + tau * (zf + sz * a - cd), ben = be + tau * (ze - sz * a - cd);
        d.mu[iv] = mun;
        d.bf[iv] = bfn;
        d.be[iv] = ben;
        if (KKT) {
            const double m = d.mass_v[v];
            kkt_v_prim_q(sv, dphi, a, lc, m);
            sv[V_LAM2] += wsq(lc, m);
            kkt_v_prim_z(sv, *ka, zf, ze, a, m);
            sv[V_MU2] += wsq(mun, m);
            kkt_v_dual_beta(sv, *ka, mun, bfn, ben, m);
            kkt_v_cong(sv, *ka, mun, lc, m);
        }
    }
}

// The triangle part for the N consecutive nodes (t .. t + N - 1) of row (f, c) that one lane owns.
// ZMODE 0: z_mid is read from memory; 1: rebuilt from the cone multiplier (zmid_of) and stored; 2: rebuilt, not stored.
// N = 1 (k_q_lambda_mult_triangle: time slabs, pitch 2, PALM stage 0): 8-byte accesses; entries whose interval does not exist are not stored.
// N = 2 (t even; k_q_lambda_mult_triangle2, k_q_lambda_mult_carry): every array of the triangle part is read and written in the column of
// the node (idxM), so both nodes of a lane sit in one aligned 16-byte word of every row; the mesh constants of (f, c) are loaded once for both.
// Half the waves for the same bytes: these launches are latency-bound at full occupancy on the small meshes (time ~ waves x chain / resident waves).
// (k_q_lambda_mult_triangle2: 120-122 VGPRs = 4 waves per SIMD.  Forcing 5 / 6 with amdgpu_waves_per_eu spills 44 / 132 bytes per lane and loses:
// torus100k 571 -> 553 / 472 it/s, knot 10 530 -> 9 750 / 7 980: profiles/studies/r03_steps23_forced_occupancy.txt)
// All loads come first and unconditional: the compiler then issues them back to back instead of one wait per guarded load.  Both corner entries of a
// node sit in ITS column, whether their interval exists or not (then the slot holds a zero that is masked below); the multiplier of interval t - 1
// comes from the previous time slab's halo when t is the slab's first node.
// CARRY (k_q_lambda_mult_carry): the lane also forms, from the registers that hold the NEW B, E and beta_mid, what the next
// iteration's right-hand side and cone projection would gather from memory -- per corner k of its triangle and node u its
// xyz component's share of  |D (sB B - beta_mid)|^2  (both halves: s = 0 of interval t + u, s = 1 of interval t + u - 1) and of
// area * hat . (B - E) -- and leaves them in LDS (xl: this lane's column, stride NBX) for the fold over xyz; its z_mid stores are non-temporal
// (z_mid is not read again inside the loop).
constexpr int CARRY_NB = 192;         // 3 wavefronts: 2 * 192 / TP rows = whole triangles for every pitch <= 128
constexpr int CARRY_VALUES = 18;      // per lane: 3 corners x (2 halves + 1 divergence share) x 2 nodes
// KKT: the lane also accumulates the triangle sums that need no gather (sf, indexed by F_* - N_VSUMS: the slots KF_SLOT; sz = scale_factor_z).
// BMNT: beta_mid is loaded and stored with the non-temporal hint (FrontSchedule::bm_nt: where the factor can live in the 256 MB Infinity Cache if the
// 36 T F values of beta_mid that stream through every iteration do not displace it -- sphere10k: 5 130-5 190 -> 5 490-5 500 it/s; where
// everything fits (knot) the hint costs 2 %, where nothing does (torus100k) it changes nothing: profiles/studies/r04_nontemporal.txt)
template <int N, int ZMODE, bool QONLY, bool CARRY, bool KKT = false, bool DIV = false, bool BMNT = false>
__device__ __forceinline__ void ql_lane(const Dev &d, int f, int c, int t, double sB, double diag_in, double diag_bd, double tau, double *xl = nullptr,
                                        double sz = 0.0, double *sf = nullptr, double dv = 1.0) {
    static_assert(N == 2 || !(CARRY || KKT), "the carried shares and the fused sums are laid out for two nodes per lane");
    const bool whole = N == 2 && t + 1 < d.nl;      // the lane's 16-byte words are stored whole (always, unless the slab holds an odd number of nodes)
    const int64_t ie = idxF(d, f, c, t);
    int vk[3];
    double hk[3], Dk[3];
    DN<N> phik[3], l0[3], b0[3], b1[3], z0[3], z1[3];
    double lm1[3];                                  // the multiplier of interval t - 1 (that of interval t is l0[.].v[0])
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        vk[k] = d.tri[f * 3 + k];
        hk[k] = d.hat[(f * 3 + k) * 3 + c];
        Dk[k] = (ZMODE || CARRY) ? d.fk_D[f * 3 + k] : 1.0;
    }
    const double area = (CARRY || KKT) ? d.area_f[f] : 0.0;
    const bool has1_0 = has_prev_interval(d, t);
    DN<N> Bold = {};
    if (ZMODE) Bold = ldn<N>(d.B + ie);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        phik[k] = ldn<N>(d.phi + idxV(d, vk[k], t));
        b0[k] = BMNT ? ldn_nt<N>(d.bm + idxM(d, f * 3 + k, 0, c, t)) : ldn<N>(d.bm + idxM(d, f * 3 + k, 0, c, t));
        b1[k] = BMNT ? ldn_nt<N>(d.bm + idxM(d, f * 3 + k, 1, c, t - 1)) : ldn<N>(d.bm + idxM(d, f * 3 + k, 1, c, t - 1));
        if (DIV) {      // (a pending penalty update: see soc_lane)
#pragma unroll
            for (int u = 0; u < N; ++u) { b0[k].v[u] /= dv; b1[k].v[u] /= dv; }
        }
        if (ZMODE) {
            l0[k] = ldn<N>(d.lamc + idxV(d, vk[k], t));
            const double *pl = t > 0 ? d.lamc + idxV(d, vk[k], t - 1) : (has1_0 ? d.lamc_lo + vk[k] : d.lamc + idxV(d, vk[k], t));
            lm1[k] = *pl;
        } else {
            z0[k] = ldn<N>(d.zm + idxM(d, f * 3 + k, 0, c, t));
            z1[k] = ldn<N>(d.zm + idxM(d, f * 3 + k, 1, c, t - 1));
        }
    }
    DN<N> Eo = ldn<N>(d.E + ie);
    if (DIV) {
#pragma unroll
        for (int u = 0; u < N; ++u) Eo.v[u] /= dv;
    }
    DN<N> Bn, En, n0[3], n1[3];
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const int tu = t + u;
        const bool has0 = tu < d.ni, has1 = has_prev_interval(d, tu);
        double gx = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) gx += hk[k] * phik[k].v[u];
        double S = 0.0;
        const double sBold = sB * Bold.v[u];      // both pre-images of a node's corners use B_old at ITS node
        double zz0[3], zz1[3], bb0[3], bb1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            bb0[k] = b0[k].v[u];
            bb1[k] = b1[k].v[u];
            if (ZMODE) {
                zz0[k] = zmid_of(l0[k].v[u], Dk[k], sBold, bb0[k]);
                zz1[k] = zmid_of(u == 0 ? lm1[k] : l0[k].v[0], Dk[k], sBold, bb1[k]);
            } else {
                zz0[k] = z0[k].v[u];
                zz1[k] = z1[k].v[u];
            }
            if (!has0) zz0[k] = bb0[k] = 0.0;
            if (!has1) zz1[k] = bb1[k] = 0.0;
            z0[k].v[u] = zz0[k];
            z1[k].v[u] = zz1[k];
            S += (zz0[k] + bb0[k]) + (zz1[k] + bb1[k]);
        }
        const double bn = (gx + Eo.v[u] + sB * S) / ((first_node(d, tu) || last_node(d, tu)) ? diag_bd : diag_in);
        Bn.v[u] = bn;
        En.v[u] = Eo.v[u] + tau * (gx - bn);
        const double sBn = sB * bn;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            // slots whose interval does not exist keep what they hold (zeros)
            n0[k].v[u] = has0 ? bb0[k] + tau * (zz0[k] - sBn) : b0[k].v[u];
            n1[k].v[u] = has1 ? bb1[k] + tau * (zz1[k] - sBn) : b1[k].v[u];
        }
        if (KKT && tu < d.nl) {      // conditions 0, 3 and the z_mid part of 1, on the values just computed
            const double en = En.v[u];
            kkt_f_prim_q(sf, gx, bn, area);
            sf[F_E2 - N_VSUMS] += wsq(en, area);
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (has0) s0 += n0[k].v[u];
                if (has1) s1 += n1[k].v[u];
            }
            kkt_f_dual_beta(sf, sB, en, s0, s1, area);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (has0) kkt_f_rmid(sf, sz, zz0[k], sBn, area);
                if (has1) kkt_f_rmid(sf, sz, zz1[k], sBn, area);
            }
        }
        if (CARRY) {      // the expressions of soc_lane / rhs_lane on the values those will find in memory
            const bool node = tu < d.nl;
            const double de = bn - En.v[u];
            if (KKT) {    // ... and of Dual(alpha)'s gather (kkt_vertex_body: sum over the corners of area * hat . E)
#pragma unroll
                for (int k = 0; k < 3; ++k) xl[(CARRY_VALUES + k * 2 + u) * CARRY_NB] = node ? (hk[k] * area) * En.v[u] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                xl[(k * 6 + u) * CARRY_NB] = has0 ? soc_w2(Dk[k], sBn, n0[k].v[u]) : 0.0;               // s = 0 half of interval tu
                xl[(k * 6 + 2 + u) * CARRY_NB] = (has1 && node) ? soc_w2(Dk[k], sBn, n1[k].v[u]) : 0.0;  // s = 1 half of interval tu - 1
                xl[(k * 6 + 4 + u) * CARRY_NB] = node ? (hk[k] * area) * de : 0.0;                       // div_x share at node tu
            }
        }
    }
    if (whole) {
        if (ZMODE == 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                // (entries of intervals that do not exist are stored as the zeros computed above; their slots are never read as data)
                double *p0 = d.zm + idxM(d, f * 3 + k, 0, c, t), *p1 = d.zm + idxM(d, f * 3 + k, 1, c, t - 1);
                if (CARRY) { stn_nt<N>(p0, z0[k]); stn_nt<N>(p1, z1[k]); }
                else { stn<N>(p0, z0[k]); stn<N>(p1, z1[k]); }
            }
        }
        stn<N>(d.B_st + ie, Bn);
        if (QONLY) return;
        stn<N>(d.E + ie, En);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double *p0 = d.bm_st + idxM(d, f * 3 + k, 0, c, t), *p1 = d.bm_st + idxM(d, f * 3 + k, 1, c, t - 1);
            if (BMNT) { stn_nt<N>(p0, n0[k]); stn_nt<N>(p1, n1[k]); }
            else { stn<N>(p0, n0[k]); stn<N>(p1, n1[k]); }
        }
    } else {      // one node (N = 1, or only the first node of the pair exists): element-wise stores, none to an entry whose interval does not exist
        const bool has0 = t < d.ni, has1 = has1_0;
        if (ZMODE == 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (has0) d.zm[idxM(d, f * 3 + k, 0, c, t)] = z0[k].v[0];
                if (has1) d.zm[idxM(d, f * 3 + k, 1, c, t - 1)] = z1[k].v[0];
            }
        }
        d.B_st[ie] = Bn.v[0];
        if (QONLY) return;
        d.E[ie] = En.v[0];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (has0) d.bm_st[idxM(d, f * 3 + k, 0, c, t)] = n0[k].v[0];
            if (has1) d.bm_st[idxM(d, f * 3 + k, 1, c, t - 1)] = n1[k].v[0];
        }
    }
}

// Workgroups [0, nf8 * SUB) do the triangle part, N elements per thread: a workgroup takes a quarter (N = 1) or half (N = 2) of a triangle tile;
// the vertex part (independent of it: different arrays) rides in the same launch as workgroups [nf8 * SUB, nf8 * SUB + nv8).
template <int N, int ZMODE, bool QONLY>
__device__ __forceinline__ void ql_tile_kernel(const Dev &d, double sz, double tau, int nf8, double cd, double cr) {
    constexpr int SUB = TILE_ELEMS / (N * BLOCK);
    if ((int)blockIdx.x >= nf8 * SUB) {
        const int vt = xcd_tile(blockIdx.x - nf8 * SUB, d.n_vtiles);
        if (vt < d.n_vtiles) q_lambda_vertex_tile<QONLY>(d, vt, sz, cd, cr, tau);
        return;
    }
    const int tile = xcd_tile(blockIdx.x % nf8, d.n_ftiles);
    if (tile >= d.n_ftiles) return;
    const int e = ((blockIdx.x / nf8) * BLOCK + threadIdx.x) * N;          // first of the lane's elements in the tile
    const int row = tile * d.FT + (e >> d.tp_shift), t = e & (d.TP - 1);
    if (row >= 3 * d.F || t >= d.nl) return;
    ql_lane<N, ZMODE, QONLY, false>(d, row / 3, row % 3, t, sz * INV_SQRT3, 1.0 + 2.0 * sz * sz, 1.0 + sz * sz, tau);
}
template <int ZMODE, bool QONLY = false>
__global__ __launch_bounds__(BLOCK) void k_q_lambda_mult_triangle(Dev d, double sz, double tau, int nf8, double cd, double cr) {
    ql_tile_kernel<1, ZMODE, QONLY>(d, sz, tau, nf8, cd, cr);
}
template <int ZMODE, bool QONLY = false>
__global__ __launch_bounds__(BLOCK) void k_q_lambda_mult_triangle2(Dev d, double sz, double tau, int nf8, double cd, double cr) {
    ql_tile_kernel<2, ZMODE, QONLY>(d, sz, tau, nf8, cd, cr);
}

// Steps 2+3 that also CARRY the next iteration's gathers (DOTS_STEP_CARRY; one GPU, pitch <= 128).  A workgroup of 192 lanes takes
// whole triangles (the three xyz rows of a triangle are TP / 2 lanes apart), the lanes exchange their shares through LDS and the
// lane of component c folds corner k = c over xyz -- (x + y) + z, the association of sum3 -- and stores
//     cn_sq[j][0][interval]   the s = 0 half of |D (sB B - beta_mid)|^2 of corner-list entry j,
//     cn_sq[j][1][interval]   the s = 1 half (formed at node interval + 1: it comes from the next lane of the row),
//     cn_g[j][node]           area * hat_k . (B - E),
// j = cpos[f * 3 + k]: the rows of a vertex's corners are CONTIGUOUS, so the next right-hand-side / projection launch streams
// them (soc_lane / rhs_lane <CARRIED>) instead of walking index lists into B, E and beta_mid.
// Replaces one of the three passes over beta_mid per iteration (solver_socp.py:997-1017 reads what :716-722 just wrote).
// 148-152 VGPRs = 3 waves per SIMD by themselves; the instantiation with the KKT sums is held there (170 otherwise).
// (Measured: 4 waves per SIMD capped the registers at 128 and spilled 20: knot 10 900 -> 9 500 it/s, torus100k 630 -> 585)
#define CARRY_OCCUPANCY __attribute__((amdgpu_waves_per_eu(3)))
// the fused slots of a lane's sums (s, indexed by slot - first) added over the workgroup and stored into the fused-KKT buffers: slot SLOT[i] of
// block `bid` of `nblk`
template <int N>
__device__ __forceinline__ void store_fused(const double *s, const int (&slot)[N], int first, double *__restrict__ part, int nblk, int bid, double *lds) {
    double v[N];
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = s[slot[i] - first];
    block_sum<N, CARRY_NB / 64>(v, lds);
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int i = 0; i < N; ++i) part[(int64_t)(slot[i] - first) * nblk + bid] = v[i];
}
template <int ZMODE, bool KKT = false, bool DIV = false, bool BMNT = false>
__global__ __launch_bounds__(CARRY_NB) CARRY_OCCUPANCY void k_q_lambda_mult_carry(Dev d, double sz, double tau, int n_fwg, int tri_per_wg, double cd, double cr,
                                                                                  KktArgs ka, KktFused kf, double dv, int emit) {
    // emit: bit 0 the gathers of the next right-hand side / projection (cn_sq, cn_g: DOTS_STEP_CARRY), bit 1 those of this
    // iterate's Dual(alpha) residual (cn_e: DOTS_STEP_KKT_SUMS, KKT instantiations only)
    __shared__ double xs[(CARRY_VALUES + (KKT ? 6 : 0)) * CARRY_NB];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= n_fwg) {
        const int vb = blockIdx.x - n_fwg, vt = xcd_tile(vb, d.n_vtiles);
        double sv[N_VSUMS] = {};
        if (vt < d.n_vtiles) q_lambda_vertex_tile<false, CARRY_NB, KKT, DIV>(d, vt, sz, cd, cr, tau, &ka, sv, dv);
        if (KKT) store_fused<KV_N>(sv, KV_SLOT, 0, kf.part_v, kf.nv, vb, xs);
        return;
    }
    const int wg = xcd_tile(blockIdx.x, (d.F + tri_per_wg - 1) / tri_per_wg);
    const int e = 2 * tid, lr = e >> d.tp_shift, t = e & (d.TP - 1);      // local row (3 per triangle), first node
    const int f = wg * tri_per_wg + lr / 3, c = lr - 3 * (lr / 3);
    const bool active = f < d.F && t < d.nl;      // (a whole triangle is active or not; so is a column over its three rows)
    const int j = active ? d.cpos[f * 3 + c] : 0; // row of this lane's corner k = c in the carried arrays (loaded with the lane's other constants)
    double sf[N_FSUMS] = {};
    if (active) ql_lane<2, ZMODE, false, true, KKT, DIV, BMNT>(d, f, c, t, sz * INV_SQRT3, 1.0 + 2.0 * sz * sz, 1.0 + sz * sz, tau, xs + tid, sz, sf, dv);
    __syncthreads();
    const int L = d.TP >> 1;                      // lanes per row
    const int t0 = tid - c * L;                   // the lane of component 0 of this triangle and column
    double q[6];                                  // corner k = c: s = 0 halves (nodes t, t + 1), s = 1 halves, divergence shares
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double *x = xs + (c * 6 + i) * CARRY_NB + t0;
        q[i] = active ? sum3(x[0], x[L], x[2 * L]) : 0.0;
    }
    // q[2], q[3]: s = 1 halves of the intervals t - 1 and t.  Stored by interval: (t, t + 1) = (own q[3], the next lane's q[2]);
    // the row's last lane (t = TP - 2) would need interval TP - 1 >= T, which does not exist.
    const double nxt = __shfl_down(q[2], 1, 64);
    if (active) {
        if (emit & 1) {
            st2_nt(d.cn_sq + ((int64_t)(2 * j) << d.tp_shift) + t, D2{{q[0], q[1]}});
            st2_nt(d.cn_sq + ((int64_t)(2 * j + 1) << d.tp_shift) + t, D2{{q[3], t + 2 < d.TP ? nxt : 0.0}});
            st2_nt(d.cn_g + ((int64_t)j << d.tp_shift) + t, D2{{q[4], q[5]}});
            if (t == 0 && has_prev_interval(d, 0)) d.cn_lo[j] = q[2];      // (time slab: the half of the previous slab's last interval formed here)
        }
        if (KKT && (emit & 2)) {
            const double *x0 = xs + (CARRY_VALUES + c * 2) * CARRY_NB + t0, *x1 = x0 + CARRY_NB;
            st2_nt(d.cn_e + ((int64_t)j << d.tp_shift) + t, D2{{sum3(x0[0], x0[L], x0[2 * L]), sum3(x1[0], x1[L], x1[2 * L])}});
        }
    }
    if (KKT) {
        __syncthreads();      // (the exchange values in xs have been read)
        store_fused<KF_N>(sf, KF_SLOT, N_VSUMS, kf.part_f, kf.nf, blockIdx.x, xs);
    }
}

// z_mid on demand (Carried::zmid): in place on z_mid's storage, which holds the beta_mid the last projection read;
// Bold: the B it read.  One node per lane; zmid_of, as the steps-2+3 kernels rebuild it (ZMODE 1).
__global__ __launch_bounds__(BLOCK) void k_rebuild_zmid(Dev d, const double *__restrict__ Bold, double sz, double dv) {
    const int tile = xcd_tile(blockIdx.x, d.n_ftiles);
    if (tile >= d.n_ftiles) return;
    const double sB = sz * INV_SQRT3;
    for (int e = threadIdx.x; e < TILE_ELEMS; e += BLOCK) {
        const int row = tile * d.FT + (e >> d.tp_shift), t = e & (d.TP - 1);
        if (row >= 3 * d.F || t >= d.nl) continue;
        const int f = row / 3, c = row - 3 * f;
        const bool has0 = t < d.ni, has1 = has_prev_interval(d, t);
        const double sBold = sB * Bold[idxF(d, f, c, t)];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int vk = d.tri[f * 3 + k];
            const double Dk = d.fk_D[f * 3 + k];
            if (has0) {
                double b = d.zm[idxM(d, f * 3 + k, 0, c, t)];
                if (dv != 0.0) b /= dv;
                d.zm[idxM(d, f * 3 + k, 0, c, t)] = zmid_of(d.lamc[idxV(d, vk, t)], Dk, sBold, b);
            }
            if (has1) {
                double b = d.zm[idxM(d, f * 3 + k, 1, c, t - 1)];
                if (dv != 0.0) b /= dv;
                d.zm[idxM(d, f * 3 + k, 1, c, t - 1)] = zmid_of(d.lamc[idxV(d, vk, t - 1)], Dk, sBold, b);
            }
        }
    }
}
int launch_rebuild_zmid(Ctx *c) {
    hipLaunchKernelGGL(k_rebuild_zmid, dim3(xcd_grid(c->d.n_ftiles)), dim3(BLOCK), 0, c->stream, c->d, c->B_alt, c->zmid_sz, c->zmid_dv);
    DOTS_HIP(hipGetLastError());
    return 0;
}

// Step 0 of is_palm = True: (A, B, lambda_c) from the current multipliers and the stored z_mid; nothing else moves.
int launch_q_lambda_only(Ctx *c) {
    const dots_params &p = c->prm;
    const int nf8 = xcd_grid(c->d.n_ftiles), nv8 = xcd_grid(c->d.n_vtiles);
    hipLaunchKernelGGL((k_q_lambda_mult_triangle<0, true>), dim3(nf8 * (TILE_ELEMS / BLOCK) + nv8), dim3(BLOCK), 0, c->stream, c->d, p.scale_z, p.tau, nf8,
                       p.const_d, p.congestion * p.r);
    DOTS_HIP(hipGetLastError());
    return 0;
}

// The facts ql_choice decides from (step_choice.h); tw, n_fwg: the carry mapping's triangles per workgroup and triangle workgroups (0 where
// the mapping does not exist)
static QlFacts ql_facts(const Ctx *c, int zmid_mode, bool pending, int *tw = nullptr, int *n_fwg = nullptr) {
    const bool possible = carry_possible(c);      // (pitch 4 .. 128)
    const int w = possible ? (2 * CARRY_NB / c->d.TP) / 3 : 0, nf = possible ? xcd_grid((c->d.F + w - 1) / w) : 0;
    if (tw) *tw = w;
    if (n_fwg) *n_fwg = nf;
    return QlFacts{possible, c->step_carry != 0, c->step_kkt != 0, zmid_mode, c->kkt_fused.part_v != nullptr,
                   xcd_grid(c->d.n_vtiles) <= c->kkt_fused_cap_v && nf <= c->kkt_fused_cap_f, c->d.slab != 0, c->step_palm != 0,
                   c->zmid_defer && c->B_alt, c->d.TP >= 4, c->sched.bm_nt != 0, pending};
}
// steps 2+3 as launch_q_lambda_mult would run them can divide the dual arrays as they read them (the carry kernels)
bool ql_divides(const Ctx *c, int zmid_mode) { return ql_choice(ql_facts(c, zmid_mode, true)).divides; }

int launch_q_lambda_mult(Ctx *c, int zmid_mode, double dv) {
    const dots_params &p = c->prm;
    const int nf8 = xcd_grid(c->d.n_ftiles), nv8 = xcd_grid(c->d.n_vtiles);
    const double cd = p.const_d, cr = p.congestion * p.r;
    int tw, n_fwg;
    const QlChoice ch = ql_choice(ql_facts(c, zmid_mode, dv != 0.0, &tw, &n_fwg));
    if (ch.refused) { set_error("launch_q_lambda_mult: a pending penalty division was handed to a steps-2+3 launch that cannot apply it"); return DOTS_ERR_STATE; }
    c->carried.drop_for_steps23();
    c->carried.step_path = (c->carried.step_path & ~STEP_PATH_QL_MASK) | ch.path;
    if (ch.kernel == QL_TRIANGLE2) {      // two nodes per lane (16-byte accesses)
        const dim3 g2(nf8 * (TILE_ELEMS / (2 * BLOCK)) + nv8);
        with_constant<2, 1, 0>(ch.Z, [&](auto Z) { hipLaunchKernelGGL((k_q_lambda_mult_triangle2<Z>), g2, dim3(BLOCK), 0, c->stream, c->d, p.scale_z, p.tau, nf8, cd, cr); });
        DOTS_HIP(hipGetLastError());
        return 0;
    }
    if (ch.kernel == QL_TRIANGLE) {
        const dim3 gf(nf8 * (TILE_ELEMS / BLOCK) + nv8);
        with_constant<2, 1, 0>(ch.Z, [&](auto Z) { hipLaunchKernelGGL((k_q_lambda_mult_triangle<Z>), gf, dim3(BLOCK), 0, c->stream, c->d, p.scale_z, p.tau, nf8, cd, cr); });
        DOTS_HIP(hipGetLastError());
        return 0;
    }
    // k_q_lambda_mult_carry
    const KktArgs ka{KKT_FUSED_MASK, p.r, p.scale_z, p.const_d, p.congestion, p.prim_scale, p.dual_scale, p.boundary_scale};
    KktFused kf = c->kkt_fused;
    kf.nv = nv8;
    kf.nf = n_fwg;
    const bool k = (ch.emit & 2) != 0;
    // z_mid on demand: nothing of it is stored; the new B / beta_mid go to the alternate buffers, the old ones stay (Carried::zmid)
    Dev dk = c->d;
    if (ch.defer) { dk.B_st = c->B_alt; dk.bm_st = c->d.zm; }
    with_constant<1, 2>(ch.Z, [&](auto Z) { with_constant<true, false>(k, [&](auto K) { with_constant<true, false>(dv != 0.0, [&](auto DIV) {
        with_constant<true, false>(c->sched.bm_nt != 0, [&](auto BMNT) {
            hipLaunchKernelGGL((k_q_lambda_mult_carry<Z, K, DIV, BMNT>), dim3(n_fwg + nv8), dim3(CARRY_NB), 0, c->stream, dk, p.scale_z, p.tau, n_fwg, tw, cd, cr, ka, kf, DIV ? dv : 1.0, ch.emit);
        }); }); }); });
    DOTS_HIP(hipGetLastError());
    if (ch.defer) {
        c->swap_deferred_zmid();
        c->carried.zmid = ZMID_DEFERRED;
        c->zmid_dv = dv;
        c->zmid_sz = p.scale_z;
    }
    c->carried.carry_valid = ch.emit & 1;
    if (k) { c->kkt_fused = kf; c->carried.kkt_fused_valid = 1; }
    return 0;
}

// ------------------------------------------------------------------------------------------
// scaling tools                                (reference: solver_socp.py:367-395)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_scale(double *x, int64_t n, double f) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) x[i] *= f;
}
__global__ __launch_bounds__(BLOCK) void k_divide(double *x, int64_t n, double f) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) x[i] /= f;
}

// Calibration launch for the PMC traffic counters (profiles/tools/pmc_summary.py): exactly one 8-byte load and
// one 8-byte store per element of the staging buffer, the access width of every kernel of this library.
__global__ __launch_bounds__(BLOCK) void k_calib_stream(double *x, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) x[i] = 2.0 * x[i];
}
int launch_calibration(Ctx *c, double *bytes_each_way) {
    const int64_t n = c->stage_count;
    hipLaunchKernelGGL(k_calib_stream, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, c->stage, n);
    DOTS_HIP(hipGetLastError());
    DOTS_HIP(hipStreamSynchronize(c->stream));
    *bytes_each_way = 8.0 * (double)n;
    return 0;
}

static int grid_for(int64_t n) {
    int64_t g = (n + BLOCK - 1) / BLOCK;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

int launch_scale_array(Ctx *c, int id, double f) {
    const int64_t n = array_count_device(c->d, id);
    hipLaunchKernelGGL(k_scale, dim3(grid_for(n)), dim3(BLOCK), 0, c->stream, c->arr(id), n, f);
    // a time slab keeps phi at the next slab's first node beside its own columns (written by the inverse transform, read by
    // grad_time in the KKT and norm kernels until the next solve): it is scaled with phi
    if (id == DOTS_PHI && c->d.slab && c->d.phi_hi) hipLaunchKernelGGL(k_scale, dim3(grid_for(c->d.V)), dim3(BLOCK), 0, c->stream, c->d.phi_hi, (int64_t)c->d.V, f);
    DOTS_HIP(hipGetLastError());
    return 0;
}

// x /= f for the five dual arrays in ONE launch (same division as k_divide, element for element)
struct DivideFive {
    double *p[5];
    int64_t end[5];      // running element counts
};
__global__ __launch_bounds__(BLOCK) void k_divide_five(DivideFive a, double f) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < a.end[4]; i += (int64_t)gridDim.x * BLOCK) {
        int k = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) k += i >= a.end[q];
        const int64_t j = i - (k ? a.end[k - 1] : 0);
        a.p[k][j] /= f;
    }
}

int launch_adjust_penalty(Ctx *c, double factor) {  // :367-371 (the boundary term is rebuilt from r in k_rhs)
    const int ids[5] = {DOTS_BETA_MID, DOTS_E, DOTS_MU, DOTS_BETA_FST, DOTS_BETA_END};
    DivideFive a{};
    int64_t n = 0;
    for (int k = 0; k < 5; ++k) {
        a.p[k] = c->arr(ids[k]);
        n += array_count_device(c->d, ids[k]);
        a.end[k] = n;
    }
    hipLaunchKernelGGL(k_divide_five, dim3(grid_for(n)), dim3(BLOCK), 0, c->stream, a, factor);
    DOTS_HIP(hipGetLastError());
    return 0;
}

// mu = sz (beta_fst - beta_end);  E = - L^T(beta_mid; sz)          (:386-388)
__global__ __launch_bounds__(BLOCK) void k_rebuild_mu(Dev d, double sz) {
    const int tile = xcd_tile(blockIdx.x, d.n_vtiles);
    if (tile >= d.n_vtiles) return;
    for (int e = threadIdx.x; e < TILE_ELEMS; e += BLOCK) {
        const int v = tile * d.VT + (e >> d.tp_shift), t = e & (d.TP - 1);
        if (v >= d.V || t >= d.ni) continue;
        const int iv = idxV(d, v, t);
        d.mu[iv] = sz * (d.bf[iv] - d.be[iv]);
    }
}
__device__ __forceinline__ double dec_adjoint_at(const Dev &d, const double *x, int f, int c, int t) {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (t < d.ni) s0 += x[idxM(d, f * 3 + k, 0, c, t)];
        if (has_prev_interval(d, t)) s1 += x[idxM(d, f * 3 + k, 1, c, t - 1)];
    }
    return s0 + s1;
}
__global__ __launch_bounds__(BLOCK) void k_rebuild_E(Dev d, double sz) {
    const int tile = xcd_tile(blockIdx.x, d.n_ftiles);
    if (tile >= d.n_ftiles) return;
    for (int e = threadIdx.x; e < TILE_ELEMS; e += BLOCK) {
        const int row = tile * d.FT + (e >> d.tp_shift), t = e & (d.TP - 1);
        if (row >= 3 * d.F || t >= d.nl) continue;
        const int f = row / 3, c = row - 3 * f;
        d.E[idxF(d, f, c, t)] = -(sz * INV_SQRT3) * dec_adjoint_at(d, d.bm, f, c, t);
    }
}

int launch_scale_z(Ctx *c, double z_mul, double beta_mul, double sz_new) {
    const int zs[3] = {DOTS_Z_FST, DOTS_Z_MID, DOTS_Z_END}, bs[3] = {DOTS_BETA_FST, DOTS_BETA_MID, DOTS_BETA_END};
    for (int id : zs) launch_scale_array(c, id, z_mul);
    for (int id : bs) launch_scale_array(c, id, beta_mul);
    hipLaunchKernelGGL(k_rebuild_mu, dim3(xcd_grid(c->d.n_vtiles)), dim3(BLOCK), 0, c->stream, c->d, sz_new);
    hipLaunchKernelGGL(k_rebuild_E, dim3(xcd_grid(c->d.n_ftiles)), dim3(BLOCK), 0, c->stream, c->d, sz_new);
    DOTS_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------
// layout conversion: reference layout (time-major) <-> device layout (time-fastest, permuted)
// ------------------------------------------------------------------------------------------
// Host layouts: one GPU -- the reference's (phi (T+1,V); interval arrays (T,V); B, E (T+1,F,3); z_mid, beta_mid (T,2,3,F,3)).
// Time slab -- the same with the slab's time extent: (nl,V), (ni,V), (nl,F,3), and the corner arrays as (nl,2,3,F,3)
// indexed by the NODE an entry belongs to (entry [j][s] is the reference's [t0 + j - s][s]; entries whose interval
// does not exist are ignored on upload and zero on download).
template <bool TO_DEV>
__global__ __launch_bounds__(BLOCK) void k_convert(Dev d, int kind, double *dev, double *host) {
    // one thread per device element (t fastest -> device side coalesced; host side strided, staging only)
    const int nt = (kind == 0 || kind == 2) ? d.nl : d.ni;
    const int64_t rows = (kind <= 1) ? d.V : (kind == 2 ? (int64_t)3 * d.F : (int64_t)18 * d.F);
    const int64_t n = rows << d.tp_shift;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const int t = (int)(i & (d.TP - 1));
        const int64_t row = i >> d.tp_shift;
        int64_t h;
        if (kind <= 1) {
            if (t >= nt) { if (TO_DEV) dev[i] = 0.0; continue; }
            const int v = d.perm_v ? d.perm_v[row] : (int)row;
            h = (int64_t)t * d.V + v;
        } else if (kind == 2) {
            if (t >= nt) { if (TO_DEV) dev[i] = 0.0; continue; }
            const int f = (int)(row / 3), c = (int)(row - 3 * (row / 3));
            const int fo = d.perm_f ? d.perm_f[f] : f;
            h = ((int64_t)t * d.F + fo) * 3 + c;
        } else {  // row = ((f*3+k)*2+s)*3+c, column t = node of the entry: interval t - s
            const int c = (int)(row % 3);
            const int s = (int)((row / 3) % 2);
            const int k = (int)((row / 6) % 3);
            const int f = (int)(row / 18);
            const int fo = d.perm_f ? d.perm_f[f] : f;
            const int ti = t - s, tg = d.t0 + ti;         // local / global interval of this slot
            const bool valid = t < d.nl && tg >= 0 && tg < d.T;
            if (!valid && !(d.slab && t < d.nl)) { if (TO_DEV) dev[i] = 0.0; continue; }
            h = ((((int64_t)(d.slab ? t : ti) * 2 + s) * 3 + k) * d.F + fo) * 3 + c;
            if (!valid) {       // a slab's host array has the slot, the interval does not exist
                if (TO_DEV) dev[i] = 0.0;
                else host[h] = 0.0;
                continue;
            }
        }
        if (TO_DEV) dev[i] = host[h];
        else host[h] = dev[i];
    }
}

int launch_to_device_layout(Ctx *c, int id, double *dev, const double *staged) {
    const int64_t n = array_count_device(c->d, id);
    hipLaunchKernelGGL(k_convert<true>, dim3(grid_for(n)), dim3(BLOCK), 0, c->stream, c->d, array_kind(id), dev,
                       const_cast<double *>(staged));
    DOTS_HIP(hipGetLastError());
    return 0;
}
int launch_from_device_layout(Ctx *c, int id, const double *dev, double *staged) {
    const int64_t n = array_count_device(c->d, id);
    hipLaunchKernelGGL(k_convert<false>, dim3(grid_for(n)), dim3(BLOCK), 0, c->stream, c->d, array_kind(id), const_cast<double *>(dev), staged);
    DOTS_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------
// standalone operators (rows a4-a6): same index arithmetic as the fused kernels, exposed so each
// reference function has a one-to-one parity test.  in/out are device-layout scratch arrays.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_op_vertex(Dev d, int op, const double *x, double *y) {
    const int tile = xcd_tile(blockIdx.x, d.n_vtiles);
    if (tile >= d.n_vtiles) return;
    const double ih = 1.0 / d.h;
    for (int e = threadIdx.x; e < TILE_ELEMS; e += BLOCK) {
        const int v = tile * d.VT + (e >> d.tp_shift), t = e & (d.TP - 1);
        if (v >= d.V) continue;
        const int iv = idxV(d, v, t);
        if (op == DOTS_OP_GRAD_TIME) {
            y[iv] = (t < d.ni) ? (x[iv + 1] - x[iv]) * ih : 0.0;
        } else if (op == DOTS_OP_DIV_TIME || op == DOTS_OP_TIME_AVG_ADJOINT) {
            if (t >= d.nl) { y[iv] = 0.0; continue; }
            const double a = (t < d.ni) ? x[iv] : 0.0, b = (t > 0) ? x[iv - 1] : 0.0;
            y[iv] = (op == DOTS_OP_DIV_TIME) ? (a - b) * ih : 0.5 * (a + b);
        } else if (op == DOTS_OP_DIV_SPACE) {
            if (t >= d.nl) { y[iv] = 0.0; continue; }
            double ds = 0.0;
            for (int j = d.cptr[v]; j < d.cptr[v + 1]; ++j) {
                const int fk = d.cidx[j], f = fk / 3, k = fk - 3 * f;
#pragma unroll
                for (int c = 0; c < 3; ++c) ds += d.hat[(f * 3 + k) * 3 + c] * x[idxF(d, f, c, t)];
            }
            y[iv] = -ds;
        }
    }
}
__global__ __launch_bounds__(BLOCK) void k_op_triangle(Dev d, int op, double scale, const double *x, double *y) {
    const int tile = xcd_tile(blockIdx.x, d.n_ftiles);
    if (tile >= d.n_ftiles) return;
    const double sB = scale * INV_SQRT3;
    for (int e = threadIdx.x; e < TILE_ELEMS; e += BLOCK) {
        const int row = tile * d.FT + (e >> d.tp_shift), t = e & (d.TP - 1);
        if (row >= 3 * d.F || t >= d.nl) continue;
        const int f = row / 3, c = row - 3 * f;
        if (op == DOTS_OP_GRAD_SPACE) {
            double gx = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) gx += d.hat[(f * 3 + k) * 3 + c] * x[idxV(d, d.tri[f * 3 + k], t)];
            y[idxF(d, f, c, t)] = gx;
        } else if (op == DOTS_OP_DECOUPLE) {
            const double b = sB * x[idxF(d, f, c, t)];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (t < d.ni) y[idxM(d, f * 3 + k, 0, c, t)] = b;
                if (t > 0) y[idxM(d, f * 3 + k, 1, c, t - 1)] = b;
            }
        } else if (op == DOTS_OP_DECOUPLE_ADJOINT) {
            y[idxF(d, f, c, t)] = sB * dec_adjoint_at(d, x, f, c, t);
        }
    }
}

int launch_operator(Ctx *c, int op, double scale, const double *in, double *out) {
    if (c->d.slab) { set_error("the standalone operators work on whole arrays: not available on a time slab"); return DOTS_ERR_STATE; }
    switch (op) {
        case DOTS_OP_GRAD_TIME:
        case DOTS_OP_DIV_TIME:
        case DOTS_OP_TIME_AVG_ADJOINT:
        case DOTS_OP_DIV_SPACE:
            hipLaunchKernelGGL(k_op_vertex, dim3(xcd_grid(c->d.n_vtiles)), dim3(BLOCK), 0, c->stream, c->d, op, in, out);
            break;
        case DOTS_OP_GRAD_SPACE:
        case DOTS_OP_DECOUPLE:
        case DOTS_OP_DECOUPLE_ADJOINT:
            hipLaunchKernelGGL(k_op_triangle, dim3(xcd_grid(c->d.n_ftiles)), dim3(BLOCK), 0, c->stream, c->d, op, scale, in, out);
            break;
        default:
            set_error("unknown operator");
            return DOTS_ERR_ARGUMENT;
    }
    DOTS_HIP(hipGetLastError());
    return 0;
}

// The runtime prepares a kernel on its first use (several hundred microseconds each): do that for the kernels of an iteration when
// the context is created, not inside the first iterations that happen to use them.
void preload_alm_kernels() {
    const void *fns[] = {
        (const void *)k_rhs<false>, (const void *)k_rhs<true>, (const void *)k_rhs_modes, (const void *)k_rhs_modes2<false>, (const void *)k_rhs_modes2<true>,
        (const void *)k_rhs_modes_mfma<false>, (const void *)k_rhs_modes_mfma<true>, (const void *)k_rhs_modes_mfma<false, true>, (const void *)k_rhs_modes2<false, true>,
        (const void *)k_rhs_modes2_deep<8>, (const void *)k_rhs_modes2_deep<16>, (const void *)k_rhs_modes2_deep<32>,
        (const void *)k_soc_projection<true>, (const void *)k_soc_projection<false>, (const void *)k_soc_projection<true, true>,
        (const void *)k_q_lambda_mult_triangle<0>, (const void *)k_q_lambda_mult_triangle<1>, (const void *)k_q_lambda_mult_triangle<2>,
        (const void *)k_q_lambda_mult_triangle<0, true>,
        (const void *)k_q_lambda_mult_triangle2<0>, (const void *)k_q_lambda_mult_triangle2<1>, (const void *)k_q_lambda_mult_triangle2<2>,
        (const void *)k_q_lambda_mult_carry<1>, (const void *)k_q_lambda_mult_carry<2>, (const void *)k_q_lambda_mult_carry<1, true>,
        (const void *)k_q_lambda_mult_carry<1, false, true>, (const void *)k_q_lambda_mult_carry<2, false, true>, (const void *)k_q_lambda_mult_carry<1, true, true>,
        (const void *)k_q_lambda_mult_carry<2, true, false>, (const void *)k_q_lambda_mult_carry<2, true, true>, (const void *)k_rebuild_zmid,
        (const void *)k_q_lambda_mult_carry<2, false, false, true>, (const void *)k_q_lambda_mult_carry<2, false, true, true>,
        (const void *)k_q_lambda_mult_carry<2, true, false, true>, (const void *)k_q_lambda_mult_carry<2, true, true, true>,

        (const void *)k_divide_five, (const void *)k_scale, (const void *)k_divide, (const void *)k_rebuild_mu, (const void *)k_rebuild_E,
    };
    hipFuncAttributes a;
    for (const void *f : fns) (void)hipFuncGetAttributes(&a, f);
    (void)hipGetLastError();
}

}  // namespace dots

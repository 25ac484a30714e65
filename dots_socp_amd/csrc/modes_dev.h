// Device bodies, LDS sizes and tile shapes of the time-mode transforms  y = Q^T x (time -> modes)  and  y = Q x (modes -> time).
// Included by kernels_modes.hip (the transform launches) and kernels_alm.hip (k_rhs_modes*, which transform the tile they have just
// formed, and the transform workgroups that ride in k_soc_projection).  Which pitch takes which form is decided by the predicates
// of dots_dev.h (time_modes_tile_ok, time_modes_mfma_ok, time_modes_fast_ok), which the other files' rules are built from.
#pragma once

#include "dots_dev.h"

namespace dots {

// The time-mode transforms stage a tile of rows and Q (in chunks of <= 32 KB) in LDS (k_time_modes_tile, k_rhs_modes)
// T + 1 in (256, 1024] (pitch 512 / 1024, one GPU, direct solver): k_time_modes_wide, Q staged in LDS one k-slice at a time
inline bool time_modes_wide_ok(const Dev &d) { return (d.TP == 512 || d.TP == 1024) && d.Qpad != nullptr && d.QpadT != nullptr; }
inline int time_modes_chunk(const Dev &d) { return (4096 / d.TP) < (d.T + 1) ? (4096 / d.TP) : (d.T + 1); }    // rows of Q per chunk
inline size_t time_modes_tile_lds(const Dev &d) { return sizeof(double) * ((size_t)time_modes_chunk(d) * d.TP + (size_t)d.VT * (d.TP + 1)); }
// pitch 8, 16 or 32 (all of Q is one chunk): the transforms' form with the pitch as a template argument (modes_from_tile_fast),
// tile rows at an even pitch
constexpr int fast_tile_pitch(int TPC) { return TPC + 2; }
inline size_t time_modes_fast_lds(const Dev &d) { return sizeof(double) * ((size_t)d.TP * d.TP + (size_t)d.VT * fast_tile_pitch(d.TP)); }

#ifdef __HIPCC__
// `elems` = rows * TP elements of a tile into xs ([rows][TP + 1]: rows padded by one double so that the rows a wavefront broadcasts
// sit in different banks), row vl = vertex v0 + vl, zero past V and past T + 1.  load(v, t): where an element comes from -- a small
// struct that carries its pointers (a lambda that captured the kernel's Dev by reference could cost the compiler their alias
// information).  No barrier: the caller's next one (modes_from_tile's first) completes the tile.
template <int NB, class Load>
__device__ __forceinline__ void stage_tile(const Dev &d, double *xs, int elems, int v0, const Load &load) {
    const int n = d.T + 1, TP = d.TP, TPp = TP + 1;
    for (int e = threadIdx.x; e < elems; e += NB) {
        const int vl = e >> d.tp_shift, t = e & (TP - 1);
        xs[vl * TPp + t] = (v0 + vl < d.V && t < n) ? load(v0 + vl, t) : 0.0;
    }
}
// the rows of a node array at the pitch 1 << shift
struct NodeRows {
    const double *__restrict__ x;
    int shift;
    __device__ __forceinline__ double operator()(int v, int t) const { return x[(v << shift) + t]; }
};

// The same product on the matrix cores (T + 1 >= 64): one v_mfma_f64_16x16x4_f64 per 16 x 16 output tile and 4
// values of i.  xs holds MROWS = 32 rows ([32][TP + 1], zero padded); wavefront w of the workgroup's NW takes the
// (row tile, column tile) pairs w, w + NW, ...  Operand layout of the instruction (lane l), measured on gfx950
// (profiles/micro/mfma_f64_layout.hip): A[i = l % 16][k = l / 16], B[k = l / 16][j = l % 16],
// D[i = l / 16 + 4 r][j = l % 16] in the r-th accumulator register.
// Qe = zero-padded Q (time -> modes) or Q^T (modes -> time), [TP][TP] row-major: no bounds checks in the loop.
typedef double mfma_f64x4 __attribute__((ext_vector_type(4)));
constexpr int TM_ROWS = 32;
template <int NW>
__device__ __forceinline__ void modes_from_tile_mfma(const Dev &d, const double *__restrict__ Qe, const double *xs, int v0, double *__restrict__ y) {
    const int n = d.T + 1, TP = d.TP, TPp = TP + 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int n_jt = TP >> 4;                            // column tiles of 16
    for (int tile = w; tile < 2 * n_jt; tile += NW) {
        const int jt = tile % n_jt, vt = tile / n_jt;
        mfma_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        const double *__restrict__ bq = Qe + (int64_t)lk * TP + jt * 16 + li;
        const double *a = xs + (vt * 16 + li) * TPp + lk;
        for (int k0 = 0; k0 < TP; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[k0], bq[(int64_t)k0 * TP], acc, 0, 0, 0);
        const int j = jt * 16 + li;
        if (j < n) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int v = v0 + vt * 16 + lk + 4 * r;
                if (v < d.V) y[idxV(d, v, j)] = acc[r];
            }
        }
    }
}

// y[v0 + vl][j] = sum_i Qeff[i][j] xs[vl][i] for the tile staged in xs ([VT][TP + 1], zero padded), with
// Qeff[i][j] = Q[i][j] (FWD: time -> modes) or Q[j][i] (modes -> time), staged through Qs in chunks of IC rows.
// A thread computes up to four outputs that share their Q column.  All threads of the workgroup must call it.
// Only the outputs j in [j0, j0 + jn) are stored, at y[(v << out_shift) + (j - j0)]  (defaults: all of them, pitch TP).
// rows [i0, i0 + ic) of Qeff into Qs.  A caller may stage the first chunk itself BEFORE its own loads of the tile (staged0):
// the Q loads then overlap them instead of adding a memory round trip behind the first barrier.
template <bool FWD, int NB = BLOCK>
__device__ __forceinline__ void stage_q_chunk(const Dev &d, const double *Q, double *Qs, int i0, int ic) {
    const int n = d.T + 1, TP = d.TP;
    for (int e = threadIdx.x; e < ic * TP; e += NB) {
        const int i = i0 + (e >> d.tp_shift), jj = e & (TP - 1);
        Qs[e] = jj < n ? (FWD ? Q[i * n + jj] : Q[jj * n + i]) : 0.0;
    }
}
template <bool FWD, int NB = BLOCK>
__device__ __forceinline__ void modes_from_tile(const Dev &d, const double *Q, const double *xs, double *Qs, int IC, int v0, double *__restrict__ y,
                                                int out_shift = -1, int j0 = 0, int jn = 1 << 30, bool staged0 = false) {
    if (out_shift < 0) out_shift = d.tp_shift;
    const int n = d.T + 1, TP = d.TP, TPp = TP + 1, tid = threadIdx.x;
    const int j = tid & (TP - 1), g = tid >> d.tp_shift, G = NB >> d.tp_shift;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i0 = 0; i0 < n; i0 += IC) {
        const int ic = min(IC, n - i0);
        if (!(staged0 && i0 == 0)) {
            __syncthreads();      // the previous chunk (or the caller's staging of xs) is complete
            stage_q_chunk<FWD, NB>(d, Q, Qs, i0, ic);
        }
        __syncthreads();
        if (j < n && g < d.VT) {
            const double *x0 = xs + g * TPp + i0;
            for (int i = 0; i < ic; ++i) {
                const double q = Qs[(i << d.tp_shift) + j];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (g + r * G < d.VT) acc[r] += q * x0[r * G * TPp + i];
            }
        }
    }
    if (j < n && j >= j0 && j - j0 < jn) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int vl = g + r * G;
            if (vl >= d.VT) continue;
            const int vv = v0 + vl;
            if (vv >= 0 && vv < d.V) y[((int64_t)vv << out_shift) + (j - j0)] = acc[r];
        }
    }
}
// A whole chunked tile transform, from the workgroup's dynamic LDS (time_modes_tile_lds: Qs [IC][TP], then xs [VT][TP + 1]): the tile
// of the vertices from v0 staged through `load`, then modes_from_tile with its arguments.  staged0: the first chunk of Q is staged
// ahead of the tile, so that one barrier serves both.  Returns the staged tile (complete: modes_from_tile has passed a barrier).
template <bool FWD, int NB = BLOCK, class Load>
__device__ __forceinline__ const double *modes_of_tile(const Dev &d, int IC, int v0, const Load &load, double *__restrict__ y, int out_shift = -1,
                                                       int j0 = 0, int jn = 1 << 30, bool staged0 = false) {
    extern __shared__ double tm_lds[];
    double *Qs = tm_lds, *xs = tm_lds + IC * d.TP;
    if (staged0) stage_q_chunk<FWD, NB>(d, d.Q, Qs, 0, min(IC, d.T + 1));      // (as compiled, two round trips: Q is waited for and written before the tile's loads are issued)
    stage_tile<NB>(d, xs, TILE_ELEMS, v0, load);
    modes_from_tile<FWD, NB>(d, d.Q, xs, Qs, IC, v0, y, out_shift, j0, jn, staged0);
    return xs;
}

// The same product for a pitch known at compile time (TPC = 8, 16 or 32: all of Q is one chunk; whole tile, every output stored at
// pitch TPC).  The loop above waits for one LDS read per term; here the loops are unrolled over a column of Q held in registers and
// the rows of the tile read in 16-byte words, so that the reads go out well ahead of their use (as compiled: a dozen in flight before
// the first counted wait): xs is [VT][TPC + 2] (an even pitch keeps the rows aligned; the rows one wavefront broadcasts still start in
// different banks), Qs is [TPC][TPC], zero beyond T.
// Output for output the arithmetic above: acc = acc + q * x for i = 0 .. T in that order, nothing added beyond T.
// A thread's outputs g, g + G, ... (TILE_ELEMS / NB of them) are all rows of the tile: no bound on vl.
// Q of the chunk as this thread stages it, loaded (addresses clamped, nothing branches) so that the caller's own loads join the
// same round trip, and written to Qs once those are issued
template <bool FWD, int NB, int TPC>
struct QStage {
    static constexpr int N = (TPC * TPC + NB - 1) / NB;
    double v[N];
    __device__ __forceinline__ void load(const Dev &d, const double *__restrict__ Q) {
        const int n = d.T + 1;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int e = threadIdx.x + k * NB, i = (e / TPC) & (TPC - 1), jj = e & (TPC - 1);
            const int ic = min(i, n - 1), jc = min(jj, n - 1);
            const double q = FWD ? Q[ic * n + jc] : Q[jc * n + ic];
            v[k] = ((i < n) & (jj < n)) ? q : 0.0;      // (&, not &&: a branch here would put the load, and a wait for it, behind the branch)
        }
    }
    __device__ __forceinline__ void store(double *Qs) const {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int e = threadIdx.x + k * NB;
            if (TPC * TPC % NB == 0 || e < TPC * TPC) Qs[e] = v[k];
        }
    }
};
template <int NB, int TPC>
__device__ __forceinline__ void modes_from_tile_fast(const Dev &d, const double *xs, const double *Qs, int v0, double *__restrict__ y) {
    constexpr int G = NB / TPC, R = TILE_ELEMS / NB, XP = fast_tile_pitch(TPC);
    const int n = d.T + 1, j = threadIdx.x & (TPC - 1), g = threadIdx.x / TPC;
    double q[TPC];
#pragma unroll
    for (int i = 0; i < TPC; ++i) q[i] = Qs[i * TPC + j];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int vl = g + r * G;
        const dots_d2v *x2 = reinterpret_cast<const dots_d2v *>(xs + vl * XP);
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < TPC; i += 2) {
            const dots_d2v x = x2[i >> 1];
            const double s0 = acc + q[i] * x.x;      // (T + 1 > TPC / 2 above a pitch of 8: the first half is always added)
            acc = (TPC > 8 && i < TPC / 2) || i < n ? s0 : acc;
            const double s1 = acc + q[i + 1] * x.y;
            acc = (TPC > 8 && i + 1 < TPC / 2) || i + 1 < n ? s1 : acc;
        }
        const int vv = v0 + vl;
        if (j < n && vv < d.V) y[((int64_t)vv << d.tp_shift) + j] = acc;
    }
}
#endif

}  // namespace dots

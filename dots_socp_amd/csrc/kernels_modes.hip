// The time-mode transforms around step 1's solve: with the orthonormal time eigen-basis Q (DCT-II),
//     FWD  y[v][a] = sum_t Q[t][a] x[v][t]   (time -> modes, the right-hand side and the PCG's warm start)
//     INV  y[v][t] = sum_a Q[t][a] x[v][a]   (modes -> time, phi from the mode-space solution)
// Every kernel that only transforms lives here, with the two ladders that choose among them (modes_forward, modes_inverse; which
// kernel serves which pitch and caller is written out in DESIGN.md, section 5) and the two launches of a time-slab context.  The bodies
// they share with the kernels that transform a tile in passing (k_rhs_modes*, k_soc_projection in kernels_alm.hip) are in modes_dev.h.
#include "modes_dev.h"

namespace dots {

// The forward transform one output per thread, straight from memory: the PCG's (it also emits the partial sums of column 0, the
// mean removal of the singular mode), and the direct solver's where no tiled form applies.
__global__ __launch_bounds__(BLOCK) void k_time_modes(Dev d, const double *__restrict__ x, double *__restrict__ y, int emit_col0) {
    __shared__ double lds[4];
    const int tile = xcd_tile(blockIdx.x, d.n_vtiles);
    const int n = d.T + 1;
    double part[1] = {0.0};
    if (tile < d.n_vtiles) {
        for (int e = threadIdx.x; e < TILE_ELEMS; e += BLOCK) {
            const int v = tile * d.VT + (e >> d.tp_shift), j = e & (d.TP - 1);
            if (v >= d.V || j >= n) continue;
            const double *row = x + idxV(d, v, 0);
            double s = 0.0;
            for (int i = 0; i < n; ++i) s += d.Q[i * n + j] * row[i];
            y[idxV(d, v, j)] = s;
            if (j == 0) part[0] += s;
        }
    }
    if (emit_col0) {
        block_sum<1>(part, lds);
        if (threadIdx.x == 0) d.partials[blockIdx.x] = part[0];
    }
}

// The transform with the tile of x and Q (in chunks) staged in LDS (modes_of_tile): every x row and every Q entry is read
// from memory once per workgroup instead of once per output; a thread computes four outputs that share their Q column.
// The first Q chunk is staged ahead of the tile: one barrier for both.
// NB = 1024 (one output per thread) where the launch is latency-bound: the inverse transform after the direct solve.
template <bool FWD, int NB = BLOCK>
__global__ __launch_bounds__(NB) void k_time_modes_tile(Dev d, const double *__restrict__ x, double *__restrict__ y, int IC) {
    const int tile = xcd_tile(blockIdx.x, d.n_vtiles);
    if (tile >= d.n_vtiles) return;
    modes_of_tile<FWD, NB>(d, IC, tile * d.VT, NodeRows{x, d.tp_shift}, y, -1, 0, 1 << 30, true);
}

// The same launch for a pitch of TPC = 8, 16 or 32 (modes_from_tile_fast): Q and the tile are loaded before either is
// written to LDS -- one round trip -- and the transform waits once for its column of Q instead of once per term.
template <bool FWD, int NB, int TPC>
__global__ __launch_bounds__(NB) void k_time_modes_tile_fast(Dev d, const double *__restrict__ x, double *__restrict__ y) {
    extern __shared__ dots_d2v tm_lds_fast[];
    constexpr int R = TILE_ELEMS / NB, XP = fast_tile_pitch(TPC);
    double *Qs = reinterpret_cast<double *>(tm_lds_fast);      // [TPC][TPC]
    double *xs = Qs + TPC * TPC;                                // [VT][XP]
    const int n = d.T + 1;
    const int tile = xcd_tile(blockIdx.x, d.n_vtiles);
    if (tile >= d.n_vtiles) return;
    const int v0 = tile * d.VT;
    QStage<FWD, NB, TPC> qs;
    qs.load(d, d.Q);
    double xv[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int e = threadIdx.x + k * NB, vl = e / TPC, t = e & (TPC - 1);
        const double v = x[idxV(d, min(v0 + vl, d.V - 1), t)];
        xv[k] = ((v0 + vl < d.V) & (t < n)) ? v : 0.0;
    }
    qs.store(Qs);
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int e = threadIdx.x + k * NB;
        xs[(e / TPC) * XP + (e & (TPC - 1))] = xv[k];
    }
    __syncthreads();
    modes_from_tile_fast<NB, TPC>(d, xs, Qs, v0, y);
}

// The transform as a GEMM on the matrix cores (T + 1 >= 64; modes_from_tile_mfma): a workgroup
// stages the rows of 32 vertices in LDS, its four wavefronts split the 16 x 16 output tiles.
__global__ __launch_bounds__(BLOCK) void k_time_modes_mfma(Dev d, const double *__restrict__ Qe, const double *__restrict__ x, double *__restrict__ y) {
    extern __shared__ double xs_m[];                    // [TM_ROWS][TP + 1]
    const int v0 = blockIdx.x * TM_ROWS;
    stage_tile<BLOCK>(d, xs_m, TM_ROWS * d.TP, v0, NodeRows{x, d.tp_shift});
    __syncthreads();
    modes_from_tile_mfma<BLOCK / 64>(d, Qe, xs_m, v0, y);
}

// The transform at pitch 512 / 1024 (T + 1 in (256, 1024]): Q of 2 / 8 MB does not fit in LDS, nor does a tile of rows with
// all their columns beside it.  A workgroup of TPC threads owns TM_ROWS = 32 vertices and ALL their TPC outputs; wavefront w
// owns the columns [64 w, 64 w + 64): 2 row tiles x 4 column tiles of 16 x 16, 8 accumulators of v_mfma_f64_16x16x4_f64
// (operand layout of modes_from_tile_mfma).  The k axis runs in slices of KS: per slice the workgroup stages KS rows of the
// zero-padded Qe and the KS columns of its 32 rows (zero past T + 1) in LDS (36 KB), then every wavefront multiplies.  Each Qe entry
// staged serves 32 vertices; x is read once.  Fixed order of the k steps: deterministic.
// One body, three layouts of the mode side:
//   WIDE_FULL          both sides at the full pitch (the direct solver: k_time_modes_wide, Qe = Qpad forward, QpadT back)
//   WIDE_TO_WINDOWS    a WINDOWED context (dots_pcg_windows: no factor), forward: x in time space at the full pitch, y compact -- mode a of
//                      vertex v lives at window_at: window k = modes [256 k, 256 k + 256) is the [V][256] array the PCG's pitch-256 view
//                      indexes.  A wavefront's 64 columns lie in one window.  Columns past T + 1 are not stored: a window without a live
//                      mode is never written.  emit_col0: the workgroup's sum of mode 0 over its 32 vertices goes to
//                      d.partials[blockIdx.x], summed in vertex order (k_cg_bmean)
//   WIDE_FROM_WINDOWS  the same context, back: x in windows, y in time space at the full pitch (Qe = QpadT)
// The windowed layouts let a wavefront without a live column skip the multiplications (it only helps to stage).
enum WideLayout { WIDE_FULL, WIDE_TO_WINDOWS, WIDE_FROM_WINDOWS };
__device__ __forceinline__ int64_t window_at(int64_t wstride, int v, int a) {      // wstride: doubles per window
    return (a >> PCG_WINDOW_SHIFT) * wstride + ((int64_t)v << PCG_WINDOW_SHIFT) + (a & (PCG_WINDOW - 1));
}
template <int TPC, WideLayout L>
__device__ __forceinline__ void modes_wide(const Dev &d, const double *__restrict__ Qe, const double *__restrict__ x, double *__restrict__ y, int emit_col0) {
    constexpr int KS = 4096 / TPC;              // rows of Qe per slice: 32 KB of LDS (with x: < 64 KB, no opt-in needed)
    constexpr int QLD = TPC + 16;               // (16 doubles of padding: the four k rows an instruction reads sit in different banks)
    constexpr int XLD = KS + 1;
    extern __shared__ double tw_lds[];
    double *Qs = tw_lds;                        // [KS][QLD]
    double *xs = tw_lds + KS * QLD;             // [TM_ROWS][XLD]
    const int n = d.T + 1, tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int v0 = blockIdx.x * TM_ROWS;
    const int64_t wstride = (int64_t)d.V << PCG_WINDOW_SHIFT;
    bool live = true;                           // this wavefront stores at least one column
    if constexpr (L != WIDE_FULL) live = w * 64 < n;
    mfma_f64x4 acc[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = mfma_f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < n; k0 += KS) {
        if (k0 > 0) __syncthreads();            // every wavefront is done with the slice before
#pragma unroll
        for (int i = 0; i < KS; ++i) Qs[i * QLD + tid] = Qe[(int64_t)(k0 + i) * TPC + tid];      // rows past T + 1 are zero
        for (int e = tid; e < TM_ROWS * KS; e += TPC) {
            const int vl = e / KS, kk = e % KS, v = v0 + vl, a = k0 + kk;
            double xv = 0.0;
            if (v < d.V && a < n) xv = L == WIDE_FROM_WINDOWS ? x[window_at(wstride, v, a)] : x[idxV(d, v, a)];
            xs[vl * XLD + kk] = xv;
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int kk = 0; kk < KS; kk += 4) {
                const double a0 = xs[li * XLD + kk + lk], a1 = xs[(16 + li) * XLD + kk + lk];
                const double *bq = Qs + (kk + lk) * QLD + w * 64 + li;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const double b = bq[ct * 16];
                    acc[0][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][ct], 0, 0, 0);
                    acc[1][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][ct], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int j = w * 64 + ct * 16 + li;
        if (j >= n) continue;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int v = v0 + rt * 16 + lk + 4 * r;
                if (v >= d.V) continue;
                y[L == WIDE_TO_WINDOWS ? window_at(wstride, v, j) : (int64_t)idxV(d, v, j)] = acc[rt][ct][r];
            }
    }
    if constexpr (L == WIDE_TO_WINDOWS) {
        if (emit_col0) {             // mode 0 of the 32 vertices sits in wavefront 0, column tile 0, lanes 0, 16, 32, 48 (rows past V are zero)
            __syncthreads();         // every wavefront is done with the last slice: xs is free
            if (w == 0 && li == 0) {
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) xs[rt * 16 + lk + 4 * r] = acc[rt][0][r];
            }
            __syncthreads();
            if (tid == 0) {
                double s = 0.0;
                for (int i = 0; i < TM_ROWS; ++i) s += xs[i];
                d.partials[blockIdx.x] = s;
            }
        }
    }
}
template <int TPC>
__global__ __launch_bounds__(TPC) void k_time_modes_wide(Dev d, const double *__restrict__ Qe, const double *__restrict__ x, double *__restrict__ y) {
    modes_wide<TPC, WIDE_FULL>(d, Qe, x, y, 0);
}
template <int TPC, bool FWD>
__global__ __launch_bounds__(TPC) void k_time_modes_windows(Dev d, const double *__restrict__ Qe, const double *__restrict__ x, double *__restrict__ y,
                                                            int emit_col0) {
    modes_wide<TPC, FWD ? WIDE_TO_WINDOWS : WIDE_FROM_WINDOWS>(d, Qe, x, y, emit_col0);
}
template <int TPC>
static size_t time_modes_wide_lds() { return sizeof(double) * ((size_t)(4096 / TPC) * (TPC + 16) + (size_t)TM_ROWS * (4096 / TPC + 1)); }
int modes_windows_sums(const Dev &d) { return (d.V + TM_ROWS - 1) / TM_ROWS; }      // one workgroup per TM_ROWS vertices, one sum each
static void launch_time_modes_wide(Ctx *c, WideLayout layout, const double *Qe, const double *x, double *y, int emit_col0 = 0) {
    const Dev &d = c->d;
    const dim3 grid((d.V + TM_ROWS - 1) / TM_ROWS);
    with_constant<512, 1024>(d.TP, [&](auto TPC) {
        const size_t lds = time_modes_wide_lds<TPC>();
        if (layout == WIDE_FULL) hipLaunchKernelGGL(k_time_modes_wide<TPC>, grid, dim3(TPC), lds, c->stream, d, Qe, x, y);
        else if (layout == WIDE_TO_WINDOWS) hipLaunchKernelGGL((k_time_modes_windows<TPC, true>), grid, dim3(TPC), lds, c->stream, d, Qe, x, y, emit_col0);
        else hipLaunchKernelGGL((k_time_modes_windows<TPC, false>), grid, dim3(TPC), lds, c->stream, d, Qe, x, y, emit_col0);
    });
}

// ---- transforms of a time-slab context (multi-GPU) -------------------------------------------------------------
// Both read an all-gathered buffer of R chunks: chunk p holds [V][pitch] doubles with `stride` live columns, column j of
// chunk p = global index p * stride + j (time node for the right-hand side, time mode for the solution).
struct Gathered {
    const double *base;
    int64_t chunk;       // doubles per rank
    int shift;           // log2 of the pitch inside a chunk
    int stride;          // live columns per chunk
    __device__ __forceinline__ double operator()(int v, int i) const {
        const int p = i / stride, j = i - p * stride;
        return base[p * chunk + ((int64_t)v << shift) + j];
    }
};
constexpr int FWD_SUB_GRID = 1024;      // grid-stride workgroups of k_time_modes_fwd_sub = the column-0 sums it leaves

// Forward transform restricted to the modes [a0, a0 + g.cg_ncol) this context solves, from the gathered right-hand
// side:  y[v][j] = sum_t Q[t][a0 + j] b[v][t]  (pitch of the PCG view).  Emits the column-0 partial sums (mean removal
// of the singular mode) when asked to.   dt: the global-time view (T, Q).
__global__ __launch_bounds__(BLOCK) void k_time_modes_fwd_sub(Dev dt, Dev g, int a0, Gathered x, double *__restrict__ y, int emit_col0) {
    __shared__ double lds[4];
    const int n = dt.T + 1, nloc = g.cg_ncol;
    double part[1] = {0.0};
    const int64_t total = (int64_t)dt.V << g.tp_shift;
    for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * BLOCK) {
        const int v = (int)(e >> g.tp_shift), j = (int)(e & (g.TP - 1));
        if (j >= nloc) continue;
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += dt.Q[i * n + a0 + j] * x(v, i);
        y[idxV(g, v, j)] = s;
        if (emit_col0 && j == 0) part[0] += s;
    }
    if (emit_col0) {
        block_sum<1>(part, lds);
        if (threadIdx.x == 0) dt.partials[blockIdx.x] = part[0];
    }
}

// Tiled forms (modes_of_tile; dt = the global-time view: pitch >= T + 1).  Forward: stores only
// this context's modes with the PCG view's pitch.
__global__ __launch_bounds__(BLOCK) void k_time_modes_fwd_sub_tile(Dev dt, int a0, int nloc, int out_shift, Gathered x, double *__restrict__ y, int IC) {
    const int tile = xcd_tile(blockIdx.x, dt.n_vtiles);
    if (tile >= dt.n_vtiles) return;
    modes_of_tile<true>(dt, IC, tile * dt.VT, x, y, out_shift, a0, nloc);
}

// Inverse: phi of this slab's nodes [t0, t0 + nl) (pitch of the slab, 1 << out_shift) from the gathered mode-space
// solution, and phi at node t0 + nl (the next slab's first node) into phi_hi: the same sum, in the same order, as the
// owner of that node forms -- no exchange of phi is ever needed.
__global__ __launch_bounds__(BLOCK) void k_time_modes_inv_gathered_tile(Dev dt, Gathered x, double *__restrict__ y, int out_shift, int t0, int nl,
                                                                        double *__restrict__ phi_hi, int IC) {
    const int n = dt.T + 1, TPp = dt.TP + 1;
    const int tile = xcd_tile(blockIdx.x, dt.n_vtiles);
    if (tile >= dt.n_vtiles) return;
    const int v0 = tile * dt.VT;
    const double *xs = modes_of_tile<false>(dt, IC, v0, x, y, out_shift, t0, nl);
    const int th = t0 + nl;      // first node of the next slab
    if (th < n && (int)threadIdx.x < dt.VT && v0 + (int)threadIdx.x < dt.V) {
        const double *x0 = xs + threadIdx.x * TPp;
        double acc = 0.0;
        for (int a = 0; a < n; ++a) acc += dt.Q[th * n + a] * x0[a];
        phi_hi[v0 + threadIdx.x] = acc;
    }
}

// ---- the ladders ---------------------------------------------------------------------------------------------------
// The time transforms around the solve of one GPU: b^ = Q^T b of `in` into `out` (mode space), and phi = Q x^ back.  `direct`: the
// sweeps solve (no warm start, no mean removal); the kernels are chosen as step 1 chooses them (cg_solve, dots_laplacian_solve_many,
// dots_step_many).  col0_sums (the PCG's forms only): modes_forward_sums(c) partial sums of mode 0 go to Dev::partials.
void modes_forward(Ctx *c, const double *in, double *out, bool direct, bool col0_sums) {
    const Dev &d = c->d;
    const int gt = xcd_grid(d.n_vtiles);
    if (!direct && pcg_windowed(c))
        launch_time_modes_wide(c, WIDE_TO_WINDOWS, d.Qpad, in, out, col0_sums ? 1 : 0);      // `out` in compact windows
    else if (direct && time_modes_wide_ok(d))
        launch_time_modes_wide(c, WIDE_FULL, d.Qpad, in, out);
    else if (direct && time_modes_tile_ok(d))
        hipLaunchKernelGGL((k_time_modes_tile<true>), dim3(gt), dim3(BLOCK), time_modes_tile_lds(d), c->stream, d, in, out, time_modes_chunk(d));
    else
        hipLaunchKernelGGL(k_time_modes, dim3(gt), dim3(BLOCK), 0, c->stream, d, in, out, col0_sums ? 1 : 0);
}
int modes_forward_sums(const Ctx *c) {
    if (c->shard_count > 0) return c->shard_begin == 0 ? FWD_SUB_GRID : 0;      // (time slab: the rank that owns mode 0)
    return pcg_windowed(c) ? modes_windows_sums(c->d) : xcd_grid(c->d.n_vtiles);
}
int modes_inverse(Ctx *c, const double *x, double *phi, bool direct) {
    const Dev &d = c->d;
    const int gt = xcd_grid(d.n_vtiles);
    c->carried.deep_path &= ~DEEP_PATH_INVERSE;
    if (!direct && pcg_windowed(c))
        launch_time_modes_wide(c, WIDE_FROM_WINDOWS, d.QpadT, x, phi);      // `x` in compact windows
    else if (direct && time_modes_wide_ok(d))
        launch_time_modes_wide(c, WIDE_FULL, d.QpadT, x, phi);
    else if (time_modes_mfma_ok(d))
        hipLaunchKernelGGL(k_time_modes_mfma, dim3((d.V + TM_ROWS - 1) / TM_ROWS), dim3(BLOCK), sizeof(double) * TM_ROWS * (d.TP + 1), c->stream, d, d.QpadT,
                           x, phi);
    else if (time_modes_tile_ok(d) && direct && d.n_vtiles <= 512 && deep_launch_wins(c, gt)) {      // ... with its reads in flight (pitch 8, 16, 32)
        with_constant<8, 16, 32>(d.TP, [&](auto TPC) {
            hipLaunchKernelGGL((k_time_modes_tile_fast<false, 1024, TPC>), dim3(gt), dim3(1024), time_modes_fast_lds(d), c->stream, d, x, phi);
        });
        c->carried.deep_path |= DEEP_PATH_INVERSE;
    }
    else if (time_modes_tile_ok(d) && direct && d.n_vtiles <= 512)      // small meshes, behind the sweeps: latency-bound, one output per thread (knot: 9.5 -> 6 us; no gain at 10^5 vertices)
        hipLaunchKernelGGL((k_time_modes_tile<false, 1024>), dim3(gt), dim3(1024), time_modes_tile_lds(d), c->stream, d, x, phi, time_modes_chunk(d));
    else if (time_modes_tile_ok(d))
        hipLaunchKernelGGL((k_time_modes_tile<false>), dim3(gt), dim3(BLOCK), time_modes_tile_lds(d), c->stream, d, x, phi, time_modes_chunk(d));
    else {      // more than 256 modes, neither sweeps nor windows: cg_solve refuses that solve before it launches anything
        set_error("inverse time transform: T + 1 > 256 needs the direct solver (dots_front_setup) or PCG windows (dots_pcg_windows)");
        return DOTS_ERR_STATE;
    }
    return 0;
}

// Time slab: the right-hand side of ALL nodes was all-gathered into slab.b_recv; this rank transforms the modes it solves, into the PCG view's cg_p0
void modes_forward_sharded(Ctx *c, bool direct) {
    const Dev &d = c->d;
    const Dev g = pcg_view(c), dt = time_view(c);
    const Gathered bg{c->slab.b_recv, c->slab_b_chunk, d.tp_shift, c->shard_stride};
    if (direct && time_modes_tile_ok(dt))     // no mean removal with the direct solver: the tiled transform
        hipLaunchKernelGGL(k_time_modes_fwd_sub_tile, dim3(xcd_grid(dt.n_vtiles)), dim3(BLOCK), time_modes_tile_lds(dt), c->stream, dt, c->shard_begin,
                           g.cg_ncol, g.tp_shift, bg, g.cg_p0, time_modes_chunk(dt));
    else
        hipLaunchKernelGGL(k_time_modes_fwd_sub, dim3(FWD_SUB_GRID), dim3(BLOCK), 0, c->stream, dt, g, c->shard_begin, bg, g.cg_p0, c->shard_begin == 0 ? 1 : 0);
}
// phi of this slab from the mode-space solutions of all ranks (slab.x_recv = [n_ranks][V][mode pitch])
int cg_finish_sharded(Ctx *c) {
    const Dev &d = c->d;
    const Dev dt = time_view(c);
    if (d.nl == 0) return 0;
    if (!time_modes_tile_ok(dt)) { set_error("time slabs need T + 1 <= 256"); return DOTS_ERR_STATE; }
    const Gathered xg{c->slab.x_recv, c->slab_x_chunk, d.tp_shift, c->shard_stride};
    hipLaunchKernelGGL(k_time_modes_inv_gathered_tile, dim3(xcd_grid(dt.n_vtiles)), dim3(BLOCK), time_modes_tile_lds(dt), c->stream, dt, xg, d.phi,
                       d.tp_shift, d.t0, d.nl, d.phi_hi, time_modes_chunk(dt));
    DOTS_HIP(hipGetLastError());
    return 0;
}

void preload_transform_kernels() {      // (see preload_alm_kernels)
    const void *fns[] = {(const void *)k_time_modes_tile<true, BLOCK>, (const void *)k_time_modes_tile<false, BLOCK>,
                         (const void *)k_time_modes_tile<false, 1024>, (const void *)k_time_modes_mfma,
                         (const void *)k_time_modes_tile_fast<false, 1024, 8>, (const void *)k_time_modes_tile_fast<false, 1024, 16>,
                         (const void *)k_time_modes_tile_fast<false, 1024, 32>, (const void *)k_time_modes,
                         (const void *)k_time_modes_wide<512>, (const void *)k_time_modes_wide<1024>,
                         (const void *)k_time_modes_windows<512, true>, (const void *)k_time_modes_windows<512, false>,
                         (const void *)k_time_modes_windows<1024, true>, (const void *)k_time_modes_windows<1024, false>};
    hipFuncAttributes a;
    for (const void *f : fns) (void)hipFuncGetAttributes(&a, f);
    (void)hipGetLastError();
}

}  // namespace dots

// Read-out of the transport (dots_readout): mu and E in the caller's numbering and the reference's layouts, scaled -- and, for mu,
// moved to the time-centred grid and summed per layer -- on the device, so that only what the plug-in boundary returns crosses to
// the host (dots_socp_amd/readout.py: read_out_host is the specification; solver_socp.py:397-405, utils/type.py:48-65,
// socp/solver_decorator.py:29-54 are what it replaces).
//
// A workgroup takes a run of NV consecutive rows in the CALLER's numbering (a vertex of mu; a (triangle, component) of E), gathers
// each one's device row (time fastest) with 16-byte loads, forms the values in registers -- x = factor * a, then y = x * w where
// weights are given: these operations in this order, the build has -ffp-contract=off, so the result is the host path's bit for
// bit -- and lays them down in LDS row by row.  Read back across the rows, a layer is one contiguous run out[l][v0 .. v0 + n) of
// the output, stored as aligned 16-byte words (a leading / trailing single where the run starts or ends on an odd element).
// The time axis is cut into chunks of at most 256 columns (one launch each): a chunk's layers are complete when its launch is,
// and can be copied while the next chunk is formed.
#include "dots_dev.h"

namespace dots {

struct ReadoutArgs {
    const double *src;       // device array [rows][TP]
    double *out;             // [layers][NR], the reference layout in the caller's numbering
    const int *inv;          // caller vertex / triangle -> device vertex / triangle, or null (same numbering)
    const double *w;         // [NR / rpe] second multiplier per caller vertex / triangle, or null
    const double *m0, *m1;   // [NR] first and last layer of the centred output
    double *part;            // [layers][2][n_wg] per-workgroup sums of the values / of the negative values, or null
    double factor;
    int NR, rpe;             // rows of a layer (V, or 3 F); rows per vertex / triangle (1 or 3)
    int T;                   // columns of src that hold values (intervals for mu, nodes for E)
    int layers;              // layers of the output: T, or T + 1 centred
    int centred;
    int tp_shift;
    int c0, CW;              // this launch forms the layers [c0, min(c0 + CW, layers))
    int NV;                  // rows per workgroup (even)
    int g_shift;             // log2 of the lanes that share a layer in the store phase
    int n_wg;
};

constexpr int READOUT_LDS = 8192;      // doubles of LDS a workgroup may use (64 KB)

// slot j of a row in LDS holds column c0 - 2 + j: the centred layer c0 reads column c0 - 1, and rows keep whole 16-byte pairs
__device__ __forceinline__ double readout_value(const ReadoutArgs &a, const double *xs, int SP, int v0, int e, int l) {
    const double *x = xs + e * SP + (l - a.c0 + 2);
    if (!a.centred) return x[0];
    if (l == 0) return a.m0[v0 + e];
    if (l == a.T) return a.m1[v0 + e];
    return 0.5 * (x[-1] + x[0]);
}

template <bool SUMS>
__device__ __forceinline__ void readout_body(const ReadoutArgs &a) {
    extern __shared__ double xs[];
    const int tid = threadIdx.x;
    const int SP = a.CW + 3;                              // (odd: neighbouring rows start on other banks)
    const int v0 = blockIdx.x * a.NV;
    const int n = min(a.NV, a.NR - v0);
    if (n <= 0) return;
    // ---- gather: LR lanes walk the column pairs of one row
    const int PP = (a.CW >> 1) + 1;                       // pairs per row, the leading pair (columns c0 - 2, c0 - 1) included
    const int p_first = (a.centred && a.c0 > 0) ? 0 : 1;
    const int lr_shift = min(6, 31 - __clz(a.CW >> 1));
    const int LR = 1 << lr_shift;
    for (int rr = tid >> lr_shift; rr < n; rr += BLOCK >> lr_shift) {
        const int R = v0 + rr;
        const int ent = a.rpe == 1 ? R : R / 3, k = R - ent * a.rpe;
        const int64_t drow = (int64_t)(a.inv ? a.inv[ent] : ent) * a.rpe + k;
        const double *row = a.src + (drow << a.tp_shift) + (a.c0 - 2);
        double *xr = xs + rr * SP;
        if (a.w) {
            const double w = a.w[ent];
            for (int p = p_first + (tid & (LR - 1)); p < PP; p += LR) {
                const D2 q = ld2(row + 2 * p);
                const double x0 = a.factor * q.v[0], x1 = a.factor * q.v[1];
                xr[2 * p] = x0 * w;
                xr[2 * p + 1] = x1 * w;
            }
        } else {
            for (int p = p_first + (tid & (LR - 1)); p < PP; p += LR) {
                const D2 q = ld2(row + 2 * p);
                xr[2 * p] = a.factor * q.v[0];
                xr[2 * p + 1] = a.factor * q.v[1];
            }
        }
    }
    __syncthreads();
    // ---- store: G lanes share a layer; a lane takes the aligned element pairs g, g + G, ... of the layer's run
    const int G = 1 << a.g_shift, g = tid & (G - 1);
    const int l_end = min(a.c0 + a.CW, a.layers);
    for (int l = a.c0 + (tid >> a.g_shift); l < l_end; l += BLOCK >> a.g_shift) {
        const int64_t base = (int64_t)l * a.NR + v0;
        const int odd = (int)(base & 1);                  // the run starts on the second half of a 16-byte word
        double *o = a.out + base;
        double s = 0.0, sneg = 0.0;
        for (int p = g; 2 * p - odd < n; p += G) {
            const int e0 = 2 * p - odd;
            const bool lo = e0 >= 0, hi = e0 + 1 < n;
            D2 y{{0.0, 0.0}};
            if (lo) y.v[0] = readout_value(a, xs, SP, v0, e0, l);
            if (hi) y.v[1] = readout_value(a, xs, SP, v0, e0 + 1, l);
            if (lo && hi) st2(o + e0, y);
            else if (lo) o[e0] = y.v[0];
            else if (hi) o[e0 + 1] = y.v[1];
            if (SUMS) {
                if (lo) { s += y.v[0]; sneg += y.v[0] < 0.0 ? y.v[0] : 0.0; }
                if (hi) { s += y.v[1]; sneg += y.v[1] < 0.0 ? y.v[1] : 0.0; }
            }
        }
        if (SUMS) {                                       // fixed order: the lane's own elements, then the lanes pairwise
            for (int m = G >> 1; m > 0; m >>= 1) {
                s += __shfl_xor(s, m, 64);
                sneg += __shfl_xor(sneg, m, 64);
            }
            if (g == 0) {
                a.part[((int64_t)l * 2) * a.n_wg + blockIdx.x] = s;
                a.part[((int64_t)l * 2 + 1) * a.n_wg + blockIdx.x] = sneg;
            }
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_readout_mu(ReadoutArgs a) {
    if (a.part) readout_body<true>(a);
    else readout_body<false>(a);
}
__global__ __launch_bounds__(BLOCK) void k_readout_E(ReadoutArgs a) { readout_body<false>(a); }

// second stage of the layer sums: workgroup = (layer, which sum), the workgroups' partial sums in a fixed order
__global__ __launch_bounds__(BLOCK) void k_readout_fold(const double *__restrict__ part, int n_wg, double *out) {
    __shared__ double lds[4];
    const double *__restrict__ p = part + (int64_t)blockIdx.x * n_wg;
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < n_wg; i += BLOCK) v[0] += p[i];
    block_sum<1>(v, lds);
    if (threadIdx.x == 0) {
        out[blockIdx.x] = v[0];
        __threadfence_system();      // (out is host memory the device writes itself; the caller waits for the stream)
    }
}

// rows per workgroup at chunk width CW: what 32 KB of LDS hold (64 KB from 128 columns on, where that is few rows), at most 256
static int readout_rows(int CW) {
    const int budget = CW >= 128 ? READOUT_LDS : READOUT_LDS / 2;
    int nv = budget / (CW + 3);
    nv = std::min(nv, 256) & ~1;
    return std::max(nv, 2);
}

// Enqueue the launches of one array on the context's stream: chunk k forms the layers [256 k, 256 k + 256) and is followed by
// ev[k] (if given).  is_E: E -> out [T + 1][F][3]; otherwise mu -> out [layers][V].  part: room for layers * 2 * n_wg doubles.
int launch_readout(Ctx *c, bool is_E, double *out, const int *inv, const double *w, const double *m0, const double *m1, int centred,
                   double factor, double *part, hipEvent_t *ev, int *n_chunks) {
    const Dev &d = c->d;
    ReadoutArgs a{};
    a.src = is_E ? d.E : d.mu;
    a.out = out;
    a.inv = inv;
    a.w = w;
    a.m0 = m0;
    a.m1 = m1;
    a.part = is_E ? nullptr : part;
    a.factor = factor;
    a.rpe = is_E ? 3 : 1;
    a.NR = is_E ? 3 * d.F : d.V;
    a.T = is_E ? d.T + 1 : d.T;
    a.centred = is_E ? 0 : centred;
    a.layers = a.T + (a.centred ? 1 : 0);
    a.tp_shift = d.tp_shift;
    a.CW = std::min(d.TP, 256);
    a.NV = readout_rows(a.CW);
    a.n_wg = (a.NR + a.NV - 1) / a.NV;
    int gs = 0;
    while ((1 << gs) < a.NV / 2 && gs < 6) ++gs;
    a.g_shift = gs;
    const size_t lds = sizeof(double) * (size_t)a.NV * (a.CW + 3);
    int k = 0;
    for (a.c0 = 0; a.c0 < a.layers; a.c0 += a.CW, ++k) {
        if (is_E) hipLaunchKernelGGL(k_readout_E, dim3(a.n_wg), dim3(BLOCK), lds, c->stream, a);
        else hipLaunchKernelGGL(k_readout_mu, dim3(a.n_wg), dim3(BLOCK), lds, c->stream, a);
        DOTS_HIP(hipGetLastError());
        if (ev) DOTS_HIP(hipEventRecord(ev[k], c->stream));
    }
    *n_chunks = k;
    return 0;
}
int readout_workgroups(const Ctx *c) {      // of a k_readout_mu launch: partial sums per layer
    const int nv = readout_rows(std::min(c->d.TP, 256));
    return (c->d.V + nv - 1) / nv;
}
void preload_readout_kernels() {
    const void *fns[] = {(const void *)k_readout_mu, (const void *)k_readout_E, (const void *)k_readout_fold};
    hipFuncAttributes a;
    for (const void *f : fns) (void)hipFuncGetAttributes(&a, f);
    (void)hipGetLastError();
}
int launch_readout_fold(Ctx *c, const double *part, int layers, int n_wg, double *out) {
    hipLaunchKernelGGL(k_readout_fold, dim3(2 * layers), dim3(BLOCK), 0, c->stream, part, n_wg, out);
    DOTS_HIP(hipGetLastError());
    return 0;
}

}  // namespace dots

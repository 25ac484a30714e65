// dots_restart (dots_api.hip): what a solve session runs on the device between two problems on one context.
//   k_restart_scale      DOTS_RESTART_WARM: the twelve state arrays times their recovery factors, in place, one launch
//   k_restart_boundary   norm_boundary's sum from end masses that are device memory, in two stages of fixed order
#include "dots_dev.h"

#include <algorithm>

namespace dots {

// The twelve arrays as one index space of 16-byte pairs (two time columns of one row: the pitch is even and >= 8, so a pair never
// leaves its row): end[k] = pairs of the arrays 0 .. k
struct RestartArrays {
    double *p[DOTS_N_ARRAYS];
    int64_t end[DOTS_N_ARRAYS];
    double f[DOTS_N_ARRAYS];
    int kind[DOTS_N_ARRAYS];      // array_kind
};

// One fp64 multiply per live element -- AlmSolver.recovered on the host is the same operation -- and zero in every column that
// k_convert<true> (the upload) writes as zero: past the nodes (kinds 0, 2) / the intervals (kind 1), and for a corner row of half s
// outside [s, T + s), the columns of the nodes its intervals are compared with.  ZERO (DOTS_RESTART_COLD): nothing is read, every
// element becomes +0.0 (a product with a factor 0 would keep a NaN and the sign of a negative value).
template <bool ZERO>
__global__ __launch_bounds__(BLOCK) void k_restart_scale(RestartArrays a, int tp_shift, int nl, int ni) {
    const int64_t total = a.end[DOTS_N_ARRAYS - 1];
    const int tmask = (1 << tp_shift) - 1;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * BLOCK) {
        int k = 0;
#pragma unroll
        for (int q = 0; q < DOTS_N_ARRAYS - 1; ++q) k += i >= a.end[q];
        const int64_t e = (i - (k ? a.end[k - 1] : 0)) * 2;      // first element of the pair in array k
        if (ZERO) {
            st2(a.p[k] + e, D2{{0.0, 0.0}});
            continue;
        }
        const int t = (int)(e & tmask), kind = a.kind[k];
        int lo = 0, hi = (kind == 1) ? ni : nl;
        if (kind == 3) {
            const int s = (int)(((e >> tp_shift) / 3) & 1);
            lo = s;
            hi = ni + s;
        }
        const double f = a.f[k];
        double *p = a.p[k] + e;
        D2 x = ld2(p);
        x.v[0] = (t >= lo && t < hi) ? x.v[0] * f : 0.0;
        x.v[1] = (t + 1 >= lo && t + 1 < hi) ? x.v[1] * f : 0.0;
        st2(p, x);
    }
}

// factor == nullptr: the twelve arrays are zeroed instead
int launch_restart_scale(Ctx *c, const double factor[4], double *bytes) {
    const Dev &d = c->d;
    if (d.slab || d.TP < 8) { set_error("restart: the in-place rescaling runs on one GPU (pitch >= 8)"); return DOTS_ERR_STATE; }
    const int group[DOTS_N_ARRAYS] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3};      // recorver_scaled_solution (solver_socp.py:397-405)
    RestartArrays a{};
    int64_t n = 0;
    for (int id = 0; id < DOTS_N_ARRAYS; ++id) {
        a.p[id] = c->arr(id);
        n += array_count_device(d, id) / 2;
        a.end[id] = n;
        a.f[id] = factor ? factor[group[id]] : 0.0;
        a.kind[id] = array_kind(id);
    }
    // memory-bound: enough workgroups to fill the chip, the rest of the index space by stride
    const int64_t want = (n + BLOCK - 1) / BLOCK;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, 2048));
    if (factor) hipLaunchKernelGGL(k_restart_scale<false>, dim3(grid), dim3(BLOCK), 0, c->stream, a, d.tp_shift, d.nl, d.ni);
    else hipLaunchKernelGGL(k_restart_scale<true>, dim3(grid), dim3(BLOCK), 0, c->stream, a, d.tp_shift, d.nl, d.ni);
    DOTS_HIP(hipGetLastError());
    if (bytes) *bytes = (factor ? 2.0 : 1.0) * 16.0 * (double)n;
    return 0;
}

// stage 1: workgroup b sums the vertices b * BLOCK + lane + j * gridDim.x * BLOCK, j ascending, then its lanes (block_sum);
// stage 2 (one workgroup): lane l sums the workgroups l, l + BLOCK, ... ascending, then the lanes.  The order depends on V alone.
__global__ __launch_bounds__(BLOCK) void k_restart_boundary(const double *__restrict__ mu0, const double *__restrict__ mu1, const double *__restrict__ mass,
                                                           int V, double *__restrict__ part) {
    __shared__ double lds[4];
    double s[1] = {0.0};
    for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * BLOCK) s[0] += (mu0[v] * mu0[v] + mu1[v] * mu1[v]) / mass[v];
    block_sum<1>(s, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}
__global__ __launch_bounds__(BLOCK) void k_restart_boundary_fold(const double *__restrict__ part, int n, double *__restrict__ out) {
    __shared__ double lds[4];
    double s[1] = {0.0};
    for (int b = threadIdx.x; b < n; b += BLOCK) s[0] += part[b];
    block_sum<1>(s, lds);
    if (threadIdx.x == 0) out[0] = s[0];
}

constexpr int RESTART_SUM_BLOCKS = 1024;      // (Dev::partials holds at least 4096 doubles)

int restart_boundary_sum(Ctx *c, const double *mu0, const double *mu1, double *out) {
    const Dev &d = c->d;
    const int grid = std::max(1, std::min((d.V + BLOCK - 1) / BLOCK, RESTART_SUM_BLOCKS));
    hipLaunchKernelGGL(k_restart_boundary, dim3(grid), dim3(BLOCK), 0, c->stream, mu0, mu1, d.mass_v, d.V, d.partials);
    hipLaunchKernelGGL(k_restart_boundary_fold, dim3(1), dim3(BLOCK), 0, c->stream, (const double *)d.partials, grid, d.partials + RESTART_SUM_BLOCKS);
    DOTS_HIP(hipGetLastError());
    DOTS_HIP(hipMemcpyAsync(c->h_pinned, d.partials + RESTART_SUM_BLOCKS, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    DOTS_HIP(hipStreamSynchronize(c->stream));
    *out = c->h_pinned[0];
    return 0;
}

void preload_restart_kernels() {      // (see preload_alm_kernels)
    const void *fns[] = {(const void *)k_restart_scale<false>, (const void *)k_restart_scale<true>, (const void *)k_restart_boundary, (const void *)k_restart_boundary_fold};
    hipFuncAttributes a;
    for (const void *f : fns) (void)hipFuncGetAttributes(&a, f);
    (void)hipGetLastError();
}

}  // namespace dots

// dots_barycenter_update (dots_api.hip): one mirror-descent step of a Wasserstein barycentre where the masses and the potentials lie
// (dots_socp_amd/barycenter.py: update_host is the specification).  The call takes no context: four launches on the caller's stream,
// every array in the caller's numbering:
//   k_bary_means    workgroup k forms m_k = sum(phi_k) / V
//   k_bary_update   g[v] = sum_k w_k * (-(phi_k[v] - m_k)), k ascending; y[v] = nu[v] * exp((-eta) * g[v]) into scratch; per workgroup
//                   the sum of y and the maximum of |g|
//   k_bary_finish   every workgroup folds the workgroups' sums of y to S in the same order, then nu[v] = y[v] * (mass / S) in place and,
//                   if asked for, at the vertex's row of a second numbering (a row outside [0, V) is not written); per workgroup the
//                   sum of |nu_new - nu| and the minimum
//   k_bary_fold     one workgroup folds those and the maxima into the four scalars
// Element by element these are update_host's operations in its order (the build has -ffp-contract=off); exp is the device library's.
// Every sum is two-stage in an order that depends on V alone -- lane l of workgroup b takes the vertices b * BLOCK + l + j * grid * BLOCK,
// j ascending; the lanes of a wave fold by shuffles, the four waves in order; lane l of the folding workgroup takes the workgroups l,
// l + BLOCK, ... -- and is carried as an unevaluated pair (hi, lo) with error-free additions (two_sum), so that it equals the host's
// fsum to the last bit or the one before it whatever the order.  Plain loads and stores; no atomics, no fences, nothing spins.
// Traffic: the potentials are read twice (n V doubles from memory, n V from the cache they stayed in), nu and y once each by the
// update and the finish (3 V), y, nu and the second numbering are written (3 V).
#include "dots_dev.h"
#include "pairs_dev.h"      // two_sum, DD, dd_add, dd_merge

#include <algorithm>

namespace dots {

enum BaryOp : int { BARY_MAX = 0, BARY_MIN = 1 };
template <int OP> __device__ __forceinline__ double bary_pick(double a, double b) { return OP == BARY_MAX ? fmax(a, b) : fmin(a, b); }

// The workgroup's pair and extremum; thread 0 gets them.  lds: [12].  Ends with the workgroup in step, so that lds may be used again.
template <int OP>
__device__ __forceinline__ void bary_block_fold(DD &s, double &x, double *lds) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        DD t;
        t.hi = __shfl_down(s.hi, o, 64);
        t.lo = __shfl_down(s.lo, o, 64);
        dd_merge(s, t);
        x = bary_pick<OP>(x, __shfl_down(x, o, 64));
    }
    if (lane == 0) {
        lds[w] = s.hi;
        lds[4 + w] = s.lo;
        lds[8 + w] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < 4; ++i) {
            dd_merge(s, DD{lds[i], lds[4 + i]});
            x = bary_pick<OP>(x, lds[8 + i]);
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(BLOCK) void k_bary_means(BaryArgs a) {
    __shared__ double lds[12];
    const double *p = a.phi[blockIdx.x];
    DD s{0.0, 0.0};
    double unused = 0.0;
    for (int v = threadIdx.x; v < a.V; v += BLOCK) dd_add(s, p[v]);
    bary_block_fold<BARY_MAX>(s, unused, lds);
    if (threadIdx.x == 0) a.mean[blockIdx.x] = (s.hi + s.lo) / (double)a.V;
}

// part: [6][G] = sum of y (hi, lo), max |g|, sum of the change (hi, lo), min
__global__ __launch_bounds__(BLOCK) void k_bary_update(BaryArgs a) {
    __shared__ double lds[12];
    DD s{0.0, 0.0};
    double gmax = 0.0;
    const double neg_eta = -a.eta;
    for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < a.V; v += (int64_t)gridDim.x * BLOCK) {
        double g = 0.0;
        for (int k = 0; k < a.n; ++k) g = g + a.w[k] * (-(a.phi[k][v] - a.mean[k]));
        const double y = a.nu[v] * exp(neg_eta * g);
        a.y[v] = y;
        dd_add(s, y);
        gmax = fmax(gmax, fabs(g));
    }
    bary_block_fold<BARY_MAX>(s, gmax, lds);
    if (threadIdx.x == 0) {
        a.part[blockIdx.x] = s.hi;
        a.part[a.G + blockIdx.x] = s.lo;
        a.part[2 * a.G + blockIdx.x] = gmax;
    }
}

// launched with the grid of k_bary_update (a.G workgroups)
__global__ __launch_bounds__(BLOCK) void k_bary_finish(BaryArgs a) {
    __shared__ double lds[12];
    __shared__ double total;
    DD s{0.0, 0.0};
    double unused = 0.0;
    for (int b = threadIdx.x; b < a.G; b += BLOCK) dd_merge(s, DD{a.part[b], a.part[a.G + b]});
    bary_block_fold<BARY_MAX>(s, unused, lds);
    if (threadIdx.x == 0) total = s.hi + s.lo;
    __syncthreads();
    const double S = total;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.out[0] = S;
    const double scale = a.mass / S;
    DD change{0.0, 0.0};
    double least = __builtin_inf();
    for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < a.V; v += (int64_t)gridDim.x * BLOCK) {
        const double old = a.nu[v];
        const double fresh = a.y[v] * scale;
        a.nu[v] = fresh;
        if (a.nu_dev) {
            const int row = a.inv_v ? a.inv_v[v] : (int)v;
            if ((unsigned)row < (unsigned)a.V) a.nu_dev[row] = fresh;      // (the map is the caller's: a bad entry must not write outside)
        }
        dd_add(change, fabs(fresh - old));
        least = fmin(least, fresh);
    }
    bary_block_fold<BARY_MIN>(change, least, lds);
    if (threadIdx.x == 0) {
        a.part[3 * a.G + blockIdx.x] = change.hi;
        a.part[4 * a.G + blockIdx.x] = change.lo;
        a.part[5 * a.G + blockIdx.x] = least;
    }
}

// one workgroup: out[1] = change, out[2] = gmax, out[3] = min
__global__ __launch_bounds__(BLOCK) void k_bary_fold(BaryArgs a) {
    __shared__ double lds[12];
    DD change{0.0, 0.0}, none{0.0, 0.0};
    double gmax = 0.0, least = __builtin_inf();
    for (int b = threadIdx.x; b < a.G; b += BLOCK) {
        dd_merge(change, DD{a.part[3 * a.G + b], a.part[4 * a.G + b]});
        gmax = fmax(gmax, a.part[2 * a.G + b]);
        least = fmin(least, a.part[5 * a.G + b]);
    }
    bary_block_fold<BARY_MAX>(change, gmax, lds);
    bary_block_fold<BARY_MIN>(none, least, lds);
    if (threadIdx.x == 0) {
        a.out[1] = change.hi + change.lo;
        a.out[2] = gmax;
        a.out[3] = least;
    }
}

int barycenter_workgroups(int V) { return std::max(1, std::min((V + BLOCK - 1) / BLOCK, BARY_MAX_WORKGROUPS)); }

// a.G = barycenter_workgroups(a.V); a.part holds 6 * a.G doubles, a.mean 16, a.out 4, a.y a.V
int launch_barycenter(hipStream_t stream, const BaryArgs &a) {
    hipLaunchKernelGGL(k_bary_means, dim3(a.n), dim3(BLOCK), 0, stream, a);
    hipLaunchKernelGGL(k_bary_update, dim3(a.G), dim3(BLOCK), 0, stream, a);
    hipLaunchKernelGGL(k_bary_finish, dim3(a.G), dim3(BLOCK), 0, stream, a);
    hipLaunchKernelGGL(k_bary_fold, dim3(1), dim3(BLOCK), 0, stream, a);
    DOTS_HIP(hipGetLastError());
    return 0;
}

void preload_barycenter_kernels() {      // (see preload_alm_kernels)
    const void *fns[] = {(const void *)k_bary_means, (const void *)k_bary_update, (const void *)k_bary_finish, (const void *)k_bary_fold};
    hipFuncAttributes attr;
    for (const void *f : fns) (void)hipFuncGetAttributes(&attr, f);
    (void)hipGetLastError();
}

}  // namespace dots

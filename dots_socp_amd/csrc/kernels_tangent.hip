// dots_tangent_velocities, dots_tangent_weights, dots_tangent_gram (dots_api.hip): linearised transport where the potentials lie
// (dots_socp_amd/tangent.py: velocities_host, weights_host and gram_host are the specifications).  The calls take no context; every
// array is in the caller's numbering:
//   k_tangent_velocities  one lane per TRIANGLE, looping over up to 16 potentials: vel[k][f][d] = (hat[f][0][d] * p0 + hat[f][1][d] * p1)
//                         + hat[f][2][d] * p2 with p_c = phi_k[tri[f][c]].  The lane reads its three indices and its nine hat doubles
//                         (contiguous) once and keeps them in registers for every potential -- one lane per (potential, triangle) would
//                         read those 84 bytes n times for 24 bytes written --; the three vertex rows are gathers, independent from one
//                         potential to the next; the three output doubles are contiguous.  More than 16 potentials take further launches.
//   k_tangent_weights     one lane per triangle: rho_c = sigma[v_c] / mass_v[v_c], w[f] = ((rho_0 + rho_1) + rho_2) * (area[f] * (1 / 3))
//   k_tangent_gram        workgroup (x, y) takes the 4 x 4 tile x of entries and the triangles y * BLOCK + lane + j * chunks * BLOCK, j
//                         ascending; per triangle a lane reads w, four rows of A and four of B (25 doubles) and adds the sixteen terms
//                         w * ((a0 * b0 + a1 * b1) + a2 * b2) to sixteen unevaluated pairs (pairs_dev.h) in registers; the lanes of a
//                         wave fold by shuffles, the four waves in order through LDS; one pair per entry and workgroup goes to scratch.
//                         A tile that reaches past na or nb reads its last row again and stores nothing for it.
//   k_tangent_gram_fold   one lane per entry merges its pairs, chunk 0 first, and writes hi + lo
// Element by element these are the specification's operations in its order (the build has -ffp-contract=off).  The number of chunks
// depends on F alone (tangent_chunks) and the order of every entry's sum on F and the chunks alone -- not on na, nb, the tile or
// whether B is A --, so two calls return the same bits, gram(A, A) is symmetric bit for bit (the products commute) and a block of rows
// and columns computed alone equals that block of the whole.  Plain loads and stores; no atomics, no fences, nothing spins.
// Traffic of the Gram: ceil(na / 4) * ceil(nb / 4) * 25 F doubles are requested against (na + nb) * 3 F + F unique ones -- every row
// of A is read ceil(nb / 4) times and every row of B ceil(na / 4) times instead of nb and na times; the repeats are served by the
// caches as long as the rows fit them.
#include "dots_dev.h"
#include "pairs_dev.h"

#include <algorithm>

namespace dots {

__global__ __launch_bounds__(BLOCK) void k_tangent_velocities(TangentVelArgs a) {
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= a.F) return;
    const int v0 = a.tri[3 * f], v1 = a.tri[3 * f + 1], v2 = a.tri[3 * f + 2];
    double h[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int d = 0; d < 3; ++d) h[c][d] = a.hat[9 * f + 3 * c + d];
    for (int k = 0; k < a.n; ++k) {
        const double *p = a.phi[k];
        const double p0 = p[v0], p1 = p[v1], p2 = p[v2];
        double *o = a.out + ((int64_t)k * a.F + f) * 3;
#pragma unroll
        for (int d = 0; d < 3; ++d) o[d] = (h[0][d] * p0 + h[1][d] * p1) + h[2][d] * p2;
    }
}

__global__ __launch_bounds__(BLOCK) void k_tangent_weights(const int *tri, const double *sigma, const double *mass_v, const double *area, double *w, int F) {
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    const int v0 = tri[3 * f], v1 = tri[3 * f + 1], v2 = tri[3 * f + 2];
    const double r0 = sigma[v0] / mass_v[v0], r1 = sigma[v1] / mass_v[v1], r2 = sigma[v2] / mass_v[v2];
    w[f] = ((r0 + r1) + r2) * (area[f] * (1.0 / 3.0));
}

// grid (tiles of entries, chunks); part: [chunks][na * nb][2]
__global__ __launch_bounds__(BLOCK) void k_tangent_gram(TangentGramArgs a) {
    constexpr int T = TANGENT_TILE;
    __shared__ double lds[T * T * 4 * 2];
    const int tiles_j = (a.nb + T - 1) / T;
    const int i0 = (blockIdx.x / tiles_j) * T, j0 = (blockIdx.x % tiles_j) * T;
    const double *pa[T], *pb[T];
#pragma unroll
    for (int r = 0; r < T; ++r) {
        pa[r] = a.A + (int64_t)min(i0 + r, a.na - 1) * a.F * 3;
        pb[r] = a.B + (int64_t)min(j0 + r, a.nb - 1) * a.F * 3;
    }
    DD acc[T][T];
#pragma unroll
    for (int r = 0; r < T; ++r)
#pragma unroll
        for (int c = 0; c < T; ++c) acc[r][c] = DD{0.0, 0.0};
    for (int64_t f = (int64_t)blockIdx.y * BLOCK + threadIdx.x; f < a.F; f += (int64_t)gridDim.y * BLOCK) {
        const double w = a.w[f];
        double x[T][3], y[T][3];
#pragma unroll
        for (int r = 0; r < T; ++r)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                x[r][d] = pa[r][3 * f + d];
                y[r][d] = pb[r][3 * f + d];
            }
#pragma unroll
        for (int r = 0; r < T; ++r)
#pragma unroll
            for (int c = 0; c < T; ++c) dd_add(acc[r][c], w * ((x[r][0] * y[c][0] + x[r][1] * y[c][1]) + x[r][2] * y[c][2]));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < T; ++r)
#pragma unroll
        for (int c = 0; c < T; ++c) {
            dd_wave_fold(acc[r][c]);
            if (lane == 0) {
                lds[((r * T + c) * 4 + wave) * 2] = acc[r][c].hi;
                lds[((r * T + c) * 4 + wave) * 2 + 1] = acc[r][c].lo;
            }
        }
    __syncthreads();
    if (threadIdx.x < T * T) {
        const int e = threadIdx.x, i = i0 + e / T, j = j0 + e % T;
        DD s{lds[e * 8], lds[e * 8 + 1]};
#pragma unroll
        for (int v = 1; v < 4; ++v) dd_merge(s, DD{lds[(e * 4 + v) * 2], lds[(e * 4 + v) * 2 + 1]});
        if (i < a.na && j < a.nb) {
            double *out = a.part + ((int64_t)blockIdx.y * a.na * a.nb + (int64_t)i * a.nb + j) * 2;
            out[0] = s.hi;
            out[1] = s.lo;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_tangent_gram_fold(TangentGramArgs a) {
    const int64_t entries = (int64_t)a.na * a.nb, e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= entries) return;
    DD s{0.0, 0.0};
    for (int c = 0; c < a.C; ++c) {
        const double *p = a.part + ((int64_t)c * entries + e) * 2;
        dd_merge(s, DD{p[0], p[1]});
    }
    a.G[e] = s.hi + s.lo;
}

int tangent_chunks(int F) { return std::max(1, std::min((F + TANGENT_CHUNK - 1) / TANGENT_CHUNK, TANGENT_MAX_CHUNKS)); }

int launch_tangent_velocities(hipStream_t stream, const TangentVelArgs &a) {
    hipLaunchKernelGGL(k_tangent_velocities, dim3((a.F + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, a);
    DOTS_HIP(hipGetLastError());
    return 0;
}

int launch_tangent_weights(hipStream_t stream, const int *tri, const double *sigma, const double *mass_v, const double *area, double *w, int F) {
    hipLaunchKernelGGL(k_tangent_weights, dim3((F + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, tri, sigma, mass_v, area, w, F);
    DOTS_HIP(hipGetLastError());
    return 0;
}

// a.C = tangent_chunks(a.F); a.part holds 2 * a.C * na * nb doubles, a.G na * nb
int launch_tangent_gram(hipStream_t stream, const TangentGramArgs &a) {
    constexpr int T = TANGENT_TILE;
    const int64_t entries = (int64_t)a.na * a.nb;
    hipLaunchKernelGGL(k_tangent_gram, dim3(((a.na + T - 1) / T) * ((a.nb + T - 1) / T), a.C), dim3(BLOCK), 0, stream, a);
    hipLaunchKernelGGL(k_tangent_gram_fold, dim3((unsigned)((entries + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, a);
    DOTS_HIP(hipGetLastError());
    return 0;
}

void preload_tangent_kernels() {      // (see preload_alm_kernels)
    const void *fns[] = {(const void *)k_tangent_velocities, (const void *)k_tangent_weights, (const void *)k_tangent_gram, (const void *)k_tangent_gram_fold};
    hipFuncAttributes attr;
    for (const void *f : fns) (void)hipFuncGetAttributes(&attr, f);
    (void)hipGetLastError();
}

}  // namespace dots

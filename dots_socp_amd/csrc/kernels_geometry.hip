// dots_move_vertices (dots_api.hip): the geometry tables of a context from new vertex positions, on the device.  The specification is
// dots_assemble (dissect.hip) and the per-corner loops of dots_create's build() (dots_api.hip): the same formulas in the same order of
// operations, and -ffp-contract=off on both sides, so the tables hold the host's bits.
//   k_geom_triangles   one lane per triangle: area, the three hat gradients, the validity flag          -> scratch
//   k_geom_mass        one lane per vertex: the sum of its corners' areas in list order, / 3.0            -> scratch
//   k_geom_corners     one lane per corner-list entry: c_area, c_D, fk_D, c_gA                            -> the context's tables
//   k_geom_stiffness   one lane per row of K: val in the order dots_assemble adds into a column, kdiag    -> the context's tables
// Gather-bound and tiny beside one iteration of the solver.
#include "dots_dev.h"

namespace dots {

__global__ __launch_bounds__(BLOCK) void k_geom_triangles(int F, const int *__restrict__ tri, const double *__restrict__ xyz, double *__restrict__ area,
                                                          double *__restrict__ hat, int *flag) {
    __shared__ double sh[BLOCK * 9];      // the block's gradients, so that the stores to hat are contiguous
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    if (f < F) {
        double p[3][3];
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int v = tri[3 * f + k];
            for (int c = 0; c < 3; ++c) {
                p[k][c] = xyz[3 * (size_t)v + c];
                finite = finite && isfinite(p[k][c]);
            }
        }
        double u[3], w2[3];
        for (int c = 0; c < 3; ++c) { u[c] = p[1][c] - p[0][c]; w2[c] = p[2][c] - p[1][c]; }
        const double cx = u[1] * w2[2] - u[2] * w2[1], cy = u[2] * w2[0] - u[0] * w2[2], cz = u[0] * w2[1] - u[1] * w2[0];
        const double a = 0.5 * __dsqrt_rn(cx * cx + cy * cy + cz * cz);
        area[f] = a;
        if (!finite || !(a > 0.0)) atomicOr(flag, 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) {       // altitude from the opposite edge to corner k, over its squared length
            const double *pa = p[(k + 1) % 3], *pb = p[(k + 2) % 3];
            double e[3], w[3], alt[3];
            for (int c = 0; c < 3; ++c) { e[c] = pb[c] - pa[c]; w[c] = p[k][c] - pa[c]; }
            const double we = w[0] * e[0] + w[1] * e[1] + w[2] * e[2], ee = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
            const double q = we / ee;
            for (int c = 0; c < 3; ++c) alt[c] = w[c] - e[c] * q;
            const double aa = alt[0] * alt[0] + alt[1] * alt[1] + alt[2] * alt[2];
            for (int c = 0; c < 3; ++c) sh[threadIdx.x * 9 + k * 3 + c] = alt[c] / aa;
        }
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * BLOCK * 9, end = (int64_t)F * 9;
    for (int i = threadIdx.x; i < BLOCK * 9 && base + i < end; i += BLOCK) hat[base + i] = sh[i];
}

__global__ __launch_bounds__(BLOCK) void k_geom_mass(int V, const int *__restrict__ cptr, const int *__restrict__ cidx, const double *__restrict__ area,
                                                     double *__restrict__ mass, int *flag) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    double m = 0.0;
    for (int j = cptr[v]; j < cptr[v + 1]; ++j) m += area[cidx[j] / 3];
    m /= 3.0;
    mass[v] = m;
    if (!(m > 0.0)) atomicOr(flag, 1);
}

__global__ __launch_bounds__(BLOCK) void k_geom_corners(int nC, const int *__restrict__ tri, const int *__restrict__ cidx, const double *__restrict__ area,
                                                        const double *__restrict__ hat, const double *__restrict__ mass, double *__restrict__ c_area,
                                                        double *__restrict__ c_D, double *__restrict__ fk_D, double *__restrict__ c_gA) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= nC) return;
    const int fk = cidx[j], f = fk / 3;
    const double a = area[f];
    const double dv = __dsqrt_rn(a / mass[tri[fk]]);
    c_area[j] = a;
    c_D[j] = dv;
    fk_D[fk] = dv;
    for (int c = 0; c < 3; ++c) c_gA[(size_t)j * 3 + c] = hat[(size_t)fk * 3 + c] * a;
}

__global__ __launch_bounds__(BLOCK) void k_geom_stiffness(int V, const int *__restrict__ tri, const int *__restrict__ cptr, const int *__restrict__ cidx,
                                                          const double *__restrict__ area, const double *__restrict__ hat, const int *__restrict__ rowptr,
                                                          const int *__restrict__ col, double *__restrict__ val, double *__restrict__ kdiag) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    for (int e = rowptr[v]; e < rowptr[v + 1]; ++e) {
        const int u = col[e];
        double s = 0.0;
        bool first = true;      // (the first contribution is assigned, as dots_assemble's row.emplace_back)
        for (int j = cptr[v]; j < cptr[v + 1]; ++j) {
            const int fk = cidx[j], f = fk / 3;
            const double *gk = hat + (size_t)fk * 3;
            for (int i = 0; i < 3; ++i) {
                if (tri[3 * f + i] != u) continue;
                const double *gi = hat + ((size_t)f * 3 + i) * 3;
                const double x = area[f] * (gk[0] * gi[0] + gk[1] * gi[1] + gk[2] * gi[2]);
                s = first ? x : s + x;
                first = false;
            }
        }
        val[e] = s;
        if (u == v) kdiag[v] = 0.0 + s;
    }
}

static unsigned blocks_for(int n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

int launch_geometry_validate(Ctx *c, const double *xyz, const GeomScratch &s) {
    const Dev &d = c->d;
    DOTS_HIP(hipMemsetAsync(s.flag, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(k_geom_triangles, dim3(blocks_for(d.F)), dim3(BLOCK), 0, c->stream, d.F, d.tri, xyz, s.area, s.hat, s.flag);
    hipLaunchKernelGGL(k_geom_mass, dim3(blocks_for(d.V)), dim3(BLOCK), 0, c->stream, d.V, d.cptr, d.cidx, (const double *)s.area, s.mass, s.flag);
    DOTS_HIP(hipGetLastError());
    return 0;
}

int launch_geometry_commit(Ctx *c, const GeomScratch &s) {
    const Dev &d = c->d;
    const int nC = 3 * d.F;
    auto w = [](const double *p) { return const_cast<double *>(p); };      // (the tables are the context's own allocations: Ctx::pool)
    hipLaunchKernelGGL(k_geom_corners, dim3(blocks_for(nC)), dim3(BLOCK), 0, c->stream, nC, d.tri, d.cidx, (const double *)s.area, (const double *)s.hat,
                       (const double *)s.mass, w(d.c_area), w(d.c_D), w(d.fk_D), w(d.c_gA));
    hipLaunchKernelGGL(k_geom_stiffness, dim3(blocks_for(d.V)), dim3(BLOCK), 0, c->stream, d.V, d.tri, d.cptr, d.cidx, (const double *)s.area,
                       (const double *)s.hat, d.rowptr, d.col, w(d.val), w(d.kdiag));
    DOTS_HIP(hipGetLastError());
    DOTS_HIP(hipMemcpyAsync(w(d.area_f), s.area, sizeof(double) * (size_t)d.F, hipMemcpyDeviceToDevice, c->stream));
    DOTS_HIP(hipMemcpyAsync(w(d.hat), s.hat, sizeof(double) * (size_t)d.F * 9, hipMemcpyDeviceToDevice, c->stream));
    DOTS_HIP(hipMemcpyAsync(w(d.mass_v), s.mass, sizeof(double) * (size_t)d.V, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

void preload_geometry_kernels() {      // (see preload_alm_kernels)
    const void *fns[] = {(const void *)k_geom_triangles, (const void *)k_geom_mass, (const void *)k_geom_corners, (const void *)k_geom_stiffness};
    hipFuncAttributes a;
    for (const void *f : fns) (void)hipFuncGetAttributes(&a, f);
    (void)hipGetLastError();
}

}  // namespace dots

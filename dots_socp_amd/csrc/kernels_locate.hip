// dots_mesh_locate: the closest point of a triangle mesh to every one of a set of points, over ALL triangles, on the device.
// dots_socp_amd/cascade.py (locate_exact, corner_exact, closest_scalar_order) is the specification; the arithmetic per point and
// triangle below is written in its order of operations (the build has -ffp-contract=off), so the results agree bit for bit.  Only the
// search differs: a uniform grid over the mesh lists every triangle in the cells its bounding box overlaps, and one lane per point
// walks rings of cells around its own cell until its best distance certifies that no triangle outside the rings can win or tie.
// It runs once per pair of levels of a cascade: the yardstick is the host location it replaces (cascade.locate), not a roofline.
#include "dots_dev.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

namespace dots {

namespace {

constexpr int LOCATE_BLOCK = 256;
constexpr double RING_MARGIN = 0.999;      // a ring certifies distances below RING_MARGIN * r * cell: the cell index of a point is rounded

struct LocateGrid {
    int nx, ny, nz;
    double cell;      // edge of the cubic cells
};

// Ericson's closest point on a triangle (Real-Time Collision Detection, 5.1.5) as cascade.closest_scalar_order states it: the clamped
// weights of the corners and the SQUARED distance.  Every quotient is formed whether its region is taken or not, as numpy does.
__device__ __forceinline__ double dot3(double x0, double x1, double x2, double y0, double y1, double y2) { return (x0 * y0 + x1 * y1) + x2 * y2; }

__device__ __forceinline__ void closest_on_triangle(double px, double py, double pz, const double *__restrict__ t, double &w0, double &w1, double &w2,
                                                    double &dist2) {
    const double ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5], cx = t[6], cy = t[7], cz = t[8];
    const double abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
    const double d1 = dot3(abx, aby, abz, px - ax, py - ay, pz - az), d2 = dot3(acx, acy, acz, px - ax, py - ay, pz - az);
    const double d3 = dot3(abx, aby, abz, px - bx, py - by, pz - bz), d4 = dot3(acx, acy, acz, px - bx, py - by, pz - bz);
    const double d5 = dot3(abx, aby, abz, px - cx, py - cy, pz - cz), d6 = dot3(acx, acy, acz, px - cx, py - cy, pz - cz);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const double t_ab = d1 / (d1 - d3), t_ac = d2 / (d2 - d6);
    const double t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    const double denom = 1.0 / ((va + vb) + vc);
    double a1 = vb * denom, a2 = vc * denom;      // the interior
    if (d1 <= 0 && d2 <= 0) { a1 = 0.0; a2 = 0.0; }
    else if (d3 >= 0 && d4 <= d3) { a1 = 1.0; a2 = 0.0; }
    else if (vc <= 0 && d1 >= 0 && d3 <= 0) { a1 = t_ab; a2 = 0.0; }
    else if (d6 >= 0 && d5 <= d6) { a1 = 0.0; a2 = 1.0; }
    else if (vb <= 0 && d2 >= 0 && d6 <= 0) { a1 = 0.0; a2 = t_ac; }
    else if (va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0) { a1 = 1.0 - t_bc; a2 = t_bc; }
    a1 = a1 < 0.0 ? 0.0 : (a1 > 1.0 ? 1.0 : a1);
    a2 = a2 < 0.0 ? 0.0 : (a2 > 1.0 ? 1.0 : a2);
    double a0 = (1.0 - a1) - a2;
    a0 = a0 < 0.0 ? 0.0 : a0;
    const double rx = px - ((a0 * ax + a1 * bx) + a2 * cx), ry = py - ((a0 * ay + a1 * by) + a2 * cy), rz = pz - ((a0 * az + a1 * bz) + a2 * cz);
    w0 = a0;
    w1 = a1;
    w2 = a2;
    dist2 = dot3(rx, ry, rz, rx, ry, rz);
}

// One lane per point, in the order `order` (the points sorted by cell: a wavefront walks the same cell lists and its loads of the
// lists and of the corners coincide).  cell_of[slot]: the point's own cell, clamped into the grid.  Ring r = the cells at Chebyshev
// distance r; after ring r every triangle not yet seen is at least r * cell away, so best < (margin * r * cell)^2 ends the search
// (strictly: a tie with a smaller index may lie just outside); it also ends when the rings have covered the grid (r_max).  A triangle
// listed in several cells is tested again with the same outcome.
__global__ __launch_bounds__(LOCATE_BLOCK) void k_locate(int n, LocateGrid g, const int *__restrict__ order, const int *__restrict__ cell_of,
                                                         const double *__restrict__ points, const int *__restrict__ cell_ptr,
                                                         const int *__restrict__ cell_tri, const double *__restrict__ corners,
                                                         int *__restrict__ tri_out, double *__restrict__ w_out, double *__restrict__ d2_out) {
    const int slot = blockIdx.x * LOCATE_BLOCK + threadIdx.x;
    if (slot >= n) return;
    const int i = order[slot];
    const double px = points[3 * (size_t)i], py = points[3 * (size_t)i + 1], pz = points[3 * (size_t)i + 2];
    const int c = cell_of[slot];
    const int cx = c % g.nx, cy = (c / g.nx) % g.ny, cz = c / (g.nx * g.ny);
    const int r_max = max(max(max(cx, g.nx - 1 - cx), max(cy, g.ny - 1 - cy)), max(cz, g.nz - 1 - cz));
    double best = INFINITY, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    int best_tri = 0x7fffffff;
    for (int r = 0; r <= r_max; ++r) {
        const int z_lo = max(cz - r, 0), z_hi = min(cz + r, g.nz - 1), y_lo = max(cy - r, 0), y_hi = min(cy + r, g.ny - 1);
        const int x_lo = max(cx - r, 0), x_hi = min(cx + r, g.nx - 1);
        for (int z = z_lo; z <= z_hi; ++z)
            for (int y = y_lo; y <= y_hi; ++y) {
                // a row on the shell in y or z is walked whole; an inner row touches the shell at its two ends only
                const bool whole = r == 0 || z == cz - r || z == cz + r || y == cy - r || y == cy + r;
                const int step = whole ? 1 : 2 * r;
                for (int x = whole ? x_lo : cx - r; x <= x_hi; x += step) {
                    if (x < x_lo) continue;
                    const int cell = (z * g.ny + y) * g.nx + x;
                    const int k_end = cell_ptr[cell + 1];
                    for (int k = cell_ptr[cell]; k < k_end; ++k) {
                        const int f = cell_tri[k];
                        double w0, w1, w2, d2;
                        closest_on_triangle(px, py, pz, corners + 9 * (size_t)f, w0, w1, w2, d2);
                        if (d2 < best || (d2 == best && f < best_tri)) {
                            best = d2;
                            best_tri = f;
                            b0 = w0;
                            b1 = w1;
                            b2 = w2;
                        }
                    }
                }
            }
        const double reach = (RING_MARGIN * (double)r) * g.cell;
        if (best < reach * reach) break;
    }
    tri_out[i] = best_tri;
    w_out[3 * (size_t)i] = b0;
    w_out[3 * (size_t)i + 1] = b1;
    w_out[3 * (size_t)i + 2] = b2;
    d2_out[i] = best;
}

// corner[i][k]: the corner of triangle tri[i] with the largest clamped weight of corner point k of point i, the first maximum on a tie
__global__ __launch_bounds__(LOCATE_BLOCK) void k_locate_corner(int n, int n_tri, const double *__restrict__ corner_points, const int *__restrict__ tri,
                                                                const double *__restrict__ corners, int *__restrict__ corner_out) {
    const int j = blockIdx.x * LOCATE_BLOCK + threadIdx.x;      // (point, corner point)
    if (j >= 3 * n) return;
    const int f = tri[j / 3];
    if (f < 0 || f >= n_tri) {      // (no triangle was found: coordinates whose differences overflow; the entry point reports it)
        corner_out[j] = 0;
        return;
    }
    double w0, w1, w2, d2;
    closest_on_triangle(corner_points[3 * (size_t)j], corner_points[3 * (size_t)j + 1], corner_points[3 * (size_t)j + 2], corners + 9 * (size_t)f, w0, w1,
                        w2, d2);
    int arg = 0;
    double top = w0;
    if (w1 > top) { arg = 1; top = w1; }
    if (w2 > top) arg = 2;
    corner_out[j] = arg;
}

int refuse(const char *what) {
    set_error(std::string("mesh_locate: ") + what);
    return DOTS_ERR_ARGUMENT;
}

struct LocateScope {      // the call's events and the caller's device ordinal, put back on every way out of the entry point
    hipEvent_t ev[2] = {nullptr, nullptr};
    int previous_device = -1;
    ~LocateScope() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (previous_device >= 0) (void)hipSetDevice(previous_device);
    }
};

inline int cell_index(double x, double lo, double inv_cell, int n) {
    double t = std::floor((x - lo) * inv_cell);
    if (!(t > 0.0)) t = 0.0;
    if (t > (double)(n - 1)) t = (double)(n - 1);
    return (int)t;
}

}  // namespace

}  // namespace dots

using namespace dots;

extern "C" int dots_mesh_locate(const dots_mesh_locate_desc *d, int device) {
    if (!d) return refuse("null descriptor");
    if (!d->points || !d->vertices || !d->triangles || !d->triangle || !d->weights || !d->distance) return refuse("null array");
    if ((d->corner != nullptr) != (d->corner_points != nullptr)) return refuse("corner and corner_points go together");
    if (d->n_points < 1 || d->n_vertices < 1 || d->n_triangles < 1) return refuse("sizes must be at least 1");
    const int N = d->n_points, V = d->n_vertices, F = d->n_triangles;
    if ((int64_t)N * 9 > 0x7fffffff || (int64_t)F * 9 > 0x7fffffff) return refuse("too many points or triangles (9 n must stay below 2^31)");
    for (int64_t i = 0; i < (int64_t)F * 3; ++i)
        if (d->triangles[i] < 0 || d->triangles[i] >= V) return refuse("triangle index out of range");
    for (int64_t i = 0; i < (int64_t)V * 3; ++i)
        if (!std::isfinite(d->vertices[i])) return refuse("non-finite coordinates");
    for (int64_t i = 0; i < (int64_t)N * 3; ++i)
        if (!std::isfinite(d->points[i])) return refuse("non-finite points");
    if (d->corner_points)
        for (int64_t i = 0; i < (int64_t)N * 9; ++i)
            if (!std::isfinite(d->corner_points[i])) return refuse("non-finite corner points");
    // the nine corner coordinates of every triangle, its bounding box, the mean edge length
    std::vector<double> corners((size_t)F * 9);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, edge_sum = 0.0;
    for (int f = 0; f < F; ++f) {
        double *t = &corners[(size_t)f * 9];
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) {
                t[3 * k + a] = d->vertices[3 * (size_t)d->triangles[3 * (size_t)f + k] + a];
                lo[a] = std::min(lo[a], t[3 * k + a]);
                hi[a] = std::max(hi[a], t[3 * k + a]);
            }
        const double e1[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]}, e2[3] = {t[6] - t[0], t[7] - t[1], t[8] - t[2]}, e3[3] = {t[6] - t[3], t[7] - t[4], t[8] - t[5]};
        const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        if (!(std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) > 0.0)) return refuse("the mesh has a triangle of zero area");
        edge_sum += std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]) + std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]) +
                    std::sqrt(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error("no HIP device"); return DOTS_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) return refuse("device ordinal out of range");

    // the grid: cubic cells of about the mean edge length, doubled until cells and list entries stay within bounds
    const double extent = std::max(std::max(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
    double cell = edge_sum / (3.0 * (double)F);
    if (!(cell > 0.0) || !std::isfinite(cell) || !std::isfinite(extent)) return refuse("the mesh has no finite extent");
    cell = std::max(cell, extent / 1024.0);
    const int64_t max_cells = 1 << 22, max_entries = std::min<int64_t>(64 * (int64_t)F + (1 << 20), 0x7fffffff);
    LocateGrid g;
    std::vector<int> cell_ptr, cell_tri, box((size_t)F * 6);
    for (int attempt = 0;; ++attempt) {
        if (attempt == 64) return refuse("no grid fits this mesh");
        const double inv = 1.0 / cell;
        g.cell = cell;
        g.nx = (int)std::min(std::floor((hi[0] - lo[0]) * inv), 1023.0) + 1;
        g.ny = (int)std::min(std::floor((hi[1] - lo[1]) * inv), 1023.0) + 1;
        g.nz = (int)std::min(std::floor((hi[2] - lo[2]) * inv), 1023.0) + 1;
        const int64_t n_cells = (int64_t)g.nx * g.ny * g.nz;
        int64_t entries = 0;
        if (n_cells <= max_cells) {
            const int dims[3] = {g.nx, g.ny, g.nz};
            for (int f = 0; f < F; ++f) {
                const double *t = &corners[(size_t)f * 9];
                int64_t count = 1;
                for (int a = 0; a < 3; ++a) {
                    const int c0 = cell_index(std::min(std::min(t[a], t[3 + a]), t[6 + a]), lo[a], inv, dims[a]);
                    const int c1 = cell_index(std::max(std::max(t[a], t[3 + a]), t[6 + a]), lo[a], inv, dims[a]);
                    box[(size_t)f * 6 + 2 * a] = c0;
                    box[(size_t)f * 6 + 2 * a + 1] = c1;
                    count *= c1 - c0 + 1;
                }
                entries += count;
            }
        }
        if (n_cells > max_cells || entries > max_entries) {
            cell *= 2.0;
            continue;
        }
        cell_ptr.assign((size_t)n_cells + 1, 0);
        cell_tri.resize((size_t)entries);
        for (int pass = 0; pass < 2; ++pass) {      // count, then fill (triangles ascending inside a cell)
            for (int f = 0; f < F; ++f) {
                const int *b = &box[(size_t)f * 6];
                for (int z = b[4]; z <= b[5]; ++z)
                    for (int y = b[2]; y <= b[3]; ++y)
                        for (int x = b[0]; x <= b[1]; ++x) {
                            const size_t c = ((size_t)z * g.ny + y) * g.nx + x;
                            if (pass == 0) ++cell_ptr[c + 1];
                            else cell_tri[(size_t)cell_ptr[c]++] = f;
                        }
            }
            if (pass == 0)
                for (size_t c = 0; c < (size_t)n_cells; ++c) cell_ptr[c + 1] += cell_ptr[c];
            else {
                for (size_t c = (size_t)n_cells; c > 0; --c) cell_ptr[c] = cell_ptr[c - 1];
                cell_ptr[0] = 0;
            }
        }
        break;
    }
    // the points sorted by their cell (a counting sort: stable, so the order is the same run to run)
    const size_t n_cells = (size_t)g.nx * g.ny * g.nz;
    std::vector<int> own((size_t)N), start(n_cells + 1, 0), order((size_t)N), cell_of((size_t)N);
    {
        const double inv = 1.0 / g.cell;
        for (int i = 0; i < N; ++i) {
            const double *p = d->points + 3 * (size_t)i;
            own[(size_t)i] = (cell_index(p[2], lo[2], inv, g.nz) * g.ny + cell_index(p[1], lo[1], inv, g.ny)) * g.nx + cell_index(p[0], lo[0], inv, g.nx);
            ++start[(size_t)own[(size_t)i] + 1];
        }
        for (size_t c = 0; c < n_cells; ++c) start[c + 1] += start[c];
        for (int i = 0; i < N; ++i) {
            const int slot = start[(size_t)own[(size_t)i]]++;
            order[(size_t)slot] = i;
            cell_of[(size_t)slot] = own[(size_t)i];
        }
    }

    LocateScope dev;
    int previous = -1;
    DOTS_HIP(hipGetDevice(&previous));
    DOTS_HIP(hipSetDevice(device));
    dev.previous_device = previous;
    int *d_order, *d_cell_of, *d_cell_ptr, *d_cell_tri, *d_tri, *d_corner = nullptr;
    double *d_points, *d_corners, *d_w, *d_d2, *d_cpoints = nullptr;
    DevicePool mem(device);      // (after `dev`: freed before the caller's device ordinal is put back)
    auto get = [&](auto **p, size_t count, const auto *host) -> int {      // not zeroed; filled from `host` where given, with a synchronous copy
        const int r = mem.alloc(p, (int64_t)count, nullptr, false);
        if (r) return r;
        if (host) DOTS_HIP(hipMemcpy(*p, host, count * sizeof(**p), hipMemcpyHostToDevice));
        return 0;
    };
    int rc;
    if ((rc = get(&d_order, (size_t)N, order.data())) || (rc = get(&d_cell_of, (size_t)N, cell_of.data())) ||
        (rc = get(&d_cell_ptr, cell_ptr.size(), cell_ptr.data())) || (rc = get(&d_cell_tri, cell_tri.size(), cell_tri.data())) ||
        (rc = get(&d_points, (size_t)N * 3, d->points)) || (rc = get(&d_corners, corners.size(), corners.data())) ||
        (rc = get(&d_tri, (size_t)N, (const int *)nullptr)) || (rc = get(&d_w, (size_t)N * 3, (const double *)nullptr)) ||
        (rc = get(&d_d2, (size_t)N, (const double *)nullptr))) return rc;
    if (d->corner && ((rc = get(&d_cpoints, (size_t)N * 9, d->corner_points)) || (rc = get(&d_corner, (size_t)N * 3, (const int *)nullptr)))) return rc;
    DOTS_HIP(hipEventCreate(&dev.ev[0]));
    DOTS_HIP(hipEventCreate(&dev.ev[1]));
    DOTS_HIP(hipEventRecord(dev.ev[0], nullptr));
    hipLaunchKernelGGL(k_locate, dim3((unsigned)((N + LOCATE_BLOCK - 1) / LOCATE_BLOCK)), dim3(LOCATE_BLOCK), 0, nullptr, N, g, d_order, d_cell_of, d_points,
                       d_cell_ptr, d_cell_tri, d_corners, d_tri, d_w, d_d2);
    DOTS_HIP(hipGetLastError());
    if (d->corner) {
        hipLaunchKernelGGL(k_locate_corner, dim3((unsigned)((3 * N + LOCATE_BLOCK - 1) / LOCATE_BLOCK)), dim3(LOCATE_BLOCK), 0, nullptr, N, F, d_cpoints, d_tri,
                           d_corners, d_corner);
        DOTS_HIP(hipGetLastError());
    }
    DOTS_HIP(hipEventRecord(dev.ev[1], nullptr));
    DOTS_HIP(hipEventSynchronize(dev.ev[1]));
    if (d->ms) {
        float ms = 0.0f;
        DOTS_HIP(hipEventElapsedTime(&ms, dev.ev[0], dev.ev[1]));
        *d->ms = (double)ms;
    }
    DOTS_HIP(hipMemcpy(d->triangle, d_tri, (size_t)N * sizeof(int), hipMemcpyDeviceToHost));
    DOTS_HIP(hipMemcpy(d->weights, d_w, (size_t)N * 3 * sizeof(double), hipMemcpyDeviceToHost));
    DOTS_HIP(hipMemcpy(d->distance, d_d2, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    if (d->corner) DOTS_HIP(hipMemcpy(d->corner, d_corner, (size_t)N * 3 * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < N; ++i)
        if (d->triangle[i] < 0 || d->triangle[i] >= F) {
            set_error("mesh_locate: a point found no triangle (coordinates whose differences overflow)");
            return DOTS_ERR_STATE;
        }
    for (int i = 0; i < N; ++i) d->distance[i] = std::sqrt(d->distance[i]);      // (on the host: the square root of the specification)
    return DOTS_OK;
}

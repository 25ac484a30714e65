// Cost gradients (dots_sensitivity): the Kantorovich potential at the two ends and the per-triangle stress of the kinetic energy,
// reduced over time where the state lies, in the caller's numbering (dots_socp_amd/sensitivity.py: potentials_host and stress_host
// are the specification).  18 doubles per triangle and 2 per vertex leave the device instead of phi and mu (16 (T + 1) V bytes).
//
// k_sens_stress: one lane per (caller triangle f, corner k).  The rows of a vertex are time-fastest, so the lane streams the mu row
// of its own vertex and the phi rows of the triangle's three vertices with 16-byte loads (two columns at a time; the three
// corners of a triangle read the same phi rows, and a row is one run of cache lines) and keeps six accumulators, one per entry
// (a, b) = 00, 01, 02, 11, 12, 22.  Per interval t, ascending: x = factor_mu * mu[t], m = x * mass; p = factor_phi * phi (one
// multiplication per value); q1 = p_{t+1}[a] * p_{t+1}[b] (q0: the q1 of the interval before), s = q0 + q1, w = 0.5 * s, c = m * w,
// acc = acc + c -- these operations in this order, the build has -ffp-contract=off, so the result is the host's bit for bit.
// The lane writes its six sums as three 16-byte words: out[f][k][0 .. 6).  Plain loads and stores only.
#include "dots_dev.h"

namespace dots {

// the six products of a node's three values, in the order of the entries
__device__ __forceinline__ void sens_products(double (&q)[6], double p0, double p1, double p2) {
    q[0] = p0 * p0; q[1] = p0 * p1; q[2] = p0 * p2;
    q[3] = p1 * p1; q[4] = p1 * p2; q[5] = p2 * p2;
}

__global__ __launch_bounds__(BLOCK) void k_sens_stress(SensArgs a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;      // caller corner f * 3 + k
    if (i >= 3 * a.F) return;
    const int f = i / 3, k = i - 3 * f;
    const int fd = a.inv_f ? a.inv_f[f] : f;
    const int v0 = a.tri[fd * 3], v1 = a.tri[fd * 3 + 1], v2 = a.tri[fd * 3 + 2];
    const int vk = k == 0 ? v0 : (k == 1 ? v1 : v2);
    const double mass = a.mass ? a.mass[a.perm_v ? a.perm_v[vk] : vk] : a.mass_dev[vk];
    const double *r0 = a.phi + ((int64_t)v0 << a.tp_shift), *r1 = a.phi + ((int64_t)v1 << a.tp_shift), *r2 = a.phi + ((int64_t)v2 << a.tp_shift);
    const double *rm = a.mu + ((int64_t)vk << a.tp_shift);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, q0[6], q1[6];
    double x_prev = 0.0;      // mu of the interval that ends at the node being taken
    // nodes c = 0 .. T two at a time; node c > 0 closes the interval c - 1 (T + 1 <= TP and TP is even: the pair stays inside the row)
    for (int c = 0; c <= a.T; c += 2) {
        const D2 a0 = ld2(r0 + c), a1 = ld2(r1 + c), a2 = ld2(r2 + c), am = ld2(rm + c);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (c + j > a.T) break;
            const double p0 = a.factor_phi * a0.v[j], p1 = a.factor_phi * a1.v[j], p2 = a.factor_phi * a2.v[j];
            sens_products(q1, p0, p1, p2);
            if (c + j > 0) {
                const double m = x_prev * mass;
#pragma unroll
                for (int e = 0; e < 6; ++e) {
                    const double s = q0[e] + q1[e];
                    const double w = 0.5 * s;
                    acc[e] = acc[e] + m * w;
                }
            }
#pragma unroll
            for (int e = 0; e < 6; ++e) q0[e] = q1[e];
            x_prev = a.factor_mu * am.v[j];
        }
    }
    double *o = a.stress + (int64_t)i * 6;
    st2(o, D2{{acc[0], acc[1]}});
    st2(o + 2, D2{{acc[2], acc[3]}});
    st2(o + 4, D2{{acc[4], acc[5]}});
}

// one lane per caller vertex: phi0[v] = factor_phi * phi[row][0], phiT[v] = factor_phi * phi[row][T]
__global__ __launch_bounds__(BLOCK) void k_sens_potentials(SensArgs a) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= a.V) return;
    const double *row = a.phi + ((int64_t)(a.inv_v ? a.inv_v[v] : v) << a.tp_shift);
    if (a.phi0) a.phi0[v] = a.factor_phi * row[0];
    if (a.phiT) a.phiT[v] = a.factor_phi * row[a.T];
}

int launch_sensitivity(Ctx *c, const SensArgs &a) {
    if (a.phi0 || a.phiT) {
        hipLaunchKernelGGL(k_sens_potentials, dim3((a.V + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, a);
        DOTS_HIP(hipGetLastError());
    }
    if (a.stress) {
        hipLaunchKernelGGL(k_sens_stress, dim3((3 * a.F + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, a);
        DOTS_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace dots

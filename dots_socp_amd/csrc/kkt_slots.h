// The per-element terms of the KKT sums (reference: solver_socp.py:433-559), each condition written once.  The stand-alone sums
// (kernels_kkt.hip: kkt_vertex_body, kkt_triangle_body, k_kkt_dual_alpha_carried) call them on what they load; steps 2+3
// (kernels_alm.hip: q_lambda_vertex_tile, ql_lane) on the values they have just computed -- DOTS_STEP_KKT_SUMS.
// sv: a lane's vertex sums, indexed by V_*; sf: its triangle sums, indexed by F_* - N_VSUMS.  m / w: the vertex's mass, the triangle's area.
#pragma once
#include "dots_dev.h"

#ifdef __HIPCC__
namespace dots {

__device__ __forceinline__ double wsq(double x, double w) { return x * x * w; }

// Prim(phi, q): :433-450, residuals of :592-593 (V_LAM2, which Comp(rho, cong.) shares, is added by the caller)
__device__ __forceinline__ void kkt_v_prim_q(double *sv, double dphi, double A, double lc, double m) {
    sv[V_DPHI2] += wsq(dphi, m);
    sv[V_A2] += wsq(A, m);
    sv[V_RESMU2] += wsq(dphi - A - lc, m);
}
// Prim(q, z): :452-464 with :598-600
__device__ __forceinline__ void kkt_v_prim_z(double *sv, const KktArgs &a, double zf, double ze, double A, double m) {
    sv[V_RFST2] += wsq(zf + a.sz * A - a.cd, m);
    sv[V_REND2] += wsq(ze - a.sz * A - a.cd, m);
}
// Dual(beta): :484-503 (V_MU2, shared with the Comp conditions, is added by the caller)
__device__ __forceinline__ void kkt_v_dual_beta(double *sv, const KktArgs &a, double mu, double bf, double be, double m) {
    const double a1 = a.sz * (be - bf);
    sv[V_AUX1_2] += wsq(a1, m);
    sv[V_MUAUX1_2] += wsq(mu + a1, m);
}
// Comp(rho, f(q)): :505-526 with :615-619; q = sum over the corners of area * (|ps B[t]|^2 + |ps B[t + 1]|^2) / 3
__device__ __forceinline__ void kkt_v_comp_rho(double *sv, const KktArgs &a, double A, double mu, double q, double m) {
    const double rho = (a.ds * a.r) * mu;
    const double aux = a.ps * A + 0.25 * q / m;
    const double res = fmax(0.0, aux + rho) - rho;
    sv[V_COMP_AUX2] += wsq(aux, m);
    sv[V_COMP_RES2] += wsq(res, m);
}
// Comp(rho, cong.): :549-559 with :633-636
__device__ __forceinline__ void kkt_v_cong(double *sv, const KktArgs &a, double mu, double lc, double m) {
    sv[V_CONG_RES2] += wsq(a.cong * ((a.ds * a.r) * mu) - a.ps * lc, m);
}
// Dual(alpha): :466-482, the term of V_DUALAUX2 at local node t.  mu / mu_prev: the multiplier of the interval that starts / ends at
// the node (used when it exists); dsx: the node's gather of area * hat . E over the vertex's corners
__device__ __forceinline__ double kkt_v_dual_alpha(const Dev &d, const KktArgs &a, int v, int t, double mu, double mu_prev, double dsx, double m) {
    double x = 0.0;
    if (t < d.ni) x += mu * m;
    if (has_prev_interval(d, t)) x -= mu_prev * m;
    x *= 1.0 / d.h;
    x -= dsx;
    if (first_node(d, t)) x -= a.bs * d.mu0[v] / (a.r * d.h);
    if (last_node(d, t)) x += a.bs * d.mu1[v] / (a.r * d.h);
    return wsq((a.r * d.h) * x / m, m);
}

// Prim(phi, q), triangle part: gx = grad_space(phi)
__device__ __forceinline__ void kkt_f_prim_q(double *sf, double gx, double B, double w) {
    sf[F_DX2 - N_VSUMS] += wsq(gx, w);
    sf[F_B2 - N_VSUMS] += wsq(B, w);
    sf[F_RESE2 - N_VSUMS] += wsq(gx - B, w);
}
// Dual(beta), triangle part: s0 / s1 = the sums over the corners of the node's s = 0 / s = 1 entries of beta_mid (F_E2, shared with
// Comp(m, rho o B), is added by the caller)
__device__ __forceinline__ void kkt_f_dual_beta(double *sf, double sB, double E, double s0, double s1, double w) {
    const double a2 = sB * (s0 + s1);
    sf[F_AUX2_2 - N_VSUMS] += wsq(a2, w);
    sf[F_EAUX2_2 - N_VSUMS] += wsq(E + a2, w);
}
// Comp(m, rho o B): :528-547 with :624-628; rn = sum over the corners of 0.5 * ds r * (mu of the node's two intervals)
__device__ __forceinline__ void kkt_f_comp_m(double *sf, const KktArgs &a, double rn, double B, double E, double w) {
    const double aux = (rn * (1.0 / 3.0)) * (a.ps * B);
    sf[F_AUX5_2 - N_VSUMS] += wsq(aux, w);
    sf[F_AUX5M_2 - N_VSUMS] += wsq(aux - (a.ds * a.r) * E, w);
}
// z_mid part of Prim(q, z): sz (z_mid - L B), one entry; sb = sz / sqrt3 * B
__device__ __forceinline__ void kkt_f_rmid(double *sf, double sz, double z, double sb, double w) { sf[F_RMID2 - N_VSUMS] += wsq(sz * (z - sb), w); }

}  // namespace dots
#endif

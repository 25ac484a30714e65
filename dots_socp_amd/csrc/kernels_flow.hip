// The flow map (dots_flow_map, dots_flow_push, dots_flow_trace, dots_flow_slide): particles traced through the transport on the device
// -- where the mass at a point ends up, where it is after every interval, what it carries there, how far it moved.
// dots_socp_amd/flow.py is the specification (flow_map_host, push_forward_host); the operations below are its operations in its order
// (the build has -ffp-contract=off, fp64 division is correctly rounded), so the outputs equal it bit for bit.  It extends what the
// reference returns (solver_socp.py:855-869, mu and E) without moving the two arrays to the host.
//
// One tracer body, flow_body<PUSH, A, SLIDE>, one lane per particle; the loop over the intervals is inside the kernel because a
// particle's steps depend on each other.  A lane reads the state where it lies (rows of mu and E, time fastest): a particle that stays
// in its triangle reads neighbouring doubles in successive intervals.  The triangle's vertices and hat gradients stay in registers
// until the particle crosses an edge.  The three weights and rates live in named registers and are selected with conditions: an array
// indexed by the exit corner would go to scratch.  It runs once per solve: the yardstick is the download of mu and E it replaces,
// not a roofline.
//
// Every trace is a span (FlowSpan): the a.T intervals j = j0 + i dj, i = 0 .. a.T - 1, between two time nodes, forward (dj = 1) or
// backward (dj = -1: the velocity negated), with the kinetic action, the sum of best |u|^2 along the path, stored on request.  The
// whole horizon of dots_flow_map / dots_flow_push is j0 = 0, dj = 1, a.T = n_time.  Direction and start are run-time values: a sign
// flip and an add per turn beside six fp64 divisions, where a template flag would double the instantiations for nothing.
//
// The template flags are the two that change what a lane holds in registers (DESIGN.md section 9 has the table):
// - PUSH, with the number of attributes A: the tracer also deposits what the particle carries on the vertices of its triangle at
//   every layer, in 64-bit fixed point with integer atomics; k_flow_push_finish turns the sums into doubles in the caller's vertex
//   numbering.  A is a template argument so that the channels are straight-line code on named registers.
// - SLIDE: the sliding mode of the discontinuous field (flow.py: step 3a of flow_map_host): where the triangle just entered pushes the
//   particle back across the edge it came through, it moves along that edge with the combination of the two velocities whose normal
//   part vanishes, instead of crossing back and forth until the cap and resting.  What step 3a needs of the triangle left (two
//   doubles and the two shared corners) is formed at the crossing and stays in registers; the corner-indexed reads are selects on the
//   named registers.  The end of a slide is selects, not branches, and the five per-particle counters go to the rows of one array
//   (FlowSlide::o_counts): one base pointer held through the loop.  With the branches and five output pointers
//   k_flow_slide_push<A> spilled 12 - 20 scalar registers.
#include "dots_dev.h"

namespace dots {

// max(x, 0.0) as the specification forms it: a NaN stays a NaN
__device__ __forceinline__ double flow_clamp0(double x) { return 0.0 > x ? 0.0 : x; }

struct FlowTriangle {
    int64_t r0, r1, r2;      // first element of the vertices' rows of mu
    int64_t e;               // first element of the triangle's three rows of E
    double g00, g01, g02, g10, g11, g12, g20, g21, g22;      // hat gradients, [corner][xyz]
};
__device__ __forceinline__ void flow_load_triangle(const FlowArgs &a, int f, FlowTriangle &t) {
    const int *v = a.tri + (int64_t)f * 3;
    t.r0 = (int64_t)v[0] << a.tp_shift;
    t.r1 = (int64_t)v[1] << a.tp_shift;
    t.r2 = (int64_t)v[2] << a.tp_shift;
    t.e = ((int64_t)f * 3) << a.tp_shift;
    const double *g = a.hat + (int64_t)f * 9;
    t.g00 = g[0]; t.g01 = g[1]; t.g02 = g[2];
    t.g10 = g[3]; t.g11 = g[4]; t.g12 = g[5];
    t.g20 = g[6]; t.g21 = g[7]; t.g22 = g[8];
}

__device__ __forceinline__ void flow_store_layer(const FlowArgs &a, int layer, int p, int f, double l0, double l1, double l2) {
    const int64_t at = (int64_t)layer * a.P + p;
    if (a.tri_at) a.tri_at[at] = a.perm_f ? a.perm_f[f] : f;
    if (a.w_at) {
        double *w = a.w_at + at * 3;
        w[0] = l0; w[1] = l1; w[2] = l2;
    }
}

// The deposit of dots_flow_push (flow.py: push_forward_host is the specification): the particle's channels g[c] -- its mass, and its
// mass times each attribute -- go to the three vertices of the triangle it is in, weighted with l0, l1, l2, as 64-bit integers
// q = rint((g * l) * 2^k_c) added with integer atomics: integer addition is associative, so the sums are the same bits for every
// arrival order.  |y| < 2^62 false (a NaN included) drops the contribution and counts it; a zero issues no atomic.
__device__ __forceinline__ void flow_deposit_one(unsigned long long *row, double g, int k, double l, int &dropped) {
    const double x = g * l;
    const double y = ldexp(x, k);      // x * 2^k, correctly rounded: the product of the specification (2^k is a double for |k| <= 1000)
    if (!(fabs(y) < 0x1p62)) { ++dropped; return; }
    const long long q = __double2ll_rn(y);
    if (q != 0) atomicAdd(row, (unsigned long long)q);
}
template <int A>
__device__ __forceinline__ void flow_deposit(const FlowArgs &a, const FlowPush &q, int layer, const FlowTriangle &t, double l0, double l1, double l2,
                                             const double (&g)[A + 1], int &dropped) {
    int slot = layer;
    if (q.L == 1) {      // (only the state after the last turn, a.T; with all the layers L = a.T + 1 >= 2)
        if (layer != a.T) return;
        slot = 0;
    }
    const int64_t v0 = t.r0 >> a.tp_shift, v1 = t.r1 >> a.tp_shift, v2 = t.r2 >> a.tp_shift;
#pragma unroll
    for (int c = 0; c <= A; ++c) {
        unsigned long long *row = q.acc + ((int64_t)c * q.L + slot) * q.V;
        flow_deposit_one(row + v0, g[c], q.k[c], l0, dropped);
        flow_deposit_one(row + v1, g[c], q.k[c], l1, dropped);
        flow_deposit_one(row + v2, g[c], q.k[c], l2, dropped);
    }
}

// element k of three named registers, as a select (an indexed array would go to scratch); k outside 0 .. 2 gives the last
__device__ __forceinline__ double flow_pick(int k, double x0, double x1, double x2) { return k == 0 ? x0 : (k == 1 ? x1 : x2); }
// element 3 - c - k of three named registers, c and k two different corners: the same two comparisons as flow_pick(c) and flow_pick(k)
__device__ __forceinline__ double flow_pick_third(int c, int k, double x0, double x1, double x2) {
    return c == 0 ? (k == 1 ? x2 : x1) : (c == 1 ? (k == 0 ? x2 : x0) : (k == 0 ? x1 : x0));
}
__device__ __forceinline__ double flow_dot(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// the tracer; PUSH: it also deposits what the particle carries (A attributes: a template argument, so that the channels are
// straight-line code on named registers) wherever it stores a layer
template <bool PUSH, int A, bool SLIDE = false>
__device__ __forceinline__ void flow_body(const FlowArgs &a, const FlowPush &q, const FlowSpan &span, const FlowSlide &sl = FlowSlide{}) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.P) return;
    int f = a.start_tri[p];
    double l0 = a.start_w[(int64_t)p * 3], l1 = a.start_w[(int64_t)p * 3 + 1], l2 = a.start_w[(int64_t)p * 3 + 2];
    int status = 0, rested = 0, total = 0;
    FlowTriangle t;
    flow_load_triangle(a, f, t);
    flow_store_layer(a, 0, p, f, l0, l1, l2);
    double g[A + 1] = {};
    int dropped = 0;
    if (PUSH) {
        g[0] = q.mass[p];
#pragma unroll
        for (int c = 1; c <= A; ++c) g[c] = g[0] * q.attr[(int64_t)(c - 1) * a.P + p];
    }
    const int pitch = 1 << a.tp_shift;
    double act = 0.0;      // the action so far
    int slides = 0, steps = 0;      // (SLIDE)
    // (PUSH: one more turn, which only deposits -- layer i at the head of turn i, so that the deposit is in the code once)
    for (int i = 0; PUSH ? i <= a.T : i < a.T; ++i) {
        if (PUSH) {
            flow_deposit<A>(a, q, i, t, l0, l1, l2, g, dropped);
            if (i == a.T) break;
        }
        const int j = span.j0 + i * span.dj;      // the interval of turn i (a.T is the number of intervals traversed)
        if (status == 0) {
            double rem = a.h;
            int crossings = 0;
            // of the crossing of the turn before: the corners that name the vertices of the edge crossed, and (SLIDE) the corner opposite
            // that edge (-1: none), the edge rate and the normal speed times the area of the triangle left
            int ca = 0, cb = 0, ent = -1;
            double sP = 0.0, mP = 0.0;
            for (;;) {
                // density of the interval on the triangle, velocity from the momentum of its two nodes
                // (loading the momentum beside the density instead of behind the floor test changed nothing: 2.38 against 2.37 ms)
                const double rho = ((a.mu[t.r0 + j] + a.mu[t.r1 + j]) + a.mu[t.r2 + j]) * (1.0 / 3.0);
                double u0 = 0.0, u1 = 0.0, u2 = 0.0;
                if (rho > a.floor) {
                    const double *e = a.E + t.e + j;
                    u0 = (0.5 * (e[0] + e[1])) / rho;
                    u1 = (0.5 * (e[pitch] + e[pitch + 1])) / rho;
                    u2 = (0.5 * (e[2 * pitch] + e[2 * pitch + 1])) / rho;
                    if (span.dj < 0) { u0 = -u0; u1 = -u1; u2 = -u2; }      // (backward; a floored triangle keeps +0.0)
                }
                // time derivatives of the weights
                const double q0 = (t.g00 * u0 + t.g01 * u1) + t.g02 * u2;
                const double q1 = (t.g10 * u0 + t.g11 * u1) + t.g12 * u2;
                const double q2 = (t.g20 * u0 + t.g21 * u1) + t.g22 * u2;
                int left_out = -1;      // (SLIDE: the corner step 4 leaves out after a slide that reached a vertex)
                if (SLIDE) {
                    ++steps;
                    const int c = ent;
                    ent = -1;
                    bool over = false;      // the slide ended the interval
                    const double qc = flow_pick(c, q0, q1, q2);
                    if (c >= 0 && qc < 0.0) {      // step 3a: this triangle pushes back across the edge just crossed
                        const double hc0 = flow_pick(c, t.g00, t.g10, t.g20), hc1 = flow_pick(c, t.g01, t.g11, t.g21), hc2 = flow_pick(c, t.g02, t.g12, t.g22);
                        const double ha0 = flow_pick(ca, t.g00, t.g10, t.g20), ha1 = flow_pick(ca, t.g01, t.g11, t.g21), ha2 = flow_pick(ca, t.g02, t.g12, t.g22);
                        const double cc = flow_dot(hc0, hc1, hc2, hc0, hc1, hc2), ac = flow_dot(ha0, ha1, ha2, hc0, hc1, hc2);
                        const double qa = flow_pick(ca, q0, q1, q2);
                        const double sG = qa - (ac / cc) * qc;
                        const double mG = (-qc) * sl.area_f[f];
                        const double s = (mG * sP + mP * sG) / (mP + mG);      // each side weighted with the other side's normal speed
                        const double la = flow_pick(ca, l0, l1, l2), lb = flow_pick_third(c, ca, l0, l1, l2);      // (cb = 3 - c - ca)
                        // (one division for both signs of s: tau = l[cb] / s or l[ca] / (-s); s = 0 or NaN takes neither)
                        const bool up = s > 0.0, moves = up || s < 0.0;
                        const double tau = (up ? lb : la) / (up ? s : -s);
                        const bool hits = moves && tau < rem;
                        const double best = hits ? tau : rem;
                        const double qh = up ? flow_pick_third(c, ca, q0, q1, q2) : qa;      // the rate of the corner hit: cb (up) or ca
                        const double aa = flow_dot(ha0, ha1, ha2, ha0, ha1, ha2);
                        act = act + best * ((s * s) * (cc / (aa * cc - ac * ac)));      // (|d|^2 of the edge from the hat gradients)
                        const double na = hits && !up ? 0.0 : flow_clamp0(la + best * s), nb = hits && up ? 0.0 : flow_clamp0(lb - best * s);
                        l0 = c == 0 ? l0 : (ca == 0 ? na : nb);      // (the weight of corner c keeps its 0.0)
                        l1 = c == 1 ? l1 : (ca == 1 ? na : nb);
                        l2 = c == 2 ? l2 : (ca == 2 ? na : nb);
                        ++slides;
                        // the interval ended; or at the cap, or at the vertex where this triangle does not pass the particle on: a rest
                        const bool rest = hits && (crossings == a.max_crossings || !(qh < 0.0));
                        over = !hits || rest;
                        rem = hits ? rem - best : rem;
                        rested += rest ? 1 : 0;
                        crossings += over ? 0 : 1;      // (bounds the loop; a slide is not an edge crossed: `total` stays)
                        left_out = over ? -1 : c;
                    }
                    if (over) break;
                }
                // the first weight to reach zero before the interval ends (strict comparisons: the first corner wins a tie)
                double best = rem;
                int kmin = -1;
                if ((!SLIDE || left_out != 0) && q0 < 0.0) { const double s = l0 / (-q0); if (s < best) { best = s; kmin = 0; } }
                if ((!SLIDE || left_out != 1) && q1 < 0.0) { const double s = l1 / (-q1); if (s < best) { best = s; kmin = 1; } }
                if ((!SLIDE || left_out != 2) && q2 < 0.0) { const double s = l2 / (-q2); if (s < best) { best = s; kmin = 2; } }
                act = act + best * ((u0 * u0 + u1 * u1) + u2 * u2);      // (a step that ends in a stop or a rest has spent best)
                const double n0 = flow_clamp0(l0 + best * q0), n1 = flow_clamp0(l1 + best * q1), n2 = flow_clamp0(l2 + best * q2);
                l0 = kmin == 0 ? 0.0 : n0;
                l1 = kmin == 1 ? 0.0 : n1;
                l2 = kmin == 2 ? 0.0 : n2;
                if (kmin < 0) break;
                rem = rem - best;
                const int packed = a.nbr[(int64_t)f * 3 + kmin];
                if (packed < 0) { status = 1; break; }
                if (crossings == a.max_crossings) { ++rested; break; }
                ++crossings;
                ++total;
                // the two kept weights go to the corners of the neighbour that name the same vertices
                const double wa = kmin == 0 ? l1 : (kmin == 1 ? l2 : l0);      // corner (kmin + 1) % 3
                const double wb = kmin == 0 ? l2 : (kmin == 1 ? l0 : l1);      // corner (kmin + 2) % 3
                if (SLIDE) {      // what step 3a of the next turn needs of the triangle left; ka = (kmin + 1) % 3
                    const double hk0 = flow_pick(kmin, t.g00, t.g10, t.g20), hk1 = flow_pick(kmin, t.g01, t.g11, t.g21), hk2 = flow_pick(kmin, t.g02, t.g12, t.g22);
                    const double ha0 = flow_pick(kmin, t.g10, t.g20, t.g00), ha1 = flow_pick(kmin, t.g11, t.g21, t.g01), ha2 = flow_pick(kmin, t.g12, t.g22, t.g02);
                    const double hh = flow_dot(hk0, hk1, hk2, hk0, hk1, hk2), ah = flow_dot(ha0, ha1, ha2, hk0, hk1, hk2);
                    const double qk = flow_pick(kmin, q0, q1, q2);
                    sP = flow_pick(kmin, q1, q2, q0) - (ah / hh) * qk;
                    mP = (-qk) * sl.area_f[f];
                }
                ca = (packed >> 2) & 3;
                cb = packed & 3;
                if (SLIDE) ent = 3 - ca - cb;      // the corner of the neighbour opposite the edge crossed
                l0 = ca == 0 ? wa : (cb == 0 ? wb : 0.0);
                l1 = ca == 1 ? wa : (cb == 1 ? wb : 0.0);
                l2 = ca == 2 ? wa : (cb == 2 ? wb : 0.0);
                f = packed >> 4;
                flow_load_triangle(a, f, t);
            }
        }
        flow_store_layer(a, i + 1, p, f, l0, l1, l2);
    }
    if (span.action) span.action[p] = act;
    a.o_tri[p] = a.perm_f ? a.perm_f[f] : f;
    a.o_w[(int64_t)p * 3] = l0;
    a.o_w[(int64_t)p * 3 + 1] = l1;
    a.o_w[(int64_t)p * 3 + 2] = l2;
    if (SLIDE) {      // (the five counters are rows of one array: one base pointer held through the loop instead of five)
        int *o = sl.o_counts + p;
        o[0] = status;
        o[(int64_t)a.P] = rested;
        o[(int64_t)a.P * 2] = total;
        o[(int64_t)a.P * 3] = slides;
        o[(int64_t)a.P * 4] = steps;
    } else {
        a.o_status[p] = status;
        a.o_rested[p] = rested;
        a.o_cross[p] = total;
    }
    if (PUSH && dropped) atomicAdd(q.acc + (int64_t)(A + 1) * q.L * q.V, (unsigned long long)dropped);      // (the word behind the sums)
}

__global__ __launch_bounds__(BLOCK) void k_flow_trace(FlowArgs a, FlowSpan s) { flow_body<false, 0>(a, FlowPush{}, s); }
template <int A>
__global__ __launch_bounds__(BLOCK) void k_flow_trace_push(FlowArgs a, FlowPush q, FlowSpan s) { flow_body<true, A>(a, q, s); }
__global__ __launch_bounds__(BLOCK) void k_flow_slide(FlowArgs a, FlowSpan s, FlowSlide sl) { flow_body<false, 0, true>(a, FlowPush{}, s, sl); }
template <int A>
__global__ __launch_bounds__(BLOCK) void k_flow_slide_push(FlowArgs a, FlowPush q, FlowSpan s, FlowSlide sl) { flow_body<true, A, true>(a, q, s, sl); }

// One lane per (channel, layer, caller vertex), the vertex fastest: the accumulator of the vertex's device row as a double, times
// 2^-k_c; a layer of the output is one contiguous run in the caller's numbering, as in k_readout_mu.
__global__ __launch_bounds__(BLOCK) void k_flow_push_finish(FlowPushFinish q) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t n_layer = (int64_t)q.L * q.V;
    if (i >= n_layer * (q.A + 1)) return;
    const int64_t cl = i / q.V;
    const int v = (int)(i - cl * q.V);
    const int c = (int)(i / n_layer);
    const long long s = (long long)q.acc[cl * q.V + (q.inv ? q.inv[v] : v)];
    q.out[i] = (double)s * q.unscale[c];
}

// the tracer of a request: `push` null: no deposits; `slide` null: without the sliding mode
int launch_flow(Ctx *c, const FlowArgs &a, const FlowSpan &s, const FlowPush *push, const FlowSlide *slide) {
    const dim3 grid((unsigned)((a.P + BLOCK - 1) / BLOCK)), block(BLOCK);
    if (push)
        with_constant<0, 1, 2, 3, 4>(push->A, [&](auto A) {
            if (slide) hipLaunchKernelGGL(k_flow_slide_push<A.value>, grid, block, 0, c->stream, a, *push, s, *slide);
            else hipLaunchKernelGGL(k_flow_trace_push<A.value>, grid, block, 0, c->stream, a, *push, s);
        });
    else if (slide) hipLaunchKernelGGL(k_flow_slide, grid, block, 0, c->stream, a, s, *slide);
    else hipLaunchKernelGGL(k_flow_trace, grid, block, 0, c->stream, a, s);
    DOTS_HIP(hipGetLastError());
    return 0;
}
int launch_flow_push_finish(Ctx *c, const FlowPushFinish &q) {
    const int64_t n = (int64_t)(q.A + 1) * q.L * q.V;
    hipLaunchKernelGGL(k_flow_push_finish, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, q);
    DOTS_HIP(hipGetLastError());
    return 0;
}
void preload_flow_kernels() {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, (const void *)k_flow_push_finish);
    (void)hipFuncGetAttributes(&attr, (const void *)k_flow_trace);
    (void)hipFuncGetAttributes(&attr, (const void *)k_flow_trace_push<0>);
    (void)hipFuncGetAttributes(&attr, (const void *)k_flow_slide);
    (void)hipFuncGetAttributes(&attr, (const void *)k_flow_slide_push<0>);
    (void)hipGetLastError();
}

}  // namespace dots

// Carrying the state from one context to another (dots_prolong_time, dots_prolong_space, dots_transfer_space, dots_carry_spacetime):
// one state array of a context on another mesh, another time grid, or both, device layout to device layout.  One family: a SPACE
// stage that forms a destination row on the source's time grid from whole source rows, a TIME stage that interpolates such a row onto
// the destination's time grid, and two kernels.  k_carry_space (both contexts have one time pitch) is the space stage alone, row to
// row through registers.  k_carry_spacetime is the space stage into LDS, then the time stage out of it; with the space mode SAME
// (the same row of the same mesh) it is dots_prolong_time.  cascade.prolong_time / prolong_space / transfer_space / carry_spacetime
// on the recovered solution are the specification: the operations below are theirs in their order (the build has -ffp-contract=off,
// the parenthesisation is the specification), so that the result is what an upload of the host's transfer leaves, bit for bit.
#include "dots_dev.h"

namespace dots {

struct CarryArgs {
    const double *src;
    double *dst;
    const int *jt;           // [nd] source time point of every destination time point      } of this array's grid: the node
    const double *wt;        // [nd] weight of source point j + 1                            } or the interval tables
    const int *vsrc;         // vertex rows: [entities] (same, or null: the same row), [entities][2] (nested) or [entities][3] (located) source rows
    const double *vw;        // located vertex rows: [entities][3] weights
    const int *fsrc;         // triangle and corner rows: [entities] source triangle (same: or null, the same triangle)
    const int *csrc;         // corner rows: [entities][3] source corner of every destination corner, or null: the same corner
    int64_t rows;            // destination rows
    int64_t run;             // k_carry_space: rows per run
    int nd, ns;              // destination / source time points of this array's grid: T + 1 (node arrays) or T
    int sh_d, sh_s;          // log2 of the destination / source pitch
    int R;                   // k_carry_spacetime: rows per pass
    double f;
};
constexpr int CARRY_XS = 4096, CARRY_RMAX = 64, CARRY_NT = 1024;      // doubles of source rows per pass, rows per pass, table entries

// ------------------------------------------------------------------------------------------
// the space stage
// ------------------------------------------------------------------------------------------
// RPE: rows per vertex / triangle: 1, 3 (B, E), 18 (corner arrays: row = ((f * 3 + k) * 2 + s) * 3 + c, column = interval + s).
// A triangle row is f times the row of the same component of its source triangle, a corner row f times the row of its source corner
// (same interval end and component): the corner csrc names, or the same corner where csrc is null (a child triangle keeps its
// parent's corner order).  A vertex row (RPE = 1) is one of three formulas, chosen at compile time because they differ in the sign of
// zero and in the subnormal range:
//   same    (the same mesh):            f * a, a the row vsrc names, or the same row where vsrc is null (one numbering);
//   nested  (a mesh to its refinement): f * a where the two source rows are one (a kept vertex), else (f * a + f * b) * 0.5;
//   located (another triangulation):    (w0 * (f * a0) + w1 * (f * a1)) + w2 * (f * a2), no special case for a weight of 0 or 1.
// SAME also lets fsrc be null (the same triangle) and reads every source row exactly once, so its loads are non-temporal; nested and
// located siblings and neighbours re-read rows from the cache.
struct CarrySource {
    const double *x0, *x1, *x2;      // source rows: one, or the 2 / 3 of a vertex row
    double w0, w1, w2;
    int s;                           // interval end of a corner row: its columns are shifted by one
};

template <int RPE, int MODE>
__device__ __forceinline__ CarrySource carry_source(const CarryArgs &a, int64_t r) {
    int64_t r0, r1 = 0, r2 = 0;
    CarrySource c{nullptr, nullptr, nullptr, 0.0, 0.0, 0.0, 0};
    if (RPE == 1 && MODE == CARRY_LOCATED) {
        const int *v = a.vsrc + 3 * r;
        const double *w = a.vw + 3 * r;
        r0 = v[0], r1 = v[1], r2 = v[2];
        c.w0 = w[0], c.w1 = w[1], c.w2 = w[2];
    } else if (RPE == 1 && MODE == CARRY_NESTED) {
        r0 = a.vsrc[2 * r];
        r1 = a.vsrc[2 * r + 1];
    } else if (RPE == 1) {
        r0 = a.vsrc ? (int64_t)a.vsrc[r] : r;
    } else {
        const int64_t ent = r / RPE;
        const int sub = (int)(r - ent * RPE);
        r0 = (MODE == CARRY_SAME && !a.fsrc) ? ent : (int64_t)a.fsrc[ent];
        if (RPE == 18) {      // sub = (k * 2 + s) * 3 + c
            const int k = sub / 6, rest = sub - 6 * k;
            c.s = rest / 3;
            r0 = (r0 * 3 + (a.csrc ? a.csrc[3 * ent + k] : k)) * 6 + rest;
        } else {
            r0 = r0 * 3 + sub;
        }
    }
    c.x0 = a.src + (r0 << a.sh_s);
    c.x1 = a.src + (r1 << a.sh_s);
    c.x2 = a.src + (r2 << a.sh_s);
    return c;
}

// columns 2 p and 2 p + 1 of the row on the source's time grid
template <int RPE, int MODE>
__device__ __forceinline__ D2 carry_pair(const CarrySource &c, double f, int p) {
    const D2 v0 = MODE == CARRY_SAME ? ld2_nt(c.x0 + 2 * p) : ld2(c.x0 + 2 * p);
    D2 out;
    if (RPE == 1 && MODE == CARRY_LOCATED) {
        const D2 v1 = ld2(c.x1 + 2 * p), v2 = ld2(c.x2 + 2 * p);
#pragma unroll
        for (int q = 0; q < 2; ++q) out.v[q] = (c.w0 * (f * v0.v[q]) + c.w1 * (f * v1.v[q])) + c.w2 * (f * v2.v[q]);
    } else if (RPE == 1 && MODE == CARRY_NESTED && c.x0 != c.x1) {
        const D2 v1 = ld2(c.x1 + 2 * p);
#pragma unroll
        for (int q = 0; q < 2; ++q) out.v[q] = (f * v0.v[q] + f * v1.v[q]) * 0.5;
    } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) out.v[q] = f * v0.v[q];
    }
    return out;
}

// ------------------------------------------------------------------------------------------
// the time stage
// ------------------------------------------------------------------------------------------
// Destination columns 2 p and 2 p + 1 from a row x on the source's time grid: time point t takes (1 - w[t]) * x[j[t]] + w[t] *
// x[min(j[t] + 1, ns - 1)].  Corner arrays hold interval i of half s in column i + s on both sides: x is the row from column s on,
// interpolated along the interval index and placed at t + s.  The slots whose interval does not exist and the padding columns are
// written as zero (as k_convert writes them).  Only columns j < ns of x are read.
__device__ __forceinline__ D2 carry_time_pair(const double *x, const int *js, const double *ws, int p, int s, int nd, int ns) {
    D2 y;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int t = 2 * p + q - s;      // time point of this column
        double v = 0.0;
        if (t >= 0 && t < nd) {
            const int j = js[t], j1 = min(j + 1, ns - 1);
            const double w = ws[t];
            v = (1.0 - w) * x[j] + w * x[j1];
        }
        y.v[q] = v;
    }
    return y;
}

// ------------------------------------------------------------------------------------------
// the run kernel (dots_prolong_space, dots_transfer_space): another mesh, the same time grid
// ------------------------------------------------------------------------------------------
// Both contexts have one time pitch, so the space stage is the whole transfer: no LDS.  A lane forms two neighbouring columns (16-byte
// words in, one out); a row's indices and weights are read once per row; a row wider than 256 columns is walked in chunks of 256.
// Columns outside the array's time points (padding, and the slot of a corner row whose interval does not exist) are written as zero, as
// k_convert writes them.  A workgroup takes runs of consecutive destination rows.  Nested, a run is a whole number of groups of four
// vertices / triangles: the four children of a triangle, which read the same 3 or 18 source rows, are numbered together by the
// subdivision (and stay close under a locality renumbering), so the source rows come from HBM once and from the cache for the
// siblings.  Located, neighbouring destination vertices / triangles under a locality numbering lie in the same or in neighbouring
// source triangles, so most of the 3 source rows per vertex row come from the cache.
template <int RPE, int MODE>
__global__ __launch_bounds__(BLOCK) void k_carry_space(CarryArgs a) {
    const int tid = threadIdx.x;
    const int hp = a.sh_d - 1;                    // log2 of the column pairs per row
    const int hl = min(hp, 7);                    // log2 of the lanes per row: at most 128 pairs = 256 columns per chunk
    const int rpp = BLOCK >> hl;                  // rows per pass
    const int rr = tid >> hl, p0 = tid & ((1 << hl) - 1);
    const int64_t n_runs = (a.rows + a.run - 1) / a.run;
    for (int64_t run = blockIdx.x; run < n_runs; run += gridDim.x) {
        const int64_t r_end = min(a.rows, (run + 1) * a.run);
        for (int64_t r = run * a.run + rr; r < r_end; r += rpp) {
            const CarrySource c = carry_source<RPE, MODE>(a, r);
            double *y = a.dst + (r << a.sh_d);
            for (int p = p0; p < (1 << hp); p += 1 << hl) {
                D2 out = carry_pair<RPE, MODE>(c, a.f, p);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int t = 2 * p + q - c.s;
                    if (t < 0 || t >= a.nd) out.v[q] = 0.0;
                }
                st2(y + 2 * p, out);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// the staged kernel (dots_carry_spacetime; with MODE = SAME: dots_prolong_time): another time grid
// ------------------------------------------------------------------------------------------
// A workgroup stages the two time tables once, then walks passes of R destination rows in two phases.  Phase 1 forms each row of the
// pass ON THE SOURCE'S TIME GRID with the space stage (the recovery factor f first) from 16-byte loads at the source pitch and writes it
// into LDS: what a carrier in space would have left in a context on the destination's mesh at the source's n_time never reaches memory.
// Phase 2 is the time stage on those rows, two destination columns per lane, one 16-byte store.  Only columns j < ns of an LDS row are
// read, so what phase 1 leaves in the source's padding columns (f times a padding column) is never used.  LDS rows are TPs + 2 doubles
// apart: an even number, so that phase 1's 16-byte writes stay aligned and neighbouring lanes write neighbouring words (no bank is hit
// twice), and not a power of two, so that in phase 2 lane groups on neighbouring rows read other banks.
// SAME against interpolating the source row directly, (1 - w) * (f * x[j]) + w * (f * x[j1]): LDS holds f * x, the time stage forms
// (1 - w) * xs[j] + w * xs[j1] -- the same two products and the same sum.
template <int RPE, int MODE>
__global__ __launch_bounds__(BLOCK) void k_carry_spacetime(CarryArgs a) {
    __shared__ __attribute__((aligned(16))) double xs[CARRY_XS + 2 * CARRY_RMAX];
    __shared__ double ws[CARRY_NT];
    __shared__ int js[CARRY_NT];
    const int tid = threadIdx.x;
    const int TPs = 1 << a.sh_s, SP = TPs + 2;
    const int hs = a.sh_s - 1, hd = a.sh_d - 1;     // log2 of the column pairs per source / destination row
    for (int t = tid; t < a.nd; t += BLOCK) {
        js[t] = a.jt[t];
        ws[t] = a.wt[t];
    }
    const int64_t n_pass = (a.rows + a.R - 1) / a.R;
    for (int64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
        const int64_t base = pass * a.R;
        __syncthreads();      // the tables are staged / the previous pass has read its rows
        // phase 1: space, source rows -> LDS
        for (int e = tid; e < (a.R << hs); e += BLOCK) {
            const int rr = e >> hs, p = e & ((1 << hs) - 1);
            const int64_t r = base + rr;
            if (r >= a.rows) continue;
            st2(xs + rr * SP + 2 * p, carry_pair<RPE, MODE>(carry_source<RPE, MODE>(a, r), a.f, p));
        }
        __syncthreads();
        // phase 2: time, LDS -> destination rows
        for (int e = tid; e < (a.R << hd); e += BLOCK) {
            const int rr = e >> hd, p = e & ((1 << hd) - 1);
            const int64_t r = base + rr;
            if (r >= a.rows) continue;
            const int s = RPE == 18 ? (int)((r / 3) & 1) : 0;
            st2(a.dst + (r << a.sh_d) + 2 * p, carry_time_pair(xs + rr * SP + s, js, ws, p, s, a.nd, a.ns));
        }
    }
}

// Array `id` of dst from the one of src, on dst's stream.  The node or the interval tables of t by the array's grid; time tables in t:
// the staged kernel, else the run kernel; who: the entry point, for the message.
int launch_carry(Ctx *dst, Ctx *src, int id, const CarryTables &t, double f, const char *who) {
    const Dev &dd = dst->d, &ds = src->d;
    const int kind = array_kind(id);
    const int node = kind == 0 || kind == 2;
    const int rpe = kind <= 1 ? 1 : (kind == 2 ? 3 : 18);
    // triangle and corner rows have one formula for nested and located
    const int mode = (rpe == 1 || t.mode == CARRY_SAME) ? t.mode : CARRY_NESTED;
    CarryArgs a{};
    a.src = src->arr(id);
    a.dst = dst->arr(id);
    a.jt = node ? t.node_j : t.interval_j;
    a.wt = node ? t.node_w : t.interval_w;
    a.vsrc = t.vsrc;
    a.vw = t.vw;
    a.fsrc = t.fsrc;
    a.csrc = t.csrc;
    a.rows = (int64_t)rpe * (kind <= 1 ? dd.V : dd.F);
    a.nd = dd.T + node;
    a.ns = ds.T + node;
    a.sh_d = dd.tp_shift;
    a.sh_s = ds.tp_shift;
    a.f = f;
    const bool staged = a.jt != nullptr;
    const bool fits = staged ? a.nd <= CARRY_NT && a.sh_s >= 1 && a.sh_d >= 1 && a.sh_d <= 12 && (1 << a.sh_s) <= CARRY_XS
                             : mode != CARRY_SAME && a.sh_d >= 1 && dd.TP <= TILE_ELEMS && a.sh_d == a.sh_s;
    if (!fits) {      // (dots_prolong_time's launches have always said "prolong")
        set_error(std::string(t.mode == CARRY_SAME ? "prolong" : who) + ": time pitch out of range");
        return DOTS_ERR_STATE;
    }
    void (*kernel)(CarryArgs);
    int64_t n_blocks;
    const int unit = 4 * rpe;      // nested: the four children of a triangle (and the vertices the subdivision numbers with them) read the same source rows
    if (staged) {
        a.R = std::max(1, std::min(std::min(CARRY_RMAX, (4 * BLOCK) >> (a.sh_d - 1)), CARRY_XS >> a.sh_s));
        // nested: a pass takes whole groups of four where R holds one (the corner arrays' 72 rows never fit: their passes stay at R)
        if (t.mode == CARRY_NESTED && a.R >= unit) a.R -= a.R % unit;
        n_blocks = std::min<int64_t>((a.rows + a.R - 1) / a.R, 1024);
        kernel = mode == CARRY_SAME      ? (rpe == 1 ? k_carry_spacetime<1, CARRY_SAME> : rpe == 3 ? k_carry_spacetime<3, CARRY_SAME> : k_carry_spacetime<18, CARRY_SAME>)
                 : mode == CARRY_LOCATED ? k_carry_spacetime<1, CARRY_LOCATED>
                                         : (rpe == 1 ? k_carry_spacetime<1, CARRY_NESTED> : rpe == 3 ? k_carry_spacetime<3, CARRY_NESTED> : k_carry_spacetime<18, CARRY_NESTED>);
    } else {
        // a run: whole groups of vertices / triangles, whole passes of the workgroup, about 32 KB of destination
        const int rpp = BLOCK >> std::min(a.sh_d - 1, 7);
        int64_t group = t.mode == CARRY_NESTED ? unit : rpe;
        while (group % rpp) group *= 2;
        const int64_t row_bytes = (int64_t)sizeof(double) << a.sh_d;
        a.run = group * std::max<int64_t>(1, (32768 + group * row_bytes - 1) / (group * row_bytes));
        n_blocks = std::min<int64_t>((a.rows + a.run - 1) / a.run, 4096);
        kernel = mode == CARRY_LOCATED ? k_carry_space<1, CARRY_LOCATED>
                                       : (rpe == 1 ? k_carry_space<1, CARRY_NESTED> : rpe == 3 ? k_carry_space<3, CARRY_NESTED> : k_carry_space<18, CARRY_NESTED>);
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)std::max<int64_t>(1, n_blocks)), dim3(BLOCK), 0, dst->stream, a);
    DOTS_HIP(hipGetLastError());
    return 0;
}

}  // namespace dots

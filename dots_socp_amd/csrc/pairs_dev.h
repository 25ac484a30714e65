// Sums carried as unevaluated pairs (hi, lo) with error-free additions, shared by kernels_barycenter.hip and kernels_tangent.hip: a
// sum accumulated this way equals the exactly rounded one to the last bit or the one before it whatever the order of its terms.
#pragma once
#include <hip/hip_runtime.h>

namespace dots {

// s + e == a + b exactly
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
struct DD {
    double hi, lo;
};
__device__ __forceinline__ void dd_add(DD &acc, double x) {
    double s, e;
    two_sum(acc.hi, x, s, e);
    acc.hi = s;
    acc.lo = acc.lo + e;
}
__device__ __forceinline__ void dd_merge(DD &acc, const DD &o) {
    double s, e;
    two_sum(acc.hi, o.hi, s, e);
    acc.hi = s;
    acc.lo = (acc.lo + o.lo) + e;
}
// the wave's pair in lane 0: lane l takes lane l + o for o = 32, 16, ..., 1
__device__ __forceinline__ void dd_wave_fold(DD &s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        DD t;
        t.hi = __shfl_down(s.hi, o, 64);
        t.lo = __shfl_down(s.lo, o, 64);
        dd_merge(s, t);
    }
}

}  // namespace dots

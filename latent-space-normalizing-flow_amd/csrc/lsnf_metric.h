// lsnf_metric.h -- device: the per-row diagonal metric of the HMC steps (include/lsnf_flow_mcmc.h, LSNF_HMC_METRIC_FOLD / _CLOSE), shared
// by the two tails (lsnf_hmc_tail.h, lsnf_rhmc_tail.h).  fp32, the operations and the order of the header, no contraction.
// A lane owns the four columns of a half-unit from load to store, so everything here is lane-local.
#pragma once
#include "lsnf_small3.h"

namespace {
// one rounded product per column: sd * g and sd * qh are formed first (the header's parentheses)
__device__ __forceinline__ f32x4 lsnf_metric_mul(const f32x4& sd, const f32x4& v) {
#pragma clang fp contract(off)
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = sd[j] * v[j];
    return r;
}
// a tail's product at its level (lsnf_hmc_launch.h): without a metric there is no sd and v stays what it is
template <bool METRIC>
__device__ __forceinline__ f32x4 lsnf_metric_mul_if(const f32x4& sd, const f32x4& v) {
    if constexpr (METRIC) return lsnf_metric_mul(sd, v);
    else return v;
}
// Welford's fold of the state x into (mean, m2), in place; n = count + 1, the row's new count
__device__ __forceinline__ void lsnf_metric_fold(f32x4& mean, f32x4& m2, const f32x4& x, float n) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float d = x[j] - mean[j];
        const float mn = mean[j] + d / n;
        m2[j] = m2[j] + d * (x[j] - mn);
        mean[j] = mn;
    }
}
// the scale a window closes with: Stan's regularised variance of the window, as a standard deviation; n < 2 keeps sd's bits.  A
// NaN variance gives scale_min (fmaxf returns its other operand).
__device__ __forceinline__ f32x4 lsnf_metric_close(const f32x4& sd, const f32x4& m2, float n, const LsnfMetricArgs& reg) {
#pragma clang fp contract(off)
    if (!(n >= 2.0f)) return sd;
    const float wn = n / (n + reg.n0), w0 = reg.n0 / (n + reg.n0), nm1 = n - 1.0f;
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float v = wn * (m2[j] / nm1) + reg.var0 * w0;
        r[j] = fminf(fmaxf(sqrtf(v), reg.scale_min), reg.scale_max);
    }
    return r;
}
}  // namespace

// lsnf_temper.h -- device: the likelihood temperature of the tempered HMC steps (include/lsnf_flow_mcmc.h, lsnf_hmc_step_tempered /
// lsnf_reverse_hmc_step_tempered, LSNF_HMC_ANNEAL), shared by the two tails (lsnf_hmc_tail.h, lsnf_rhmc_tail.h).  fp32, the
// operations and the order of the header, no contraction.  A lane owns the four columns of a half-unit from load to store and the
// row scalars are formed by every wave from the same values, so everything here is lane-local.
#pragma once
#include "lsnf_small3.h"

namespace {
// one rounded product per column: beta * gl is formed first (the header's parentheses); 1.0f * x is x, 2^k * x an exact scaling
__device__ __forceinline__ f32x4 lsnf_temper_mul(float beta, const f32x4& v) {
#pragma clang fp contract(off)
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = beta * v[j];
    return r;
}
__device__ __forceinline__ float lsnf_temper_mul(float beta, float v) {
#pragma clang fp contract(off)
    return beta * v;
}
// a tail's product at its level (lsnf_hmc_launch.h): without a temperature there is no beta and v (a quad or a scalar) stays what it is
template <bool TEMPER, class V>
__device__ __forceinline__ V lsnf_temper_mul_if(float beta, const V& v) {
    if constexpr (TEMPER) return lsnf_temper_mul(beta, v);
    else return v;
}
// the re-temper of a kept gradient / potential from beta to beta + d: g_s + (d * gl_s), the product rounded on its own
__device__ __forceinline__ f32x4 lsnf_retemper(const f32x4& gs, float d, const f32x4& gl) {
#pragma clang fp contract(off)
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const float p = d * gl[j]; r[j] = gs[j] + p; }
    return r;
}
__device__ __forceinline__ float lsnf_retemper(float us, float d, float el) {
#pragma clang fp contract(off)
    const float p = d * el;
    return us + p;
}
// the importance weight's increment -(d * el_s) into the row's Kahan pair {w, c}
__device__ __forceinline__ void lsnf_temper_weigh(float& w, float& c, float d, float el) {
#pragma clang fp contract(off)
    const float p = d * el;
    const float inc = -p;
    const float y = inc - c;
    const float t = w + y;
    c = (t - w) - y;
    w = t;
}
}  // namespace

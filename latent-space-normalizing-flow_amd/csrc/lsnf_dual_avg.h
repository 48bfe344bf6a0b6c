// lsnf_dual_avg.h -- device: the dual-averaging update of a row's step size (include/lsnf_flow_mcmc.h, LSNF_HMC_ADAPT), shared by the
// two tails (lsnf_hmc_tail.h, lsnf_rhmc_tail.h) from their ROWS level up.  fp32, the operations and the order of the header, no contraction.
#pragma once
#include "lsnf_small3.h"

namespace {
// ad: the row's {log_step_bar, hbar, count, mu}, updated in place; la: the row's log_alpha (a NaN counts as a rejection); returns the
// row's next step: exp(log_step) of this update or, with last, exp(log_step_bar), the averaged one.  A pure function of its inputs:
// the waves of a workgroup call it with the same numbers and get the same bits.
__device__ __forceinline__ float lsnf_dual_average(f32x4& ad, float la, const LsnfDualAvgArgs& da, bool last) {
#pragma clang fp contract(off)
    const float acc = (la == la) ? fminf(1.0f, expf(la)) : 0.0f;
    const float t = ad[2] + 1.0f, eta = 1.0f / (t + da.t0);
    const float hbar = (1.0f - eta) * ad[1] + eta * (da.target_accept - acc);
    const float ls = fminf(fmaxf(ad[3] - (sqrtf(t) / da.gamma) * hbar, da.log_step_min), da.log_step_max);
    const float w = powf(t, -da.kappa);
    const float lsb = w * ls + (1.0f - w) * ad[0];
    ad[0] = lsb; ad[1] = hbar; ad[2] = t;
    return expf(last ? lsb : ls);
}
}  // namespace

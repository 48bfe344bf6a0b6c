// lsnf_resample.h -- device: the resampling move of the annealing HMC end calls (include/lsnf_flow_mcmc.h, lsnf_hmc_step_resample /
// lsnf_reverse_hmc_step_resample, LSNF_HMC_RESAMPLE), shared by the two tails (lsnf_hmc_tail.h, lsnf_rhmc_tail.h): the
// group's effective sample size, its systematic ancestors and its uniform.  fp32, the operations and the order of the header, no
// contraction.  A group of P <= 16 aligned rows lies inside one wave's 16-row tile (lsnf_exchange.h: a lane is g * 16 + n), so
// rung j's numbers are the registers of lane (lane & 48) | (first tile row of the group + j): every lane of every wave forms the
// sums from the same shuffled values in the same order, as the swap's decision is formed, and writes its own row only.
#pragma once
#include "lsnf_small3.h"
#include "lsnf_exchange.h"

namespace {
// the group's uniform in (0, 1): chain_uniform's number at field value 4 of the noise's counter (the noise draws use 0 and 1, the
// trajectory's uniform 2, the swap's 3), at the global row of the group's first row -- a pure function of (seed, offset, that row)
__device__ __forceinline__ float lsnf_resample_uniform(const LsnfRngState& rs, long long row0, long sample_0) {
    const unsigned long long grow = (unsigned long long)(row0 + sample_0);
    unsigned c0 = 4u << 16, c1 = (unsigned)grow, c2 = rs.c2, c3 = rs.c3hi ^ (unsigned)(grow >> 32);
    lsnf_philox4x32_10(c0, c1, c2, c3, rs.k0, rs.k1);
    return ((float)(c0 >> 8) + 0.5f) * 5.9604644775390625e-08f;
}

struct LsnfResample {
    bool on;        // the group resamples (the same on all its rows)
    int ancestor;   // the rung this row's state comes from; the row's own rung where the group does not resample
    float ess;      // the group's effective sample size
    float lw;       // a resampling group's new log weight, m + logf(S1 / P)
};

// The decision of the group of `P` rows this lane's row lies in.  l: the row's log weight w - c after the increment; u: the group's
// uniform (the same on all its rows); lane: this lane's index in its wave.  To be called where every lane of the wave is active.
// The three loops are rolled on purpose (P is kernel-uniform): one permute in flight at a time, no register per rung.
__device__ __forceinline__ LsnfResample lsnf_resample_decide(float l, float u, int P, float ess_frac, int lane) {
#pragma clang fp contract(off)
    const int k = lane & (P - 1), base = lane - k;                     // the row's rung; the lane of rung 0, the same columns
    const float fp = (float)P;
    float m = lsnf_exchange_take(l, base);
#pragma unroll 1
    for (int j = 1; j < P; ++j) m = fmaxf(m, lsnf_exchange_take(l, base + j));
    const float e = expf(l - m);
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll 1
    for (int j = 0; j < P; ++j) {
        const float ej = lsnf_exchange_take(e, base + j);
        const float q = ej * ej;
        s1 = s1 + ej; s2 = s2 + q;
    }
    LsnfResample r;
    const float ss = s1 * s1;
    r.ess = ss / s2;
    r.on = r.ess < ess_frac * fp;                                      // (a NaN anywhere: false)
    const float ku = (float)k + u;
    const float kp = ku / fp;
    const float tau = kp * s1;
    float cum = 0.0f;
    int cnt = 0;
#pragma unroll 1
    for (int j = 0; j < P; ++j) {
        cum = cum + lsnf_exchange_take(e, base + j);
        cnt += (cum <= tau) ? 1 : 0;
    }
    r.ancestor = r.on ? min(cnt, P - 1) : k;
    const float mean = s1 / fp;
    r.lw = m + logf(mean);
    return r;
}
}  // namespace

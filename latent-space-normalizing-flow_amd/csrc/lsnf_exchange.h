// lsnf_exchange.h -- device: the replica-exchange move of the tempered HMC steps (include/lsnf_flow_mcmc.h, lsnf_hmc_step_exchange /
// lsnf_reverse_hmc_step_exchange, LSNF_HMC_SWAP), shared by the two tails (lsnf_hmc_tail.h, lsnf_rhmc_tail.h): the partner-lane
// rule, the pair's log ratio, its uniform and the cross-lane move.  fp32, the operations and the order of the header, no contraction.
// A lane is g * 16 + n and row n of a 16-row tile is held by lane index n of every column group g and of every wave, so the partner
// of a row of a ladder of R <= 16 aligned rows is another lane of the same wave with the same g: a swap moves registers, and every
// lane keeps writing its own row only.
#pragma once
#include "lsnf_small3.h"

namespace {
// the tile row of row n's partner; n itself for an idle rung.  16 % ladder == 0, so the rung of global row q * 16 + n is n % ladder.
// even: (0,1), (2,3), ..; odd: (1,2), (3,4), .., rungs 0 and ladder - 1 idle (ladder == 2: every rung)
__device__ __forceinline__ int lsnf_exchange_partner(int n, int ladder, bool odd) {
    const int r = n & (ladder - 1);
    if (!odd) return n ^ 1;
    if (r == 0 || r == ladder - 1) return n;
    return (r & 1) ? n + 1 : n - 1;
}
// log_r of the pair (a, b), a the lower row: (beta_a - beta_b) * (el_a - el_b), one rounded product; both rows form it in this order
__device__ __forceinline__ float lsnf_exchange_log_ratio(float beta_a, float beta_b, float el_a, float el_b) {
#pragma clang fp contract(off)
    const float d = beta_a - beta_b, e = el_a - el_b;
    return d * e;
}
// the pair's uniform in (0, 1): chain_uniform's number at field value 3 of the noise's counter (the noise draws use 0 and 1, the
// trajectory's uniform 2), at the global row of the pair's lower row -- a pure function of (seed, offset, that row)
__device__ __forceinline__ float lsnf_exchange_uniform(const LsnfRngState& rs, long long row0, long sample_a) {
    const unsigned long long grow = (unsigned long long)(row0 + sample_a);
    unsigned c0 = 3u << 16, c1 = (unsigned)grow, c2 = rs.c2, c3 = rs.c3hi ^ (unsigned)(grow >> 32);
    lsnf_philox4x32_10(c0, c1, c2, c3, rs.k0, rs.k1);
    return ((float)(c0 >> 8) + 0.5f) * 5.9604644775390625e-08f;
}
// this lane's index in its wave, formed where it is used: the tails sit behind kernels that fill the register file, and a lane index
// kept alive across their stages for the tail's sake is a register they do not have (lsnf_small3_rhmcx_kernel<2, 4, 1>)
__device__ __forceinline__ int lsnf_exchange_lane() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// the partner lane's registers: a variable-source permute (ds_bpermute) for both parities.  To be issued where every lane of the
// wave is active -- a lane masked off returns nothing usable
__device__ __forceinline__ float lsnf_exchange_take(float v, int lane) { return __shfl(v, lane, 64); }
__device__ __forceinline__ f32x4 lsnf_exchange_take(const f32x4& v, int lane) {
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = __shfl(v[j], lane, 64);
    return r;
}
}  // namespace

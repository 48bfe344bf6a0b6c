// lsnf_schedule.h -- device: the schedule search of the annealing HMC calls (include/lsnf_flow_mcmc.h, lsnf_hmc_step_schedule /
// lsnf_reverse_hmc_step_schedule, LSNF_HMC_SCHEDULE), shared by the two tails (lsnf_hmc_tail.h, lsnf_rhmc_tail.h): the group's next
// temperature, the step at which the conditional effective sample size of the incremental weights meets cess_frac, by twelve
// halvings.  fp32, the operations and the order of the header, no contraction.  A group of P <= 16 aligned rows lies inside one
// wave's 16-row tile (lsnf_exchange.h: a lane is g * 16 + n), which is one DPP row of the wave: the group's sums, maximum and
// minimum are xor-butterflies over the lanes lane ^ 1, lane ^ 2, .. lane ^ (P / 2), log2 P exchanges each, and, `+`, fmaxf and fminf
// being commutative, the same bits on every lane of the group.  The exchanges are DPP moves and touch no LDS (the rolled loops of
// lsnf_resample.h pay a ds_bpermute per rung): lane ^ 1 and lane ^ 2 are quad permutes; at the levels 4 and 8 the value is already
// equal on each aligned run of 4 / 8 lanes, so the half-row mirror (lane 7 - i of each 8) and the row mirror (lane 15 - i) hold
// lane ^ 4's and lane ^ 8's value.  Nothing here branches on a group's numbers: the groups of a wave differ in them and every
// exchange needs the whole wave.
#pragma once
#include "lsnf_small3.h"
#include "lsnf_exchange.h"

namespace {
constexpr int LSNF_SCHEDULE_HALVINGS = 12;

// DPP controls: quad_perm [1, 0, 3, 2], quad_perm [2, 3, 0, 1], row_half_mirror, row_mirror
constexpr int LSNF_DPP_XOR1 = 0xB1, LSNF_DPP_XOR2 = 0x4E, LSNF_DPP_HALF_MIRROR = 0x141, LSNF_DPP_MIRROR = 0x140;
template <int CTRL>
__device__ __forceinline__ float lsnf_schedule_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// one butterfly of the group of P rows (kernel-uniform); OP: 0 `+`, 1 fmaxf, 2 fminf
template <int OP>
__device__ __forceinline__ float lsnf_schedule_op(float a, float b) {
#pragma clang fp contract(off)
    return OP == 0 ? a + b : OP == 1 ? fmaxf(a, b) : fminf(a, b);
}
template <int OP>
__device__ __forceinline__ float lsnf_schedule_tree(float x, int P) {
    x = lsnf_schedule_op<OP>(x, lsnf_schedule_dpp<LSNF_DPP_XOR1>(x));
    if (P >= 4) x = lsnf_schedule_op<OP>(x, lsnf_schedule_dpp<LSNF_DPP_XOR2>(x));
    if (P >= 8) x = lsnf_schedule_op<OP>(x, lsnf_schedule_dpp<LSNF_DPP_HALF_MIRROR>(x));
    if (P >= 16) x = lsnf_schedule_op<OP>(x, lsnf_schedule_dpp<LSNF_DPP_MIRROR>(x));
    return x;
}

// cess(x) of the group: W the row's normalised weight, r its likelihood energy above the group's least, S0 the group's sum of W
__device__ __forceinline__ float lsnf_schedule_cess(float x, float W, float r, float S0, int P) {
#pragma clang fp contract(off)
    const float a = x * r;
    const float v = expf(-a);
    const float t = W * v;
    const float q = t * v;
    const float n1 = lsnf_schedule_tree<0>(t, P), n2 = lsnf_schedule_tree<0>(q, P);
    const float nn = n1 * n1, dd = n2 * S0;
    return nn / dd;
}

// beta' of the group of `P` rows this lane's row lies in.  b / cap: the row's beta_rows / beta_next (rung 0's are used); l: the row's
// log weight w - c before the increment; els: el_s of its state after the decision; lane: this lane's index in its wave.  To be
// called where every lane of the wave is active.
__device__ __forceinline__ float lsnf_schedule_next(float b, float cap, float l, float els, int P, float cess_frac, float min_step, int lane) {
#pragma clang fp contract(off)
    const int base = lane & ~(P - 1);                                  // the lane of rung 0, the same columns
    b = lsnf_exchange_take(b, base); cap = lsnf_exchange_take(cap, base);
    const float D = cap - b;
    const float m = lsnf_schedule_tree<1>(l, P), emin = lsnf_schedule_tree<2>(els, P);
    const float W = expf(l - m);
    const float S0 = lsnf_schedule_tree<0>(W, P);
    const float r = els - emin;
    const bool whole = lsnf_schedule_cess(D, W, r, S0, P) >= cess_frac;      // (a NaN anywhere: false)
    float lo = 0.0f, hi = D;
#pragma unroll 1
    for (int it = 0; it < LSNF_SCHEDULE_HALVINGS; ++it) {
        const float sum = lo + hi;
        const float mid = 0.5f * sum;
        const bool ok = lsnf_schedule_cess(mid, W, r, S0, P) >= cess_frac;
        lo = ok ? mid : lo; hi = ok ? hi : mid;
    }
    const float delta = fmaxf(lo, min_step);
    const float stepped = fminf(b + delta, cap);
    return !(D > 0.0f) ? b : (whole ? cap : stepped);
}
}  // namespace

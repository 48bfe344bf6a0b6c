// lsnf_small3_bwd.hip -- latency backward w.r.t. z (+ fused Langevin update) on the bf16 matrix pipe, from the forward's
// activation stash: the partner of lsnf_small3_fwd.hip (workgroups of ST sample tiles of 16 rows, L16 layout, producer-side
// bf16x3 split, weights re-loaded in place one block ahead: lsnf_small3.h units_mma_st).
// Same math and ABI entry points as lsnf_small_bwd.hip's SAVED variant (replaces autograd of train.py:316-329).
//
// Per block, last to first; wave w owns the half-units g_x1[w], g_x2[w] of the running gradient (registers):
//   B4 : g_a2 = (W3s g_t + W3p g_p) * [h2 > 0]   (masks: stash)                          GTP -> GA2
//   B3 : g_a1 = (W2' g_a2) * [h1 > 0]                                                    GA2 -> GA1
//   B2 : g_v1 = g_x1 + W1' g_a1                                                          GA1 -> GV[first half]
//   B1 : g_x  = Wa [g_v1; g_v2]                                                          GV  -> registers
//   CB : s = sigma (stash); g_t = g_v2 = g_y2*s ; g_p = (1-s)(g_y2*y2 + g_l)  of the NEXT block (blk - 1): this wave's own B1
//        output and stash slice, so it runs as B1's epilogue (under the next sample tile's MFMAs) -> GTP, GV[second half, other buffer]
// Four barriers per block.  The transposed matrices come as bf16x3 panels in the 16x16x32 operand order (off_b3b_panels).
// The kernel text itself is lsnf_small3_bwd_kernel.h, which lsnf_small3_mala.hip instantiates a second time with another output section.
#include <stdlib.h>
#include "lsnf_small3.h"
#include "lsnf_launch.h"

#define LSNF_S3B_KERNEL lsnf_small3_bwd_kernel
#define LSNF_S3B_ARGS Small3BwdArgs
#define LSNF_S3B_TAIL
#include "lsnf_small3_bwd_kernel.h"

namespace {
template <class C, int ST>
hipError_t launch_small3_bwd_st(const Small3BwdArgs& a, hipStream_t stream) {
    if constexpr (!small3_bwd_built<C, ST>) {
        return hipErrorInvalidValue;                 // (a selection bug)
    } else {
        const size_t lds = (size_t)Small3BwdLds<C, ST>::L_END * sizeof(float);
        const unsigned grid = lsnf_grid(a.B, ST * S3_SAMPLES);
        return a.dump ? lsnf_launch_kernel<lsnf_small3_bwd_kernel<C, ST, true>>(grid, 256, lds, stream, a)
                      : lsnf_launch_kernel<lsnf_small3_bwd_kernel<C, ST, false>>(grid, 256, lds, stream, a);
    }
}
}  // namespace

// Rows per workgroup (16 x ST) for this call (lsnf_api.hip selects by it): what lsnf_small3_st_wanted asks for; a shape that is
// not instantiated gives way to the next smaller one.  Never 0: the kernel takes every call that brings the activation stash.
int lsnf_small3_backward_st(const LsnfBackwardCall& c) {
    return lsnf_with_cfg<Small3BwdCfg>(c.g, [&](auto cfg) {
        using C = decltype(cfg);
        const int st = lsnf_small3_st_wanted(c.B);
        return (st >= 4 && small3_bwd_built<C, 4>) ? 4 : (st >= 2 && small3_bwd_built<C, 2>) ? 2 : 1;
    });
}

// the backward from the activation stash; st: lsnf_small3_backward_st of the call
hipError_t lsnf_launch_small3_backward_z(const LsnfBackwardCall& c, int st) {
    if (!c.act_saved) return hipErrorInvalidValue;     // (a selection bug)
    Small3BwdArgs a;
    lsnf_fill_backward(a, c);
    a.panels = c.plan + c.g.off_b3b_panels;
    return lsnf_with_cfg<Small3BwdCfg>(c.g, [&](auto cfg) {
        return lsnf_with_st(st, [&](auto s) { return launch_small3_bwd_st<decltype(cfg), decltype(s)::value>(a, c.stream); });
    });
}

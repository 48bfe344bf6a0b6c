// lsnf_small3_rbwd.hip -- backward of the REVERSE (sampling) pass w.r.t. its input, on the bf16 matrix pipe: the sibling of
// lsnf_small3_bwd.hip (workgroups of ST sample tiles of 16 rows, L16 layout, producer-side bf16x3 split, weights re-loaded in
// place one block ahead: lsnf_small3.h units_mma_st).  With f the forward stack, x = f^-1(y) the reverse and
// o_out = o_in - logdet_f(x):   g_y = J_f(x)^-T (g_x - g_o grad_x logdet_f(x)).
// The MLP input of a block is the first half of its forward OUTPUT in both directions (model.py:404,422,426), so sigma and the
// two ReLU masks are the activation stash of lsnf_forward run on x (or lsnf_restash of its block outputs), whichever kernel
// family wrote it.
//
// Per block, FIRST to LAST; wave w owns the half-units g1[w], g2[w] of the running gradient (registers); [y1 | y2] = the block's
// forward output, Winv' = W^-1 diag(exp(-3 logs)) the matrix of the inverse stage I1:
//   T1 : g_v  = Winv' g                              (off_t3b_panels: the transpose of I1)            G   -> registers
//   CB': s = sigma (stash); g_y2 = g_v2 / s ; g_t = -g_v2 ; g_p = -(1 - s)(g_y2 * y2 + g_o): this wave's own T1 output and
//        stash slice, so it runs as T1's epilogue (under the next sample tile's MFMAs)               -> GTP, G[second half, other buffer]
//   B4 : g_a2 = (W3s g_t + W3p g_p) * [h2 > 0]       (off_b3b_panels, masks: stash)                   GTP -> GA2
//   B3 : g_a1 = (W2' g_a2) * [h1 > 0]                                                                 GA2 -> GA1
//   B2 : g_y1 = g_v1 + W1' g_a1                                                                       GA1 -> G[first half]
// Four barriers per block.  Additive coupling: the stash holds sigma = 1 exactly, so g_y2 = g_v2 and g_p = 0.
//
// ONE arithmetic for every lsnf_set_math_mode: bf16x3 is not narrower than fp32, so this kernel also serves LSNF_MATH_FP32 and
// LSNF_MATH_FP16X2.  ONE form for every batch size: above 16 384 rows the grid simply runs more rounds of workgroups;
// lsnf_set_small_batch_max does not affect it.  A row's result does not depend on the batch size or on ST (MFMA columns are
// independent, the split and the coupling arithmetic are compiled without fp contraction).
//
// UPDATE form (lsnf_reverse_langevin_step): the reverse's input y IS the point eps of the base-space Langevin sampler and z_out holds it,
// so the output section becomes  eps_new = eps - 0.5 s^2 (eps + g_y) [+ s xi]  on the registers that hold g_y -- xi from a tensor or
// drawn here (lsnf_device.h lsnf_sample4) --, with optional per-row norms of g_y and eps.  The UPDATE = false code is what it was.
// The kernel text itself is lsnf_small3_rbwd_kernel.h, which lsnf_small3_rmala.hip instantiates a second time with another output section.
#include <stdlib.h>
#include "lsnf_small3.h"
#include "lsnf_launch.h"

#define LSNF_S3R_KERNEL lsnf_small3_rbwd_kernel
#define LSNF_S3R_ARGS std::conditional_t<UPDATE, Small3RlvArgs, Small3RbwdArgs>
#define LSNF_S3R_TAIL
#include "lsnf_small3_rbwd_kernel.h"

namespace {
template <class C, int ST, bool UPDATE, class Args>
hipError_t launch_small3_rbwd_st(const Args& a, hipStream_t stream) {
    if constexpr (!small3_rbwd_built<C, ST>) {
        return hipErrorInvalidValue;                 // (a selection bug)
    } else {
        const size_t lds = (size_t)Small3RbwdLds<C, ST>::L_END * sizeof(float);
        return lsnf_launch_kernel<lsnf_small3_rbwd_kernel<C, ST, UPDATE>>(lsnf_grid(a.B, ST * S3_SAMPLES), 256, lds, stream, a);
    }
}
}  // namespace

// Rows per workgroup (16 x ST) for this call (lsnf_api.hip selects by it): what lsnf_small3_st_wanted asks for; a shape that is
// not instantiated gives way to the next smaller one.  Never 0: the kernel takes every call.
int lsnf_small3_reverse_backward_st(const LsnfReverseBackwardCall& c) {
    return lsnf_with_cfg<Small3RbwdCfg>(c.g, [&](auto cfg) {
        using C = decltype(cfg);
        const int st = lsnf_small3_st_wanted(c.B);
        return (st >= 4 && small3_rbwd_built<C, 4>) ? 4 : (st >= 2 && small3_rbwd_built<C, 2>) ? 2 : 1;
    });
}

// st: lsnf_small3_reverse_backward_st of the call
hipError_t lsnf_launch_small3_reverse_backward_z(const LsnfReverseBackwardCall& c, int st) {
    if (!c.act_saved || !c.g_z_in || c.B < 1) return hipErrorInvalidValue;     // (a selection bug)
    Small3RbwdArgs a;
    a.panels = c.plan + c.g.off_b3b_panels;
    a.tpanels = c.plan + c.g.off_t3b_panels;
    a.z_out = c.z_out; a.z_saved = c.z_saved; a.act_saved = c.act_saved; a.g_x = c.g_x; a.g_obj = c.g_objective; a.g_z_in = c.g_z_in;
    a.B = c.B; a.nz = c.g.nz; a.half = c.g.half; a.depth = c.g.depth; a.vec4 = c.vec4;
    return lsnf_with_cfg<Small3RbwdCfg>(c.g, [&](auto cfg) {
        return lsnf_with_st(st, [&](auto s) { return launch_small3_rbwd_st<decltype(cfg), decltype(s)::value, false>(a, c.stream); });
    });
}

// the same backward with the Langevin update of eps = z_out as its output section; st: lsnf_small3_reverse_backward_st of the call
hipError_t lsnf_launch_small3_reverse_langevin(const LsnfReverseLangevinCall& c, int st) {
    if (!c.act_saved || !c.eps_new || c.B < 1 || (c.noise && c.rng.enabled)) return hipErrorInvalidValue;     // (a selection bug)
    Small3RlvArgs a;
    a.panels = c.plan + c.g.off_b3b_panels;
    a.tpanels = c.plan + c.g.off_t3b_panels;
    a.z_out = c.z_out; a.z_saved = c.z_saved; a.act_saved = c.act_saved; a.g_x = c.grad_g; a.g_obj = nullptr; a.g_z_in = c.g_z_in;
    a.B = c.B; a.nz = c.g.nz; a.half = c.g.half; a.depth = c.g.depth; a.vec4 = c.vec4;
    a.noise = c.noise; a.eps_new = c.eps_new; a.g_norm = c.g_norm; a.eps_norm = c.eps_norm; a.step = c.step; a.rng = c.rng;
    return lsnf_with_cfg<Small3RbwdCfg>(c.g, [&](auto cfg) {
        return lsnf_with_st(st, [&](auto s) { return launch_small3_rbwd_st<decltype(cfg), decltype(s)::value, true>(a, c.stream); });
    });
}

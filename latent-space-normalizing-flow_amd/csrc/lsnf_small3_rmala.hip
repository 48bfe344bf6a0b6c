// lsnf_small3_rmala.hip -- the Metropolis-adjusted Langevin step in the flow's base space (lsnf_reverse_mala_step,
// include/lsnf_flow_mcmc.h): the latency bf16x3 reverse-backward of lsnf_small3_rbwd.hip with the accept / reject tail as its output
// section, as a translation unit of its own (the lsnf_small3_mala.hip arrangement), so that the kernels of lsnf_small3_rbwd.o are
// compiled from the text they always were.
//
// The stages T1 / CB' / B4 / B3 / B2 run at a PROPOSAL eps_prop (= z_out: the reverse's input, the point the stash of x = f^-1(eps_prop)
// belongs to) and leave g = J_{f^-1}(eps_prop)^T grad_g in registers, next to the second half of the rows of eps_prop themselves (the
// last block's y2; the first half, e1, is one more load_row_half in phase 1, in flight with the state's loads -- carried through
// the last block as the UPDATE form carries it, it put the f_width > 64, ST = 1 shape over its 512 registers: 28 B of scratch).  Target pi(eps) ~ exp(-U), U = |eps|^2 / 2 + energy_g, grad U = eps + g.  The output section decides
// the proposal against a kept chain state (eps_acc, grad_acc = grad U(eps_acc), u_acc = U(eps_acc)), updates the state in place and
// proposes again from it.  Two phases around one barrier: (1) every wave with a unit of its own loads its half-units of eps_acc /
// grad_acc, forms t_prop = eps_prop + g (one fp32 add, the `t` of the UPDATE form) in place of g, and leaves its partial row sums of
// A = |coef t_prop - d|^2, Bq = |d + coef grad_acc|^2 (d = eps_prop - eps_acc, coef = s^2 / 2) and |eps_prop|^2 in RED (the dead GTP
// tiles); every wave loads the rows' scalars; (2) every wave adds the four partials of its rows in wave order -- the same numbers in
// the same order, so the four waves decide alike --, forms U_prop = energy_g + |eps_prop|^2 / 2 and
// log_alpha = (u_acc - U_prop) - (A - Bq) / (2 s^2), draws (or has loaded) the row's uniform, and stores its half-units of the state
// (accepted rows only) and of eps_next = fma(s, xi, fma(-coef, grad_state, eps_state)): the UPDATE form's instructions, a loaded and a
// drawn xi through the same ones.  All loads of a workgroup's rows precede the barrier and a lane stores the columns it loaded:
// eps_next may be eps_prop.  The uniform is word 0 of Philox at hh = 2 of the noise's counter (lsnf_device.h), as lsnf_mala_step's.
#include <stdlib.h>
#include "lsnf_small3.h"
#include "lsnf_launch.h"

namespace {
// The output section of the MALA form: a: Small3RmalaArgs; g1 / g2: this wave's half-units of g, replaced by t_prop = eps_prop + g;
// y2: its second-half unit of eps_prop; the rest: the kernel's locals of the same names.
template <int HT, int ST, class A>
__device__ __forceinline__ void small3_rmala_tail(const A& a, f32x4 (&g1)[ST], f32x4 (&g2)[ST], const f32x4 (&y2)[ST],
                                                  const long (&sample)[ST], const bool (&live)[ST], const long (&row)[ST], float* RED,
                                                  bool has1, int nt1, int ft1, int wave, int g, int n, int vec4) {
#pragma clang fp contract(off)
    const bool init = (a.flags & 1u) != 0;                             // kernel-uniform
    const LsnfRngState rs = a.rng.enabled ? lsnf_rng_state(a.rng) : LsnfRngState{0u, 0u, 0u, 0u, 0};
    const float coef = __fmul_rn(__fmul_rn(0.5f, a.step), a.step);
    f32x4 e1[ST], ea[ST][2], ga[ST][2];                               // e1: the first half of this wave's unit of eps_prop (the second is y2)
    float en_g[ST], u_old[ST], uni[ST];                               // per row; read before the barrier: wave 0 stores u_acc after it
    // phase 1: this wave's half-units of the rows, its partial sums into RED
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        float sa = 0.0f, sb = 0.0f, se = 0.0f;
        en_g[st] = a.energy_g ? a.energy_g[row[st]] : 0.0f;
        u_old[st] = init ? 0.0f : a.u_acc[row[st]];
        uni[st] = (a.uniform && !init) ? a.uniform[row[st]] : 0.5f;
        e1[st] = load_row_half<HT>(nt1, ft1, a.z_out + row[st] * (long)a.nz, a.half, g, vec4);
#pragma unroll
        for (int hs = 0; hs < 2; ++hs) {
            const int t = hs * HT + nt1;
            const long ro = row[st] * (long)a.nz;
            ea[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f}; ga[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!init && has1) {                                       // (a wave without a unit repeats unit 0: counted once, by wave 0)
                ea[st][hs] = load_row_half<HT>(t, ft1, a.eps_acc + ro, a.half, g, vec4);
                ga[st][hs] = load_row_half<HT>(t, ft1, a.grad_acc + ro, a.half, g, vec4);
            }
            const f32x4 ec = hs ? y2[st] : e1[st];
            f32x4& tp = hs ? g2[st] : g1[st];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                tp[r] = __fadd_rn(ec[r], tp[r]);                        // t_prop = eps_prop + g
                const float d = ec[r] - ea[st][hs][r];
                const float fa = coef * tp[r] - d, fb = d + coef * ga[st][hs][r];
                sa += fa * fa; sb += fb * fb; se += ec[r] * ec[r];
            }
        }
        if (!has1) { sa = 0.0f; sb = 0.0f; se = 0.0f; }
        sa = group_sum(sa); sb = group_sum(sb); se = group_sum(se);
        if (g == 0) {
            float* slot = RED + ((st * 4 + wave) * 16 + n) * 3;
            slot[0] = sa; slot[1] = sb; slot[2] = se;
        }
    }
    __syncthreads();
    // phase 2: every wave decides its rows (the same sums in the same order: the same decision), then stores its half-units
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        float s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float* slot = RED + ((st * 4 + w) * 16 + n) * 3;
            s1 += slot[0]; s2 += slot[1]; s3 += slot[2];
        }
        const float u_prop = en_g[st] + 0.5f * s3;
        float la = 0.0f;
        bool acc = true;
        if (!init) {
            la = (u_old[st] - u_prop) - (s1 - s2) / (2.0f * a.step * a.step);
            float u = uni[st];
            if (!a.uniform) {
                const unsigned long long grow = (unsigned long long)(a.rng.row0 + sample[st]);
                unsigned c0 = 2u << 16, c1 = (unsigned)grow, c2 = rs.c2, c3 = rs.c3hi ^ (unsigned)(grow >> 32);
                lsnf_philox4x32_10(c0, c1, c2, c3, rs.k0, rs.k1);
                u = ((float)(c0 >> 8) + 0.5f) * 5.9604644775390625e-08f;
            }
            acc = logf(u) < la;                                        // (a NaN log_alpha rejects)
        }
        if (has1 && live[st]) {
#pragma unroll
            for (int hs = 0; hs < 2; ++hs) {
                const int t = hs * HT + nt1;
                const long so = sample[st] * (long)a.nz;
                const f32x4 ec = hs ? y2[st] : e1[st];
                const f32x4 tp = hs ? g2[st] : g1[st];
                if (acc) {
                    store_row_half<HT>(t, ft1, ec, a.eps_acc + so, a.half, g, vec4);
                    store_row_half<HT>(t, ft1, tp, a.grad_acc + so, a.half, g, vec4);
                }
                if (a.eps_new) {
                    const f32x4 es = acc ? ec : ea[st][hs], gs = acc ? tp : ga[st][hs];
                    f32x4 xi = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (a.noise) {
                        xi = load_row_half<HT>(t, ft1, a.noise + row[st] * (long)a.nz, a.half, g, vec4);
                    } else if (rs.on) {     // the UPDATE form's draw (lsnf_device.h): lsnf_sample's eps at temperature 1
                        float unused = 0.0f;
                        xi = lsnf_sample4(hs, 32 * nt1 + 16 * ft1 + 4 * g, a.half, (unsigned long long)(a.rng.row0 + sample[st]), rs, 1.0f, unused);
                    }
                    f32x4 en;
#pragma unroll
                    for (int r = 0; r < 4; ++r) en[r] = __fmaf_rn(a.step, xi[r], __fmaf_rn(-coef, gs[r], es[r]));
                    store_row_half<HT>(t, ft1, en, a.eps_new + so, a.half, g, vec4);
                }
            }
        }
        if (wave == 0 && g == 0 && live[st]) {
            if (acc) a.u_acc[sample[st]] = u_prop;
            if (a.accept_out) a.accept_out[sample[st]] = acc ? 1.0f : 0.0f;
            if (a.log_alpha_out) a.log_alpha_out[sample[st]] = la;
        }
    }
}
}  // namespace

#define LSNF_S3R_KERNEL lsnf_small3_rmala_kernel
#define LSNF_S3R_ARGS Small3RmalaArgs
#define LSNF_S3R_TAIL small3_rmala_tail<HT, ST>(a, g1, g2, y2, sample, live, row, GTP, has1, nt1, ft1, wave, g, n, vec4); return;
#include "lsnf_small3_rbwd_kernel.h"

namespace {
// three partial row sums per wave and row in the g_t | g_p tiles, which are dead after the last block's barrier
static_assert(4 * 16 * 3 <= Small3RbwdLds<Small3RbwdCfg<1, 1>, 1>::TP, "the partial sums of the MALA tail live in GTP (HT = 1, ST = 1)");
template <class C, int ST>
hipError_t launch_small3_rmala_st(const Small3RmalaArgs& a, hipStream_t stream) {
    if constexpr (!small3_rbwd_built<C, ST>) {
        return hipErrorInvalidValue;                 // (a selection bug)
    } else {
        const size_t lds = (size_t)Small3RbwdLds<C, ST>::L_END * sizeof(float);
        return lsnf_launch_kernel<lsnf_small3_rmala_kernel<C, ST, false>>(lsnf_grid(a.B, ST * S3_SAMPLES), 256, lds, stream, a);
    }
}
}  // namespace

// the MALA form (lsnf_reverse_mala_step): the same stages, the accept / reject tail as the output section; st:
// lsnf_small3_reverse_backward_st of the call
hipError_t lsnf_launch_small3_reverse_mala(const LsnfReverseMalaCall& c, int st) {
    if (!c.act_saved || !c.chain.acc || !c.chain.grad_acc || !c.chain.u_acc || c.g_z_in || c.g_norm || c.eps_norm || c.B < 1 ||
        (c.rng.enabled && (c.noise || c.chain.uniform)))
        return hipErrorInvalidValue;                    // (a selection bug)
    Small3RmalaArgs a;
    a.panels = c.plan + c.g.off_b3b_panels;
    a.tpanels = c.plan + c.g.off_t3b_panels;
    a.z_out = c.z_out; a.z_saved = c.z_saved; a.act_saved = c.act_saved; a.g_x = c.grad_g; a.g_obj = nullptr; a.g_z_in = nullptr;
    a.B = c.B; a.nz = c.g.nz; a.half = c.g.half; a.depth = c.g.depth; a.vec4 = c.vec4;
    a.noise = c.noise; a.eps_new = c.eps_new; a.g_norm = nullptr; a.eps_norm = nullptr; a.step = c.step; a.rng = c.rng;
    a.eps_acc = c.chain.acc;
    lsnf_fill_chain(a, c.chain);
    return lsnf_with_cfg<Small3RbwdCfg>(c.g, [&](auto cfg) {
        return lsnf_with_st(st, [&](auto s) { return launch_small3_rmala_st<decltype(cfg), decltype(s)::value>(a, c.stream); });
    });
}

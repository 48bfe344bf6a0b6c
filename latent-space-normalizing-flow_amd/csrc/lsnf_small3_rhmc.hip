// lsnf_small3_rhmc.hip -- Hamiltonian Monte Carlo in the flow's base space (lsnf_reverse_hmc_step, include/lsnf_flow_mcmc.h): the
// latency bf16x3 reverse-backward of lsnf_small3_rbwd.hip with a leapfrog tail as its output section, as a translation unit of its
// own (the lsnf_small3_rmala.hip arrangement), so that the kernels of lsnf_small3_rbwd.o and lsnf_small3_rmala.o are compiled from the
// text they always were.
//
// The stages T1 / CB' / B4 / B3 / B2 run at a point eps_prop of a trajectory (= z_out: the reverse's input, the point the stash of
// x = f^-1(eps_prop) belongs to) and leave g = J_{f^-1}(eps_prop)^T grad_g in registers, next to the second half of the rows of
// eps_prop (the last block's y2; the first half, e1, is one more load_row_half in the tail, as in lsnf_small3_rmala.hip and for its
// reason).  Target pi(eps) ~ exp(-U), U = |eps|^2 / 2 + energy_g, grad U = eps + g.  Every phase forms t_prop = eps_prop + g (one fp32
// add: lsnf_reverse_mala_step's grad_acc) in place of g; the phase is a kernel-uniform branch:
//   INNER        a leapfrog step inside a trajectory: ph = mom - s t_prop, eps_next = eps_prop + s ph, mom <- ph.  Per lane and
//                column: no cross-wave sum, no barrier; a lane stores the columns it loaded, so eps_next may be eps_prop.
//   INIT / end   two phases around one barrier, as the MALA tail.  (1) every wave with a unit of its own loads its half-units of mom /
//                eps_acc / grad_acc, draws or loads its half-units of xi (xi does not depend on the decision) and leaves its partial
//                row sums of sum pL^2 (pL = mom - (s/2) t_prop), sum xi^2 and sum eps_prop^2 in the three RED slots per row and wave
//                (the dead GTP tiles); every wave loads the rows' scalars; (2) every wave adds the four partials of its rows in wave
//                order -- the same numbers in the same order, so the four waves decide alike --, forms U_prop = energy_g +
//                |eps_prop|^2 / 2 and log_alpha = (u_acc - U_prop) + (kin0 - kinL), draws (or has loaded) the row's uniform, and stores
//                its half-units of the state (accepted rows only) and of the next trajectory's first half-kick ph = xi - (s/2) t_state,
//                eps_next = eps_state + s ph, mom <- ph.  Wave 0 stores the row scalars (u_acc, kin0, accept_out, log_alpha_out).  All
//                loads of a workgroup's rows precede the barrier and a lane stores the columns it loaded.
// sum eps_prop^2 is accumulated as lsnf_small3_rmala.hip accumulates it (an INIT call writes that kernel's INIT state bit for bit), the
// other two sums as lsnf_small3_hmc.hip's.  The uniform is lsnf_mala_step's (word 0 of Philox at hh = 2 of the noise's counter), xi
// lsnf_reverse_mala_step's draw (lsnf_sample's eps at temperature 1: a padding column, beyond nz / 2 of its half, is 0 and so not
// counted in sum xi^2).  Everything here is fp32 without fp contraction.
#include <stdlib.h>
#include "lsnf_small3.h"
#include "lsnf_launch.h"

namespace {
// The output section of the base-space HMC form: a: Small3RhmcArgs; g1 / g2: this wave's half-units of g, replaced by
// t_prop = eps_prop + g; y2: its second-half unit of eps_prop; the rest: the kernel's locals of the same names.
template <int HT, int ST, class A>
__device__ __forceinline__ void small3_rhmc_tail(const A& a, f32x4 (&g1)[ST], f32x4 (&g2)[ST], const f32x4 (&y2)[ST],
                                                 const long (&sample)[ST], const bool (&live)[ST], const long (&row)[ST], float* RED,
                                                 bool has1, int nt1, int ft1, int wave, int g, int n, int vec4) {
#pragma clang fp contract(off)
    const bool init = (a.flags & 1u) != 0, inner = (a.flags & 2u) != 0;      // kernel-uniform
    const float s = a.step, hs2 = 0.5f * a.step;
    if (inner) {                                                       // ---- a leapfrog step inside a trajectory ----
        if (!has1) return;
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            const long ro = row[st] * (long)a.nz, so = sample[st] * (long)a.nz;
            const f32x4 e1 = load_row_half<HT>(nt1, ft1, a.z_out + ro, a.half, g, vec4);
#pragma unroll
            for (int hs = 0; hs < 2; ++hs) {
                const int t = hs * HT + nt1;
                const f32x4 pm = load_row_half<HT>(t, ft1, a.mom + ro, a.half, g, vec4);
                const f32x4 ec = hs ? y2[st] : e1;
                const f32x4 gq = hs ? g2[st] : g1[st];
                f32x4 ph, en;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float tp = __fadd_rn(ec[r], gq[r]);          // t_prop = eps_prop + g
                    ph[r] = pm[r] - s * tp;
                    en[r] = ec[r] + s * ph[r];
                }
                if (live[st]) {
                    store_row_half<HT>(t, ft1, ph, a.mom + so, a.half, g, vec4);
                    store_row_half<HT>(t, ft1, en, a.eps_new + so, a.half, g, vec4);
                }
            }
        }
        return;
    }
    // ---- INIT / end of a trajectory ----
    const LsnfRngState rs = a.rng.enabled ? lsnf_rng_state(a.rng) : LsnfRngState{0u, 0u, 0u, 0u, 0};
    f32x4 e1[ST], ea[ST][2], ga[ST][2], xi[ST][2];                     // e1: the first half of this wave's unit of eps_prop (the second is y2)
    float en_g[ST], u_old[ST], k_old[ST], uni[ST];                     // per row; read before the barrier: wave 0 stores u_acc / kin0 after it
    // phase 1: this wave's half-units of the rows, its partial sums into RED
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        float sl = 0.0f, sx = 0.0f, se = 0.0f;
        en_g[st] = a.energy_g ? a.energy_g[row[st]] : 0.0f;
        u_old[st] = init ? 0.0f : a.u_acc[row[st]];
        k_old[st] = init ? 0.0f : a.kin0[row[st]];
        uni[st] = (a.uniform && !init) ? a.uniform[row[st]] : 0.5f;
        e1[st] = load_row_half<HT>(nt1, ft1, a.z_out + row[st] * (long)a.nz, a.half, g, vec4);
#pragma unroll
        for (int hs = 0; hs < 2; ++hs) {
            const int t = hs * HT + nt1;
            const long ro = row[st] * (long)a.nz;
            ea[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f}; ga[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 pm = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!init && has1) {                                       // (a wave without a unit repeats unit 0: counted once, by wave 0)
                ea[st][hs] = load_row_half<HT>(t, ft1, a.eps_acc + ro, a.half, g, vec4);
                ga[st][hs] = load_row_half<HT>(t, ft1, a.grad_acc + ro, a.half, g, vec4);
                pm = load_row_half<HT>(t, ft1, a.mom + ro, a.half, g, vec4);
            }
            xi[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.eps_new && has1)          // (lsnf_reverse_mala_step's draw)
                xi[st][hs] = chain_xi<HT>(a.noise, rs, a.rng.row0, a.nz, a.half, hs, nt1, ft1, g, row[st], sample[st], vec4);
            const f32x4 ec = hs ? y2[st] : e1[st];
            f32x4& tp = hs ? g2[st] : g1[st];
            f32x4 pl;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                tp[r] = __fadd_rn(ec[r], tp[r]);                        // t_prop = eps_prop + g
                pl[r] = pm[r] - hs2 * tp[r];
                sl += pl[r] * pl[r]; se += ec[r] * ec[r];
                sx += xi[st][hs][r] * xi[st][hs][r];
            }
            // nothing is proposed: the full-step momentum at the proposal is left readable (this lane loaded these columns)
            if (!init && !a.eps_new && has1 && live[st]) store_row_half<HT>(t, ft1, pl, a.mom + sample[st] * (long)a.nz, a.half, g, vec4);
        }
        if (!has1) { sl = 0.0f; sx = 0.0f; se = 0.0f; }
        sl = group_sum(sl); sx = group_sum(sx); se = group_sum(se);
        if (g == 0) {
            float* slot = RED + ((st * 4 + wave) * 16 + n) * 3;
            slot[0] = sl; slot[1] = sx; slot[2] = se;
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
            const float kin_l = 0.5f * s1;
            la = (u_old[st] - u_prop) + (k_old[st] - kin_l);
            float u = uni[st];
            if (!a.uniform) u = chain_uniform(rs, a.rng.row0, sample[st]);
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
                if (a.eps_new) {                                       // begin the next trajectory from the (updated) state
                    const f32x4 es = acc ? ec : ea[st][hs], gs = acc ? tp : ga[st][hs];
                    f32x4 ph, en;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        ph[r] = xi[st][hs][r] - hs2 * gs[r];
                        en[r] = es[r] + s * ph[r];
                    }
                    store_row_half<HT>(t, ft1, ph, a.mom + so, a.half, g, vec4);
                    store_row_half<HT>(t, ft1, en, a.eps_new + so, a.half, g, vec4);
                }
            }
        }
        if (wave == 0 && g == 0 && live[st]) {
            if (acc) a.u_acc[sample[st]] = u_prop;
            if (a.eps_new) a.kin0[sample[st]] = 0.5f * s2;
            if (a.accept_out) a.accept_out[sample[st]] = acc ? 1.0f : 0.0f;
            if (a.log_alpha_out) a.log_alpha_out[sample[st]] = la;
        }
    }
}
}  // namespace

#define LSNF_S3R_KERNEL lsnf_small3_rhmc_kernel
#define LSNF_S3R_ARGS Small3RhmcArgs
#define LSNF_S3R_TAIL small3_rhmc_tail<HT, ST>(a, g1, g2, y2, sample, live, row, GTP, has1, nt1, ft1, wave, g, n, vec4); return;
#include "lsnf_small3_rbwd_kernel.h"

namespace {
// three partial row sums per wave and row in the g_t | g_p tiles, which are dead after the last block's barrier
static_assert(4 * 16 * 3 <= Small3RbwdLds<Small3RbwdCfg<1, 1>, 1>::TP, "the partial sums of the HMC tail live in GTP (HT = 1, ST = 1)");
template <class C, int ST>
hipError_t launch_small3_rhmc_st(const Small3RhmcArgs& a, hipStream_t stream) {
    if constexpr (!small3_rbwd_built<C, ST>) {
        return hipErrorInvalidValue;                 // (a selection bug)
    } else {
        const size_t lds = (size_t)Small3RbwdLds<C, ST>::L_END * sizeof(float);
        return lsnf_launch_kernel<lsnf_small3_rhmc_kernel<C, ST, false>>(lsnf_grid(a.B, ST * S3_SAMPLES), 256, lds, stream, a);
    }
}
}  // namespace

// the base-space HMC form (lsnf_reverse_hmc_step): the same stages, the leapfrog tail as the output section; st:
// lsnf_small3_reverse_backward_st of the call
hipError_t lsnf_launch_small3_reverse_hmc(const LsnfReverseHmcCall& c, int st) {
    const bool inner = (c.chain.flags & 2u) != 0;
    if (!c.act_saved || !c.chain.acc || !c.chain.grad_acc || !c.chain.u_acc || c.g_z_in || c.g_norm || c.eps_norm || c.B < 1 ||
        !c.mom || !c.kin0 || (c.rng.enabled && (c.noise || c.chain.uniform)) || (!inner && c.eps_new && !c.noise && !c.rng.enabled) ||
        (inner && (!c.eps_new || c.noise || c.chain.uniform || c.rng.enabled || (c.chain.flags & 1u))))
        return hipErrorInvalidValue;                    // (a selection bug)
    Small3RhmcArgs a;
    a.panels = c.plan + c.g.off_b3b_panels;
    a.tpanels = c.plan + c.g.off_t3b_panels;
    a.z_out = c.z_out; a.z_saved = c.z_saved; a.act_saved = c.act_saved; a.g_x = c.grad_g; a.g_obj = nullptr; a.g_z_in = nullptr;
    a.B = c.B; a.nz = c.g.nz; a.half = c.g.half; a.depth = c.g.depth; a.vec4 = c.vec4;
    a.noise = c.noise; a.eps_new = c.eps_new; a.g_norm = nullptr; a.eps_norm = nullptr; a.step = c.step; a.rng = c.rng;
    a.eps_acc = c.chain.acc;
    lsnf_fill_chain(a, c.chain);
    a.mom = c.mom; a.kin0 = c.kin0;
    return lsnf_with_cfg<Small3RbwdCfg>(c.g, [&](auto cfg) {
        return lsnf_with_st(st, [&](auto s) { return launch_small3_rhmc_st<decltype(cfg), decltype(s)::value>(a, c.stream); });
    });
}

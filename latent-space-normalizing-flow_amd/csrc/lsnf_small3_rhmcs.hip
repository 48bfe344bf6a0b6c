// lsnf_small3_rhmcs.hip -- Hamiltonian Monte Carlo in the flow's base space with a likelihood temperature per row and a resampling
// move between the rows of a group on an annealing end call (lsnf_reverse_hmc_step_resample, include/lsnf_flow_mcmc.h): the kernel
// text of lsnf_small3_rbwd_kernel.h with the tempered leapfrog tail of lsnf_small3_rhmct.hip, as a translation unit of its own, so that
// the kernels of lsnf_small3_rhmct.o and lsnf_small3_rhmcx.o are compiled from the text they always were.  The tail is
// lsnf_small3_rhmct.hip's, statement for statement, with the differences of lsnf_small3_hmcs.hip:
//   RESAMPLE     (flags & 512, end calls with ANNEAL and without ADAPT / FOLD / CLOSE, kernel-uniform) every lane of every wave forms
//                its row's new Kahan pair and re-tempered potential and the group's decision (lsnf_resample.h); the per-quad loop
//                is entered by the whole wave with the row's loads and stores under live[st], and inside it the ancestor's es, gs,
//                gls of the same columns come over by ds_bpermute; a row whose ancestor is another row stores the ancestor's es /
//                gls / els and its gs / us re-tempered to the row's own beta_next over what the update stored, and the next
//                trajectory begins from them.
//   resample_uniform (B) read at the group's first row where the decision is formed, or drawn in-kernel at counter field 4 of that row.
// Without RESAMPLE a row's outputs are lsnf_small3_rhmct_kernel's bit for bit in every phase.  Everything here is fp32 without fp
// contraction.
#include <stdlib.h>
#include "lsnf_small3.h"
#include "lsnf_dual_avg.h"
#include "lsnf_metric.h"
#include "lsnf_temper.h"
#include "lsnf_exchange.h"
#include "lsnf_resample.h"
#include "lsnf_launch.h"

namespace {
// The output section of the resampling base-space HMC form: a: Small3RhmcResampleArgs; g1 / g2: this wave's half-units of g (kept:
// gl); y2: its second-half unit of eps_prop; the rest: the kernel's locals of the same names.
template <int HT, int ST, class A>
__device__ __forceinline__ void small3_rhmcs_tail(const A& a, f32x4 (&g1)[ST], f32x4 (&g2)[ST], const f32x4 (&y2)[ST],
                                                  const long (&sample)[ST], const bool (&live)[ST], const long (&row)[ST], float* RED,
                                                  bool has1, int nt1, int ft1, int wave, int g, int n, int vec4) {
#pragma clang fp contract(off)
    const bool init = (a.flags & 1u) != 0, inner = (a.flags & 2u) != 0, adapt = (a.flags & 4u) != 0;      // kernel-uniform
    const bool fold = (a.flags & 16u) != 0, close = (a.flags & 32u) != 0, anneal = (a.flags & 64u) != 0;
    const bool resample = (a.flags & 512u) != 0;
    const int P = resample ? a.group : 1;                              // the group's length (RESAMPLE)
    const int xlane = lsnf_exchange_lane(), rk = xlane & (P - 1);      // the row's rung: 16 % P == 0, so it is (global row) % P
    float s[ST], hs2[ST], bt[ST];                                      // per row: fixed before the momentum is drawn, constant in a trajectory
#pragma unroll
    for (int st = 0; st < ST; ++st) { s[st] = a.step_rows[row[st]]; hs2[st] = 0.5f * s[st]; bt[st] = a.beta_rows[row[st]]; }
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
                const f32x4 sd = load_row_half<HT>(t, ft1, a.scale + ro, a.half, g, vec4);
                const f32x4 ec = hs ? y2[st] : e1;
                const f32x4 bg = lsnf_temper_mul(bt[st], hs ? g2[st] : g1[st]);
                f32x4 tp, ph, en;
#pragma unroll
                for (int r = 0; r < 4; ++r) tp[r] = __fadd_rn(ec[r], bg[r]);      // t_prop = eps_prop + (beta * g)
                const f32x4 sg = lsnf_metric_mul(sd, tp);
#pragma unroll
                for (int r = 0; r < 4; ++r) ph[r] = pm[r] - s[st] * sg[r];
                const f32x4 sq = lsnf_metric_mul(sd, ph);
#pragma unroll
                for (int r = 0; r < 4; ++r) en[r] = ec[r] + s[st] * sq[r];
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
    float en_g[ST], u_old[ST], k_old[ST], uni[ST], cnt[ST];            // per row; read before the barrier: wave 0 stores u_acc / kin0 / count after it
    float el_old[ST], bn[ST], lw[ST], lc[ST];                          // likewise like_u_acc, beta_next and the Kahan pair
    f32x4 ad[ST];                                                      // likewise the rows' {log_step_bar, hbar, count, mu}
    // phase 1: this wave's half-units of the rows, its partial sums into RED
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        float sl = 0.0f, sx = 0.0f, se = 0.0f;
        en_g[st] = a.energy_g ? a.energy_g[row[st]] : 0.0f;
        u_old[st] = init ? 0.0f : a.u_acc[row[st]];
        k_old[st] = init ? 0.0f : a.kin0[row[st]];
        uni[st] = (a.uniform && !init) ? a.uniform[row[st]] : 0.5f;
        cnt[st] = fold ? a.count[row[st]] : 0.0f;
        el_old[st] = (anneal && !init) ? a.like_u_acc[row[st]] : 0.0f;
        bn[st] = anneal ? a.beta_next[row[st]] : 0.0f;
        lw[st] = 0.0f; lc[st] = 0.0f;
        if (anneal) { const float2 p = reinterpret_cast<const float2*>(a.log_w)[row[st]]; lw[st] = p.x; lc[st] = p.y; }
        ad[st] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (adapt) ad[st] = reinterpret_cast<const f32x4*>(a.adapt)[row[st]];
        e1[st] = load_row_half<HT>(nt1, ft1, a.z_out + row[st] * (long)a.nz, a.half, g, vec4);
#pragma unroll
        for (int hs = 0; hs < 2; ++hs) {
            const int t = hs * HT + nt1;
            const long ro = row[st] * (long)a.nz;
            ea[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f}; ga[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 pm = f32x4{0.f, 0.f, 0.f, 0.f}, sd = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!init && has1) {                                       // (a wave without a unit repeats unit 0: counted once, by wave 0)
                ea[st][hs] = load_row_half<HT>(t, ft1, a.eps_acc + ro, a.half, g, vec4);
                ga[st][hs] = load_row_half<HT>(t, ft1, a.grad_acc + ro, a.half, g, vec4);
                pm = load_row_half<HT>(t, ft1, a.mom + ro, a.half, g, vec4);
                sd = load_row_half<HT>(t, ft1, a.scale + ro, a.half, g, vec4);
            }
            xi[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.eps_new && has1)          // (lsnf_reverse_mala_step's draw)
                xi[st][hs] = chain_xi<HT>(a.noise, rs, a.rng.row0, a.nz, a.half, hs, nt1, ft1, g, row[st], sample[st], vec4);
            const f32x4 ec = hs ? y2[st] : e1[st];
            const f32x4 bg = lsnf_temper_mul(bt[st], hs ? g2[st] : g1[st]);
            f32x4 tp;
#pragma unroll
            for (int r = 0; r < 4; ++r) tp[r] = __fadd_rn(ec[r], bg[r]);            // t_prop = eps_prop + (beta * g)
            const f32x4 sg = lsnf_metric_mul(sd, tp);
            f32x4 pl;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pl[r] = pm[r] - hs2[st] * sg[r];
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
    // phase 2: every wave decides its rows (the same sums in the same order: the same decision, the same new step), then stores its
    // half-units
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        float s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float* slot = RED + ((st * 4 + w) * 16 + n) * 3;
            s1 += slot[0]; s2 += slot[1]; s3 += slot[2];
        }
        const float u_prop = lsnf_temper_mul(bt[st], en_g[st]) + 0.5f * s3;
        float la = 0.0f;
        bool acc = true;
        if (!init) {
            const float kin_l = 0.5f * s1;
            la = (u_old[st] - u_prop) + (k_old[st] - kin_l);
            float u = uni[st];
            if (!a.uniform) u = chain_uniform(rs, a.rng.row0, sample[st]);
            acc = logf(u) < la;                                        // (a NaN log_alpha rejects)
        }
        float sn = s[st], hn = hs2[st];                                // the step of the trajectory this call begins
        if (adapt) {
            sn = lsnf_dual_average(ad[st], la, a.da, (a.flags & 8u) != 0);
            hn = 0.5f * sn;
            if (close && !(a.flags & 8u)) ad[st] = f32x4{0.f, 0.f, 0.f, logf(10.0f * sn)};      // the window's end restarts the averaging
        }
        const float nf = cnt[st] + 1.0f;                               // the row's count after the fold
        const float d = bn[st] - bt[st];                               // (ANNEAL) the change of the row's temperature
        float ep = 0.0f, uf = 0.0f, dn = 0.0f;                          // (RESAMPLE) the ancestor's el_s, its u_s at this row's beta_next, beta_next - its beta_next
        int al = xlane;                                                // the ancestor's lane: the same wave, the same columns
        if (resample) {                                                // the group's decision: the whole wave is active here
            const float els = acc ? en_g[st] : el_old[st];
            const float us = lsnf_retemper(acc ? u_prop : u_old[st], d, els);      // what the ANNEAL lines below store, formed by every lane
            float nw = lw[st], nc = lc[st];
            lsnf_temper_weigh(nw, nc, d, els);
            // the group's uniform, read here and not in front of the barrier: held across it, it is a register that
            // lsnf_small3_rhmcs_kernel<2, 4, 1> does not have (12 bytes of scratch); (B >= group: row - rk is in bounds)
            const float u = a.resample_uniform ? a.resample_uniform[row[st] - rk] : lsnf_resample_uniform(rs, a.rng.row0, sample[st] - rk);
            const LsnfResample rv = lsnf_resample_decide(nw - nc, u, P, a.ess_frac, xlane);
            al = xlane - rk + rv.ancestor;
            const float ba = lsnf_exchange_take(bn[st], al), up = lsnf_exchange_take(us, al);
            ep = lsnf_exchange_take(els, al);
            dn = bn[st] - ba;                                          // the ancestor's state comes to this row's temperature
            uf = lsnf_retemper(up, dn, ep);
            lw[st] = rv.on ? rv.lw : nw; lc[st] = rv.on ? 0.0f : nc;   // the pair the ANNEAL lines below store (they do not weigh again)
            if (wave == 0 && g == 0 && live[st]) {                     // (stored here: nothing of the decision but al stays live)
                if (a.ancestor_out) a.ancestor_out[sample[st]] = (float)rv.ancestor;
                if (a.ess_out) a.ess_out[sample[st]] = rv.ess;
            }
        }
        const bool moved = al != xlane;
        if (has1) {                                                    // (wave-uniform: the move below needs the whole wave)
#pragma unroll
            for (int hs = 0; hs < 2; ++hs) {
                const int t = hs * HT + nt1;
                const long so = sample[st] * (long)a.nz;
                f32x4 es = f32x4{0.f, 0.f, 0.f, 0.f}, gs = es, gls = es, sd = es;      // (a dead row's: zeros nobody uses)
                if (live[st]) {
                    const f32x4 ec = hs ? y2[st] : e1[st];
                    gls = hs ? g2[st] : g1[st];                         // gl of the state after the decision: g, or the kept one
                    const f32x4 bg = lsnf_temper_mul(bt[st], gls);
                    f32x4 tp;
#pragma unroll
                    for (int r = 0; r < 4; ++r) tp[r] = __fadd_rn(ec[r], bg[r]);        // t_prop again: phase 1's bits
                    es = acc ? ec : ea[st][hs];                         // the state after the decision
                    if (acc) {
                        store_row_half<HT>(t, ft1, ec, a.eps_acc + so, a.half, g, vec4);
                        store_row_half<HT>(t, ft1, gls, a.like_grad_acc + so, a.half, g, vec4);
                        if (!anneal) store_row_half<HT>(t, ft1, tp, a.grad_acc + so, a.half, g, vec4);
                    } else if (anneal) {
                        gls = load_row_half<HT>(t, ft1, a.like_grad_acc + so, a.half, g, vec4);      // (live: so is the row's own offset)
                    }
                    sd = load_row_half<HT>(t, ft1, a.scale + so, a.half, g, vec4);
                    if (fold) {
                        f32x4 mean = load_row_half<HT>(t, ft1, a.mean + so, a.half, g, vec4);
                        f32x4 m2 = load_row_half<HT>(t, ft1, a.m2 + so, a.half, g, vec4);
                        lsnf_metric_fold(mean, m2, es, nf);
                        if (close) {
                            sd = lsnf_metric_close(sd, m2, nf, a.reg);
                            store_row_half<HT>(t, ft1, sd, a.scale + so, a.half, g, vec4);
                            mean = f32x4{0.f, 0.f, 0.f, 0.f}; m2 = f32x4{0.f, 0.f, 0.f, 0.f};
                        }
                        store_row_half<HT>(t, ft1, mean, a.mean + so, a.half, g, vec4);
                        store_row_half<HT>(t, ft1, m2, a.m2 + so, a.half, g, vec4);
                    }
                    gs = acc ? tp : ga[st][hs];
                    if (anneal) {                                      // every row, accepted or not: the kept gradient at beta_next
                        gs = lsnf_retemper(gs, d, gls);
                        store_row_half<HT>(t, ft1, gs, a.grad_acc + so, a.half, g, vec4);
                    }
                }
                if (resample) {                                        // the ancestor's quads of the same columns, lane to lane
                    const f32x4 eq = lsnf_exchange_take(es, al), gq = lsnf_exchange_take(gs, al), lq = lsnf_exchange_take(gls, al);
                    if (live[st] && moved) {                           // over what the update stored, to the row's own row
                        es = eq; gs = lsnf_retemper(gq, dn, lq);
                        store_row_half<HT>(t, ft1, es, a.eps_acc + so, a.half, g, vec4);
                        store_row_half<HT>(t, ft1, gs, a.grad_acc + so, a.half, g, vec4);
                        store_row_half<HT>(t, ft1, lq, a.like_grad_acc + so, a.half, g, vec4);
                    }
                }
                if (a.eps_new && live[st]) {                           // begin the next trajectory from the (updated, resampled) state
                    const f32x4 sg = lsnf_metric_mul(sd, gs);
                    f32x4 ph, en;
#pragma unroll
                    for (int r = 0; r < 4; ++r) ph[r] = xi[st][hs][r] - hn * sg[r];
                    const f32x4 sq = lsnf_metric_mul(sd, ph);
#pragma unroll
                    for (int r = 0; r < 4; ++r) en[r] = es[r] + sn * sq[r];
                    store_row_half<HT>(t, ft1, ph, a.mom + so, a.half, g, vec4);
                    store_row_half<HT>(t, ft1, en, a.eps_new + so, a.half, g, vec4);
                }
            }
        }
        if (wave == 0 && g == 0 && live[st]) {
            if (acc) a.like_u_acc[sample[st]] = en_g[st];
            if (anneal) {
                const float els = acc ? en_g[st] : el_old[st];
                a.u_acc[sample[st]] = lsnf_retemper(acc ? u_prop : u_old[st], d, els);
                if (!resample) lsnf_temper_weigh(lw[st], lc[st], d, els);
                reinterpret_cast<float2*>(a.log_w)[sample[st]] = float2{lw[st], lc[st]};
                a.beta_rows[sample[st]] = bn[st];
            } else if (acc) {
                a.u_acc[sample[st]] = u_prop;
            }
            if (a.eps_new) a.kin0[sample[st]] = 0.5f * s2;
            if (a.accept_out) a.accept_out[sample[st]] = acc ? 1.0f : 0.0f;
            if (a.log_alpha_out) a.log_alpha_out[sample[st]] = la;
            if (adapt) {
                reinterpret_cast<f32x4*>(a.adapt)[sample[st]] = ad[st];
                a.step_rows[sample[st]] = sn;
            }
            if (fold) a.count[sample[st]] = close ? 0.0f : nf;
            if (resample && moved) {                                   // (after the update's own stores of the same words)
                a.like_u_acc[sample[st]] = ep;
                a.u_acc[sample[st]] = uf;
            }
        }
    }
}
}  // namespace

#define LSNF_S3R_KERNEL lsnf_small3_rhmcs_kernel
#define LSNF_S3R_ARGS Small3RhmcResampleArgs
#define LSNF_S3R_TAIL small3_rhmcs_tail<HT, ST>(a, g1, g2, y2, sample, live, row, GTP, has1, nt1, ft1, wave, g, n, vec4); return;
#include "lsnf_small3_rbwd_kernel.h"

namespace {
// three partial row sums per wave and row in the g_t | g_p tiles, which are dead after the last block's barrier
static_assert(4 * 16 * 3 <= Small3RbwdLds<Small3RbwdCfg<1, 1>, 1>::TP, "the partial sums of the HMC tail live in GTP (HT = 1, ST = 1)");
template <class C, int ST>
hipError_t launch_small3_rhmcs_st(const Small3RhmcResampleArgs& a, hipStream_t stream) {
    if constexpr (!small3_rbwd_built<C, ST>) {
        return hipErrorInvalidValue;                 // (a selection bug)
    } else {
        const size_t lds = (size_t)Small3RbwdLds<C, ST>::L_END * sizeof(float);
        return lsnf_launch_kernel<lsnf_small3_rhmcs_kernel<C, ST, false>>(lsnf_grid(a.B, ST * S3_SAMPLES), 256, lds, stream, a);
    }
}
}  // namespace

// the resampling base-space HMC form (lsnf_reverse_hmc_step_resample): the same stages, the tempered leapfrog tail with the move as the
// output section; st: lsnf_small3_reverse_backward_st of the call
hipError_t lsnf_launch_small3_reverse_hmc_resample(const LsnfReverseHmcResampleCall& c, int st) {
    const bool inner = (c.chain.flags & 2u) != 0, adapt = (c.chain.flags & 4u) != 0, fold = (c.chain.flags & 16u) != 0;
    const bool anneal = (c.chain.flags & 64u) != 0, resample = (c.chain.flags & 512u) != 0;
    const bool group_ok = (c.group == 2 || c.group == 4 || c.group == 8 || c.group == 16) && c.B % c.group == 0;
    if (!c.act_saved || !c.chain.acc || !c.chain.grad_acc || !c.chain.u_acc || c.g_z_in || c.g_norm || c.eps_norm || c.B < 1 ||
        !c.mom || !c.kin0 || !c.step_rows || !c.scale || (adapt != (c.adapt != nullptr)) || (adapt && (c.chain.flags & 3u)) ||
        ((c.chain.flags & 8u) && !adapt) || (fold && (c.chain.flags & 3u)) || ((c.chain.flags & 32u) && !fold) ||
        (fold != (c.mean != nullptr)) || (fold != (c.m2 != nullptr)) || (fold != (c.count != nullptr)) ||
        !c.beta_rows || !c.like_grad_acc || !c.like_u_acc || (anneal && inner) || (anneal != (c.beta_next != nullptr)) ||
        (anneal != (c.log_w != nullptr)) || (c.chain.flags & (128u | 256u)) ||
        (resample && (!group_ok || !anneal || (c.chain.flags & (1u | 2u | 4u | 16u | 32u)))) ||
        (!resample && (c.resample_uniform || c.ancestor_out || c.ess_out)) ||
        (resample && (c.rng.enabled ? c.resample_uniform != nullptr : c.resample_uniform == nullptr)) ||
        (c.rng.enabled && (c.noise || c.chain.uniform)) || (!inner && c.eps_new && !c.noise && !c.rng.enabled) ||
        (inner && (!c.eps_new || c.noise || c.chain.uniform || c.rng.enabled || (c.chain.flags & 1u))))
        return hipErrorInvalidValue;                    // (a selection bug)
    Small3RhmcResampleArgs a;
    a.panels = c.plan + c.g.off_b3b_panels;
    a.tpanels = c.plan + c.g.off_t3b_panels;
    a.z_out = c.z_out; a.z_saved = c.z_saved; a.act_saved = c.act_saved; a.g_x = c.grad_g; a.g_obj = nullptr; a.g_z_in = nullptr;
    a.B = c.B; a.nz = c.g.nz; a.half = c.g.half; a.depth = c.g.depth; a.vec4 = c.vec4;
    a.noise = c.noise; a.eps_new = c.eps_new; a.g_norm = nullptr; a.eps_norm = nullptr; a.step = 0.0f; a.rng = c.rng;
    a.eps_acc = c.chain.acc;
    lsnf_fill_chain(a, c.chain);
    a.mom = c.mom; a.kin0 = c.kin0;
    a.step_rows = c.step_rows; a.adapt = c.adapt; a.da = c.da;
    a.scale = c.scale; a.mean = c.mean; a.m2 = c.m2; a.count = c.count; a.reg = c.reg;
    a.beta_rows = c.beta_rows; a.beta_next = c.beta_next; a.like_grad_acc = c.like_grad_acc; a.like_u_acc = c.like_u_acc; a.log_w = c.log_w;
    a.group = c.group; a.ess_frac = c.ess_frac; a.resample_uniform = c.resample_uniform; a.ancestor_out = c.ancestor_out; a.ess_out = c.ess_out;
    return lsnf_with_cfg<Small3RbwdCfg>(c.g, [&](auto cfg) {
        return lsnf_with_st(st, [&](auto s) { return launch_small3_rhmcs_st<decltype(cfg), decltype(s)::value>(a, c.stream); });
    });
}

// lsnf_small3_hmcs.hip -- Hamiltonian Monte Carlo in z with a likelihood temperature per row and a resampling move between the rows
// of a group on an annealing end call: a sequential Monte Carlo sampler (lsnf_hmc_step_resample, include/lsnf_flow_mcmc.h).  The
// kernel text of lsnf_small3_bwd_kernel.h with the tempered leapfrog tail of lsnf_small3_hmct.hip, as a translation unit of its own,
// so that the kernels of lsnf_small3_hmct.o and lsnf_small3_hmcx.o are compiled from the text they always were.  The tail is
// lsnf_small3_hmct.hip's, statement for statement, with these differences:
//   RESAMPLE     (flags & 512, end calls with ANNEAL and without ADAPT / FOLD / CLOSE, kernel-uniform) after the decision, the state
//                update and the ANNEAL lines, before the next trajectory begins.  Every lane of every wave forms its row's new
//                Kahan pair and re-tempered potential (pure functions of scalars every lane holds) and the group's decision
//                (lsnf_resample.h) from the rows' shuffled log weights.  The per-quad loop is entered by the whole wave (has1 alone,
//                wave-uniform; the row's loads and stores under live[st]), as in lsnf_small3_hmcx.hip, so that the move can sit
//                inside it, between the update of a quad and the begin of the next trajectory from it.  Row n's ancestor is a tile
//                row of the same group, i.e. a lane of the same wave and column group: beta_next, els, us and the three quads come
//                over by ds_bpermute (a group is live or not as a whole since B % group == 0).  A row whose ancestor is another row
//                stores the ancestor's zs / gls / els and its gs / us re-tempered to its OWN beta_next over what the update stored,
//                to its own row, and begins the next trajectory from them; temperatures, steps and metric stay with the row.
//   resample_uniform (B) read at the group's first row where the decision is formed, or drawn in-kernel at counter field 4 of that row.
// Without RESAMPLE a row's outputs are lsnf_small3_hmct_kernel's bit for bit in every phase.  Everything here is fp32 without fp
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
// xi of one half-unit (lsnf_small3_hmc.hip hmc_xi): a row of the noise tensor, or the in-kernel draw; padding columns are 0
template <int HT, class A>
__device__ __forceinline__ f32x4 hmcs_xi(const A& a, const LsnfRngState& rs, int hs, int t, int nt1, int ft1, int g, long row, long sample, int vec4) {
    if (a.noise) return load_row_half<HT>(t, ft1, a.noise + row * (long)a.nz, a.half, g, vec4);
    f32x4 xi = f32x4{0.f, 0.f, 0.f, 0.f};
    if (rs.on) {
        const unsigned long long grow = (unsigned long long)(a.rng.row0 + sample);
        const int f0 = 32 * nt1 + 16 * ft1 + 4 * g;
        unsigned c0 = ((unsigned)hs << 16) | (unsigned)(f0 >> 2), c1 = (unsigned)grow, c2 = rs.c2, c3 = rs.c3hi ^ (unsigned)(grow >> 32);
        lsnf_philox4x32_10(c0, c1, c2, c3, rs.k0, rs.k1);
        float n0, n1, n2, n3;
        lsnf_box_muller(c0, c1, n0, n1);
        lsnf_box_muller(c2, c3, n2, n3);
        xi = f32x4{n0, n1, n2, n3};
#pragma unroll
        for (int r = 0; r < 4; ++r) xi[r] = (f0 + r < a.half) ? xi[r] : 0.0f;
    }
    return xi;
}

// The output section of the resampling HMC form: a: Small3HmcResampleArgs; gx1 / gx2: this wave's half-units of grad(-ll)(z_prop),
// replaced by g_prop; the rest: the kernel's locals of the same names.
template <int HT, int ST, class A>
__device__ __forceinline__ void small3_hmcs_tail(const A& a, f32x4 (&gx1)[ST], f32x4 (&gx2)[ST], const long (&sample)[ST], const bool (&live)[ST],
                                                 const long (&row)[ST], float* RED, bool has1, int nt1, int ft1, int wave, int g, int n, int vec4) {
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
#pragma unroll
            for (int hs = 0; hs < 2; ++hs) {
                const int t = hs * HT + nt1;
                const long ro = row[st] * (long)a.nz, so = sample[st] * (long)a.nz;
                const f32x4 zp = load_row_half<HT>(t, ft1, a.z_cur + ro, a.half, g, vec4);
                const f32x4 pm = load_row_half<HT>(t, ft1, a.mom + ro, a.half, g, vec4);
                const f32x4 sd = load_row_half<HT>(t, ft1, a.scale + ro, a.half, g, vec4);
                f32x4 gg = f32x4{0.f, 0.f, 0.f, 0.f};
                if (a.grad_g) gg = load_row_half<HT>(t, ft1, a.grad_g + ro, a.half, g, vec4);
                const f32x4 bg = lsnf_temper_mul(bt[st], gg);
                const f32x4 gq = hs ? gx2[st] : gx1[st];
                f32x4 gp, ph, zn;
#pragma unroll
                for (int r = 0; r < 4; ++r) gp[r] = bg[r] + gq[r];     // g = (beta * grad_g) + grad(-ll)
                const f32x4 sg = lsnf_metric_mul(sd, gp);
#pragma unroll
                for (int r = 0; r < 4; ++r) ph[r] = pm[r] - s[st] * sg[r];
                const f32x4 sq = lsnf_metric_mul(sd, ph);
#pragma unroll
                for (int r = 0; r < 4; ++r) zn[r] = zp[r] + s[st] * sq[r];
                if (live[st]) {
                    store_row_half<HT>(t, ft1, ph, a.mom + so, a.half, g, vec4);
                    store_row_half<HT>(t, ft1, zn, a.z_new + so, a.half, g, vec4);
                }
            }
        }
        return;
    }
    // ---- INIT / end of a trajectory ----
    const LsnfRngState rs = a.rng.enabled ? lsnf_rng_state(a.rng) : LsnfRngState{0u, 0u, 0u, 0u, 0};
    f32x4 zp[ST][2], za[ST][2], ga[ST][2], xi[ST][2];                  // (g_prop replaces gx1 / gx2)
    float u_prop[ST], u_old[ST], k_old[ST], uni[ST], cnt[ST];          // per row; read before the barrier: wave 0 stores u_acc / kin0 / count after it
    float el[ST], el_old[ST], bn[ST], lw[ST], lc[ST];                  // likewise like_u_acc, beta_next and the Kahan pair
    f32x4 ad[ST];                                                      // likewise the rows' {log_step_bar, hbar, count, mu}
    // phase 1: this wave's half-units of the rows, its partial sums into RED
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        float sl = 0.0f, sx = 0.0f;
        el[st] = a.energy_g ? a.energy_g[row[st]] : 0.0f;
        u_prop[st] = lsnf_temper_mul(bt[st], el[st]) - a.ll_prop[row[st]];
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
#pragma unroll
        for (int hs = 0; hs < 2; ++hs) {
            const int t = hs * HT + nt1;
            const long ro = row[st] * (long)a.nz;
            zp[st][hs] = load_row_half<HT>(t, ft1, a.z_cur + ro, a.half, g, vec4);
            f32x4 gg = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.grad_g) gg = load_row_half<HT>(t, ft1, a.grad_g + ro, a.half, g, vec4);
            const f32x4 bg = lsnf_temper_mul(bt[st], gg);
            f32x4& gp = hs ? gx2[st] : gx1[st];
#pragma unroll
            for (int r = 0; r < 4; ++r) gp[r] = bg[r] + gp[r];         // g_prop = (beta * grad_g) + grad(-ll)
            za[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f}; ga[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!init) {
                za[st][hs] = load_row_half<HT>(t, ft1, a.z_acc + ro, a.half, g, vec4);
                ga[st][hs] = load_row_half<HT>(t, ft1, a.grad_acc + ro, a.half, g, vec4);
                const f32x4 pm = load_row_half<HT>(t, ft1, a.mom + ro, a.half, g, vec4);
                const f32x4 sg = lsnf_metric_mul(load_row_half<HT>(t, ft1, a.scale + ro, a.half, g, vec4), gp);
                f32x4 pl;
#pragma unroll
                for (int r = 0; r < 4; ++r) { pl[r] = pm[r] - hs2[st] * sg[r]; sl += pl[r] * pl[r]; }
                // nothing is proposed: the full-step momentum at the proposal is left readable (this lane loaded these columns)
                if (!a.z_new && has1 && live[st]) store_row_half<HT>(t, ft1, pl, a.mom + sample[st] * (long)a.nz, a.half, g, vec4);
            }
            xi[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.z_new) {
                xi[st][hs] = hmcs_xi<HT>(a, rs, hs, t, nt1, ft1, g, row[st], sample[st], vec4);
#pragma unroll
                for (int r = 0; r < 4; ++r) sx += xi[st][hs][r] * xi[st][hs][r];
            }
        }
        if (!has1) { sl = 0.0f; sx = 0.0f; }                           // (a wave without a unit repeats unit 0: counted once)
        sl = group_sum(sl); sx = group_sum(sx);
        if (g == 0) { RED[((st * 4 + wave) * 16 + n) * 2] = sl; RED[((st * 4 + wave) * 16 + n) * 2 + 1] = sx; }
    }
    __syncthreads();
    // phase 2: every wave decides its rows (the same sums in the same order: the same decision, the same new step), then stores its
    // half-units
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) { s1 += RED[((st * 4 + w) * 16 + n) * 2]; s2 += RED[((st * 4 + w) * 16 + n) * 2 + 1]; }
        float la = 0.0f;
        bool acc = true;
        if (!init) {
            const float kin_l = 0.5f * s1;
            la = (u_old[st] - u_prop[st]) + (k_old[st] - kin_l);
            float u = uni[st];
            if (!a.uniform) {
                const unsigned long long grow = (unsigned long long)(a.rng.row0 + sample[st]);
                unsigned c0 = 2u << 16, c1 = (unsigned)grow, c2 = rs.c2, c3 = rs.c3hi ^ (unsigned)(grow >> 32);
                lsnf_philox4x32_10(c0, c1, c2, c3, rs.k0, rs.k1);
                u = ((float)(c0 >> 8) + 0.5f) * 5.9604644775390625e-08f;
            }
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
            const float els = acc ? el[st] : el_old[st];
            const float us = lsnf_retemper(acc ? u_prop[st] : u_old[st], d, els);      // what the ANNEAL lines below store, formed by every lane
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
                f32x4 zs = f32x4{0.f, 0.f, 0.f, 0.f}, gs = zs, gls = zs, sd = zs;      // (a dead row's: zeros nobody uses)
                if (live[st]) {
                    const f32x4 gp = hs ? gx2[st] : gx1[st];
                    zs = acc ? zp[st][hs] : za[st][hs];                 // the state after the decision
                    if (acc) {                                         // its gl: grad_g (read again) on accepted rows, the kept one otherwise
                        if (a.grad_g) gls = load_row_half<HT>(t, ft1, a.grad_g + so, a.half, g, vec4);      // (live: so is the row's own offset)
                        store_row_half<HT>(t, ft1, zp[st][hs], a.z_acc + so, a.half, g, vec4);
                        store_row_half<HT>(t, ft1, gls, a.like_grad_acc + so, a.half, g, vec4);
                        if (!anneal) store_row_half<HT>(t, ft1, gp, a.grad_acc + so, a.half, g, vec4);
                    } else if (anneal) {
                        gls = load_row_half<HT>(t, ft1, a.like_grad_acc + so, a.half, g, vec4);
                    }
                    sd = load_row_half<HT>(t, ft1, a.scale + so, a.half, g, vec4);
                    if (fold) {
                        f32x4 mean = load_row_half<HT>(t, ft1, a.mean + so, a.half, g, vec4);
                        f32x4 m2 = load_row_half<HT>(t, ft1, a.m2 + so, a.half, g, vec4);
                        lsnf_metric_fold(mean, m2, zs, nf);
                        if (close) {
                            sd = lsnf_metric_close(sd, m2, nf, a.reg);
                            store_row_half<HT>(t, ft1, sd, a.scale + so, a.half, g, vec4);
                            mean = f32x4{0.f, 0.f, 0.f, 0.f}; m2 = f32x4{0.f, 0.f, 0.f, 0.f};
                        }
                        store_row_half<HT>(t, ft1, mean, a.mean + so, a.half, g, vec4);
                        store_row_half<HT>(t, ft1, m2, a.m2 + so, a.half, g, vec4);
                    }
                    gs = acc ? gp : ga[st][hs];
                    if (anneal) {                                      // every row, accepted or not: the kept gradient at beta_next
                        gs = lsnf_retemper(gs, d, gls);
                        store_row_half<HT>(t, ft1, gs, a.grad_acc + so, a.half, g, vec4);
                    }
                }
                if (resample) {                                        // the ancestor's quads of the same columns, lane to lane
                    const f32x4 zq = lsnf_exchange_take(zs, al), gq = lsnf_exchange_take(gs, al), lq = lsnf_exchange_take(gls, al);
                    if (live[st] && moved) {                           // over what the update stored, to the row's own row
                        zs = zq; gs = lsnf_retemper(gq, dn, lq);
                        store_row_half<HT>(t, ft1, zs, a.z_acc + so, a.half, g, vec4);
                        store_row_half<HT>(t, ft1, gs, a.grad_acc + so, a.half, g, vec4);
                        store_row_half<HT>(t, ft1, lq, a.like_grad_acc + so, a.half, g, vec4);
                    }
                }
                if (a.z_new && live[st]) {                             // begin the next trajectory from the (updated, resampled) state
                    const f32x4 sg = lsnf_metric_mul(sd, gs);
                    f32x4 ph, zn;
#pragma unroll
                    for (int r = 0; r < 4; ++r) ph[r] = xi[st][hs][r] - hn * sg[r];
                    const f32x4 sq = lsnf_metric_mul(sd, ph);
#pragma unroll
                    for (int r = 0; r < 4; ++r) zn[r] = zs[r] + sn * sq[r];
                    store_row_half<HT>(t, ft1, ph, a.mom + so, a.half, g, vec4);
                    store_row_half<HT>(t, ft1, zn, a.z_new + so, a.half, g, vec4);
                }
            }
        }
        if (wave == 0 && g == 0 && live[st]) {
            if (acc) a.like_u_acc[sample[st]] = el[st];
            if (anneal) {
                const float els = acc ? el[st] : el_old[st];
                a.u_acc[sample[st]] = lsnf_retemper(acc ? u_prop[st] : u_old[st], d, els);
                if (!resample) lsnf_temper_weigh(lw[st], lc[st], d, els);
                reinterpret_cast<float2*>(a.log_w)[sample[st]] = float2{lw[st], lc[st]};
                a.beta_rows[sample[st]] = bn[st];
            } else if (acc) {
                a.u_acc[sample[st]] = u_prop[st];
            }
            if (a.z_new) a.kin0[sample[st]] = 0.5f * s2;
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

#define LSNF_S3B_KERNEL lsnf_small3_hmcs_kernel
#define LSNF_S3B_ARGS Small3HmcResampleArgs
#define LSNF_S3B_TAIL small3_hmcs_tail<HT, ST>(a, gx1, gx2, sample, live, row, RED, has1, nt1, ft1, wave, g, n, vec4); return;
#include "lsnf_small3_bwd_kernel.h"

namespace {
template <class C, int ST>
hipError_t launch_small3_hmcs_st(const Small3HmcResampleArgs& a, hipStream_t stream) {
    if constexpr (!small3_bwd_built<C, ST>) {
        return hipErrorInvalidValue;                 // (a selection bug)
    } else {
        const size_t lds = (size_t)Small3BwdLds<C, ST>::L_END * sizeof(float);
        return lsnf_launch_kernel<lsnf_small3_hmcs_kernel<C, ST, false>>(lsnf_grid(a.B, ST * S3_SAMPLES), 256, lds, stream, a);
    }
}
}  // namespace

// the resampling HMC form (lsnf_hmc_step_resample): the same stages, the tempered leapfrog tail with the move as the output section; st:
// lsnf_small3_backward_st of the call
hipError_t lsnf_launch_small3_hmc_resample(const LsnfHmcResampleCall& c, int st) {
    const bool inner = (c.chain.flags & 2u) != 0, adapt = (c.chain.flags & 4u) != 0, fold = (c.chain.flags & 16u) != 0;
    const bool anneal = (c.chain.flags & 64u) != 0, resample = (c.chain.flags & 512u) != 0;
    const bool group_ok = (c.group == 2 || c.group == 4 || c.group == 8 || c.group == 16) && c.B % c.group == 0;
    if (!c.act_saved || !c.lv || c.dump || c.g_z_in || c.B < 1 || !c.mom || !c.kin0 || !c.step_rows || !c.scale ||
        (c.lv->rng.enabled && (c.lv->noise || c.chain.uniform)) || (adapt != (c.adapt != nullptr)) || (adapt && (c.chain.flags & 3u)) ||
        ((c.chain.flags & 8u) && !adapt) || (fold && (c.chain.flags & 3u)) || ((c.chain.flags & 32u) && !fold) ||
        (fold != (c.mean != nullptr)) || (fold != (c.m2 != nullptr)) || (fold != (c.count != nullptr)) ||
        !c.beta_rows || !c.like_grad_acc || !c.like_u_acc || (anneal && inner) || (anneal != (c.beta_next != nullptr)) ||
        (anneal != (c.log_w != nullptr)) || (c.chain.flags & (128u | 256u)) ||
        (resample && (!group_ok || !anneal || (c.chain.flags & (1u | 2u | 4u | 16u | 32u)))) ||
        (!resample && (c.resample_uniform || c.ancestor_out || c.ess_out)) ||
        (resample && (c.lv->rng.enabled ? c.resample_uniform != nullptr : c.resample_uniform == nullptr)) ||
        (inner && (!c.lv->z_new || c.lv->noise || c.chain.uniform || c.lv->rng.enabled || (c.chain.flags & 1u))))
        return hipErrorInvalidValue;                    // (a selection bug)
    Small3HmcResampleArgs a;
    lsnf_fill_mala(a, c);
    a.mom = c.mom; a.kin0 = c.kin0;
    a.step_rows = c.step_rows; a.adapt = c.adapt; a.da = c.da;
    a.scale = c.scale; a.mean = c.mean; a.m2 = c.m2; a.count = c.count; a.reg = c.reg;
    a.beta_rows = c.beta_rows; a.beta_next = c.beta_next; a.like_grad_acc = c.like_grad_acc; a.like_u_acc = c.like_u_acc; a.log_w = c.log_w;
    a.group = c.group; a.ess_frac = c.ess_frac; a.resample_uniform = c.resample_uniform; a.ancestor_out = c.ancestor_out; a.ess_out = c.ess_out;
    return lsnf_with_cfg<Small3BwdCfg>(c.g, [&](auto cfg) {
        return lsnf_with_st(st, [&](auto s) { return launch_small3_hmcs_st<decltype(cfg), decltype(s)::value>(a, c.stream); });
    });
}

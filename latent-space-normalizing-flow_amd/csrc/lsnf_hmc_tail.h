// lsnf_hmc_tail.h -- device: the leapfrog tail of Hamiltonian Monte Carlo in z (lsnf_hmc_step and its levels, include/lsnf_flow_mcmc.h):
// the output section that lsnf_small3_hmc.hip / _hmcm / _hmct / _hmcx / _hmcs / _hmca give the latency bf16x3 backward
// (lsnf_small3_bwd_kernel.h), one translation unit and one kernel name per level F (lsnf_hmc_level.h), so that no other kernel's text
// changes with a level.  (lsnf_small3_hmcr.hip, the per-row level in z, keeps a tail of its own: from this one its kernels were 1 - 2 %
// slower at 100 rows, profiles/hmc_one_tail_ab.txt.  The ROWS switches below serve the levels above it.)
//
// The stages run at a point z_prop of a trajectory (the point the forward's stash belongs to); the phase is a kernel-uniform branch:
//   INNER        a leapfrog step inside a trajectory: ph = mom - s sd g, z_next = z_prop + s sd ph, mom <- ph.  Per lane and column: no
//                cross-wave sum, no barrier; a lane stores the columns it loaded, so z_next may be z_prop.
//   INIT / end   two phases around one barrier, as the MALA tail.  (1) every wave loads its half-units of z_prop / grad_g / mom /
//                z_acc / grad_acc and the rows' scalars, draws or loads its half-units of xi (xi does not depend on the decision) and
//                leaves its partial row sums of sum pL^2 (pL = mom - (s/2) sd g_prop) and sum xi^2 in the two RED slots per row and
//                wave; (2) every wave adds the four partials of its rows in wave order -- the same numbers in the same order, so the
//                four waves decide alike --, forms log_alpha = (u_acc - U_prop) + (kin0 - kinL), draws (or has loaded) the row's
//                uniform, and stores its half-units of the state (accepted rows only) and of the next trajectory's first half-kick
//                ph = xi - (s/2) sd g_state, z_next = z_state + s sd ph, mom <- ph.  Wave 0 stores the row scalars.  All loads of a
//                workgroup's rows precede the barrier and a lane stores the columns it loaded.
// The uniform is lsnf_mala_step's (chain_uniform), xi lsnf_langevin_step's draw (chain_xi: a draw for a padding column, beyond nz / 2
// of its half, is 0 and not counted in sum xi^2).  Everything here is fp32 without fp contraction.
//
// Each level's products are one rounded product each, formed first (sd * g, sd * ph, beta * gl, beta * el), and 1.0f * x is x: with
// sd == 1 a METRIC row's outputs are the ROWS level's bit for bit, with beta == 1 and without ANNEAL a TEMPER row's the METRIC level's,
// without its move an EXCHANGE or RESAMPLE row's the TEMPER level's, without its search a SCHEDULE row's the RESAMPLE level's, and
// without ADAPT a ROWS row's the scalar level's at step_size = step_rows[row].
#pragma once
#include "lsnf_small3.h"
#include "lsnf_dual_avg.h"
#include "lsnf_metric.h"
#include "lsnf_temper.h"
#include "lsnf_exchange.h"
#include "lsnf_resample.h"
#include "lsnf_schedule.h"
#include "lsnf_hmc_level.h"

namespace {
// a: the level's Small3Hmc*Args; gx1 / gx2: this wave's half-units of grad(-ll)(z_prop), replaced by g_prop; the rest: the kernel's
// locals of the same names.
template <class F, int HT, int ST, class A>
__device__ __forceinline__ void small3_hmc_tail(const A& a, f32x4 (&gx1)[ST], f32x4 (&gx2)[ST], const long (&sample)[ST], const bool (&live)[ST],
                                                const long (&row)[ST], float* RED, bool has1, int nt1, int ft1, int wave, int g, int n, int vec4) {
#pragma clang fp contract(off)
    constexpr bool MOVE = F::EXCHANGE || F::RESAMPLE;
    // kernel-uniform.  ADAPT / FOLD / CLOSE: end calls only; ANNEAL: INIT and end calls; SWAP: end calls without ADAPT / FOLD / CLOSE /
    // ANNEAL; RESAMPLE: end calls with ANNEAL and without ADAPT / FOLD / CLOSE.  A flag above the level is a constant false.
    const bool init = (a.flags & 1u) != 0, inner = (a.flags & 2u) != 0, adapt = F::ROWS && (a.flags & 4u) != 0;
    const bool fold = F::METRIC && (a.flags & 16u) != 0, close = F::METRIC && (a.flags & 32u) != 0, anneal = F::TEMPER && (a.flags & 64u) != 0;
    const bool swap = F::EXCHANGE && (a.flags & 128u) != 0, resample = F::RESAMPLE && (a.flags & 512u) != 0;
    const bool schedule = F::SCHEDULE && (a.flags & 1024u) != 0;      // (SCHEDULE: INIT and end calls with ANNEAL, without ADAPT / FOLD / CLOSE)
    // A move's other row is a tile row of the same ladder / group, i.e. a lane of the same wave and column group: its scalars and
    // quads come over by ds_bpermute (lsnf_exchange.h).  A ladder or group is live or not as a whole since B % its length == 0; a
    // dead lane's registers are zeros that only dead lanes receive.
    int xlane = 0, pl = 0, rk = 0, P = 1;
    bool paired = false, lower = false;
    if constexpr (MOVE) xlane = lsnf_exchange_lane();
    if constexpr (F::EXCHANGE) {
        const int xn = xlane & 15;                                     // (n and g again, from the lane index itself)
        const int pn = swap ? lsnf_exchange_partner(xn, a.ladder, (a.flags & 256u) != 0) : xn;     // the partner's tile row (SWAP)
        paired = pn != xn; lower = pn > xn;
        pl = (xlane & 48) | pn;                                        // the partner's lane: the same wave, the same columns
    }
    if constexpr (F::RESAMPLE) {
        P = resample ? a.group : 1;                                    // the group's length (RESAMPLE)
        rk = xlane & (P - 1);                                          // the row's rung: 16 % P == 0, so it is (global row) % P
    }
    // per row: fixed before the momentum is drawn, constant in a trajectory.  Like u_acc / kin0 every wave loads them through the
    // clamped row[st] in front of the barrier (inner calls: in front of their loads); 0.5f * s is exact.
    float s[ST], hs2[ST], bt[ST];
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        if constexpr (F::ROWS) s[st] = a.step_rows[row[st]];
        else s[st] = a.step;
        hs2[st] = 0.5f * s[st];
        bt[st] = 0.0f;
        if constexpr (F::TEMPER) bt[st] = a.beta_rows[row[st]];
    }
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
                f32x4 sd = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (F::METRIC) sd = load_row_half<HT>(t, ft1, a.scale + ro, a.half, g, vec4);
                f32x4 gg = f32x4{0.f, 0.f, 0.f, 0.f};
                if (a.grad_g) gg = load_row_half<HT>(t, ft1, a.grad_g + ro, a.half, g, vec4);
                const f32x4 bg = lsnf_temper_mul_if<F::TEMPER>(bt[st], gg);
                const f32x4 gq = hs ? gx2[st] : gx1[st];
                f32x4 gp, ph, zn;
                // g = (beta * grad_g) + grad(-ll).  With a metric the products sd * g and sd * ph are formed first, over the quad; below
                // that level the step runs column by column, the statement shape the scalar kernel always had
                if constexpr (F::METRIC) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) gp[r] = bg[r] + gq[r];
                    const f32x4 sg = lsnf_metric_mul(sd, gp);
#pragma unroll
                    for (int r = 0; r < 4; ++r) ph[r] = pm[r] - s[st] * sg[r];
                    const f32x4 sq = lsnf_metric_mul(sd, ph);
#pragma unroll
                    for (int r = 0; r < 4; ++r) zn[r] = zp[r] + s[st] * sq[r];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        gp[r] = bg[r] + gq[r];
                        ph[r] = pm[r] - s[st] * gp[r];
                        zn[r] = zp[r] + s[st] * ph[r];
                    }
                }
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
    // per row; read by every wave before the barrier, through the clamped row[st]: wave 0 (lane g == 0) stores them after it
    float el[ST], u_prop[ST], u_old[ST], k_old[ST], uni[ST];
    f32x4 ad[ST];                                                      // ROWS: the rows' {log_step_bar, hbar, count, mu}
    float cnt[ST];                                                     // METRIC: the window's count
    float el_old[ST], bn[ST], lw[ST], lc[ST];                          // TEMPER: like_u_acc (el of the kept state), beta_next, the Kahan pair log_w
    float su[ST];                                                      // EXCHANGE: the swap's uniform
    // phase 1: this wave's half-units of the rows, its partial sums into RED
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        float sl = 0.0f, sx = 0.0f;
        el[st] = a.energy_g ? a.energy_g[row[st]] : 0.0f;
        u_prop[st] = lsnf_temper_mul_if<F::TEMPER>(bt[st], el[st]) - a.ll_prop[row[st]];
        u_old[st] = init ? 0.0f : a.u_acc[row[st]];
        k_old[st] = init ? 0.0f : a.kin0[row[st]];
        uni[st] = (a.uniform && !init) ? a.uniform[row[st]] : 0.5f;
        if constexpr (F::METRIC) cnt[st] = fold ? a.count[row[st]] : 0.0f;
        if constexpr (F::TEMPER) {                                     // (a rejected row re-tempers, or swaps, from its kept el)
            el_old[st] = ((anneal || swap) && !init) ? a.like_u_acc[row[st]] : 0.0f;
            // the pair's uniform is read at its lower row (B >= ladder: in bounds)
            if constexpr (F::EXCHANGE) su[st] = (paired && a.swap_uniform) ? a.swap_uniform[lower ? row[st] : row[st] - 1] : 0.5f;
            bn[st] = anneal ? a.beta_next[row[st]] : 0.0f;
            lw[st] = 0.0f; lc[st] = 0.0f;
            if (anneal) { const float2 p = reinterpret_cast<const float2*>(a.log_w)[row[st]]; lw[st] = p.x; lc[st] = p.y; }
        }
        if constexpr (F::ROWS) {
            ad[st] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (adapt) ad[st] = reinterpret_cast<const f32x4*>(a.adapt)[row[st]];
        }
#pragma unroll
        for (int hs = 0; hs < 2; ++hs) {
            const int t = hs * HT + nt1;
            const long ro = row[st] * (long)a.nz;
            zp[st][hs] = load_row_half<HT>(t, ft1, a.z_cur + ro, a.half, g, vec4);
            f32x4 gg = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.grad_g) gg = load_row_half<HT>(t, ft1, a.grad_g + ro, a.half, g, vec4);
            const f32x4 bg = lsnf_temper_mul_if<F::TEMPER>(bt[st], gg);
            f32x4& gp = hs ? gx2[st] : gx1[st];
#pragma unroll
            for (int r = 0; r < 4; ++r) gp[r] = bg[r] + gp[r];         // g_prop = (beta * grad_g) + grad(-ll)
            za[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f}; ga[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!init) {
                za[st][hs] = load_row_half<HT>(t, ft1, a.z_acc + ro, a.half, g, vec4);
                ga[st][hs] = load_row_half<HT>(t, ft1, a.grad_acc + ro, a.half, g, vec4);
                const f32x4 pm = load_row_half<HT>(t, ft1, a.mom + ro, a.half, g, vec4);
                // sd is read here for the last half-kick and AGAIN in phase 2 (or sd' is formed there): not 8 more quads live across
                // the barrier.  Padding columns load sd = 0 and store nothing.
                f32x4 sd = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (F::METRIC) sd = load_row_half<HT>(t, ft1, a.scale + ro, a.half, g, vec4);
                const f32x4 sg = lsnf_metric_mul_if<F::METRIC>(sd, gp);
                f32x4 pL;
#pragma unroll
                for (int r = 0; r < 4; ++r) { pL[r] = pm[r] - hs2[st] * sg[r]; sl += pL[r] * pL[r]; }
                // nothing is proposed: the full-step momentum at the proposal is left readable (this lane loaded these columns)
                if (!a.z_new && has1 && live[st]) store_row_half<HT>(t, ft1, pL, a.mom + sample[st] * (long)a.nz, a.half, g, vec4);
            }
            xi[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.z_new) {
                xi[st][hs] = chain_xi<HT>(a.noise, rs, a.rng.row0, a.nz, a.half, hs, nt1, ft1, g, row[st], sample[st], vec4);
#pragma unroll
                for (int r = 0; r < 4; ++r) sx += xi[st][hs][r] * xi[st][hs][r];
            }
        }
        if (!has1) { sl = 0.0f; sx = 0.0f; }                           // (a wave without a unit repeats unit 0: counted once)
        sl = group_sum(sl); sx = group_sum(sx);
        if (g == 0) { RED[((st * 4 + wave) * 16 + n) * 2] = sl; RED[((st * 4 + wave) * 16 + n) * 2 + 1] = sx; }
    }
    __syncthreads();
    // phase 2: every wave decides its rows (the same sums in the same order: the same decision, the same new step, the same move),
    // then stores its half-units
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
            if (!a.uniform) u = chain_uniform(rs, a.rng.row0, sample[st]);
            acc = logf(u) < la;                                        // (a NaN log_alpha rejects)
        }
        // ADAPT: the dual-averaging update from the row's log_alpha -- through the same instructions on the four waves, as the
        // decision itself, because the new step feeds every wave's half-units of the next trajectory's first half-kick
        float sn = s[st], hn = hs2[st];                                // the step of the trajectory this call begins
        if constexpr (F::ROWS) {
            if (adapt) {
                sn = lsnf_dual_average(ad[st], la, a.da, (a.flags & 8u) != 0);
                hn = 0.5f * sn;
                if (close && !(a.flags & 8u)) ad[st] = f32x4{0.f, 0.f, 0.f, logf(10.0f * sn)};      // the window's end restarts the averaging
            }
        }
        // SCHEDULE: the group's next temperature (lsnf_schedule.h) from its rows' log weights before the increment and el_s of their
        // states after the decision, in the place of beta_next, which is its ceiling: the same value on every row of the group and on
        // every wave.  The ANNEAL lines and the resampling move below read it as they read beta_next.  The whole wave is active here.
        if constexpr (F::SCHEDULE) {
            if (schedule) bn[st] = lsnf_schedule_next(bt[st], bn[st], lw[st] - lc[st], acc ? el[st] : el_old[st], a.group, a.cess_frac, a.min_step, xlane);
        }
        float nf = 0.0f, d = 0.0f;
        if constexpr (F::METRIC) nf = cnt[st] + 1.0f;                  // the row's count after the fold
        if constexpr (F::TEMPER) d = bn[st] - bt[st];                  // (ANNEAL) the change of the row's temperature
        // A move sits after the decision, the state update and the ANNEAL lines, before the next trajectory begins.  Every lane of
        // every wave forms its decision from the rows' scalars; the whole wave is active here.  ml: the lane of the row whose state
        // comes to this row, mv: it does; ep / up: that row's el_s / u_s, dn: what re-tempers its state to THIS row's temperature
        // (temperatures, steps and metric stay with the row), uf: its u_s there.
        float ep = 0.0f, up = 0.0f, dn = 0.0f, uf = 0.0f, lr = 0.0f;
        int ml = xlane;
        bool mv = false;
        if constexpr (F::EXCHANGE) {
            ml = pl;
            if (swap) {                                                // the pair's decision: the same log_r, the same decision on both rows
                const float els = acc ? el[st] : el_old[st], us = acc ? u_prop[st] : u_old[st];
                const float bp = lsnf_exchange_take(bt[st], pl);
                ep = lsnf_exchange_take(els, pl); up = lsnf_exchange_take(us, pl);
                if (paired) lr = lower ? lsnf_exchange_log_ratio(bt[st], bp, els, ep) : lsnf_exchange_log_ratio(bp, bt[st], ep, els);
                float u = su[st];
                if (!a.swap_uniform) u = lsnf_exchange_uniform(rs, a.rng.row0, lower ? sample[st] : sample[st] - 1);      // (counter field 3 of the lower row)
                mv = paired && logf(u) < lr;                           // (a NaN log_r rejects)
                dn = bt[st] - bp;
            }
        }
        if constexpr (F::RESAMPLE) {
            if (resample) {                                            // the group's decision (lsnf_resample.h) from the rows' shuffled log weights
                const float els = acc ? el[st] : el_old[st];
                const float us = lsnf_retemper(acc ? u_prop[st] : u_old[st], d, els);      // what the ANNEAL lines below store, formed by every lane
                float nw = lw[st], nc = lc[st];
                lsnf_temper_weigh(nw, nc, d, els);
                // the group's uniform, read here (at the group's first row; drawn: counter field 4 of that row) and not in front of the
                // barrier: held across it, it is a register that lsnf_small3_rhmcs_kernel<2, 4, 1> does not have (12 bytes of
                // scratch); (B >= group: row - rk is in bounds)
                const float u = a.resample_uniform ? a.resample_uniform[row[st] - rk] : lsnf_resample_uniform(rs, a.rng.row0, sample[st] - rk);
                const LsnfResample rv = lsnf_resample_decide(nw - nc, u, P, a.ess_frac, xlane);
                ml = xlane - rk + rv.ancestor;
                const float ba = lsnf_exchange_take(bn[st], ml);
                up = lsnf_exchange_take(us, ml);
                ep = lsnf_exchange_take(els, ml);
                dn = bn[st] - ba;                                      // (the ancestor's state comes to this row's beta_next)
                uf = lsnf_retemper(up, dn, ep);
                lw[st] = rv.on ? rv.lw : nw; lc[st] = rv.on ? 0.0f : nc;   // the pair the ANNEAL lines below store (they do not weigh again)
                if (wave == 0 && g == 0 && live[st]) {                 // (stored here: nothing of the decision but ml stays live)
                    if (a.ancestor_out) a.ancestor_out[sample[st]] = (float)rv.ancestor;
                    if (a.ess_out) a.ess_out[sample[st]] = rv.ess;
                }
            }
            mv = ml != xlane;
        }
        // With a move the per-quad loop is entered by the whole wave (has1 alone, wave-uniform; the row's loads and stores under
        // live[st]) so that the move can sit inside it, between the update of a quad and the begin of the next trajectory from it:
        // zs, gs, gls live for one quad only.  Without a move only live rows enter and the row's test below is a compile-time true:
        // entering with the whole wave at every level cost the tempered end call 4.5 % (profiles/hmc_one_tail_ab.txt, section 3).
        if (has1 && (MOVE || live[st])) {
            const bool lv = MOVE ? live[st] : true;
#pragma unroll
            for (int hs = 0; hs < 2; ++hs) {
                const int t = hs * HT + nt1;
                const long so = sample[st] * (long)a.nz;
                f32x4 zs = f32x4{0.f, 0.f, 0.f, 0.f}, gs = zs, gls = zs, sd = zs;      // (a dead row's: zeros nobody uses)
                if (lv) {                                              // (so is the row's own offset)
                    const f32x4 gp = hs ? gx2[st] : gx1[st];
                    zs = acc ? zp[st][hs] : za[st][hs];                 // the state after the decision
                    // TEMPER: gls, the state's gl, is grad_g on accepted rows -- read AGAIN, not 2 more quads live across the barrier --
                    // and the kept one (like_grad_acc) otherwise, which only a re-tempering or swapping call needs
                    if (acc) {
                        if constexpr (F::TEMPER)
                            if (a.grad_g) gls = load_row_half<HT>(t, ft1, a.grad_g + so, a.half, g, vec4);
                        store_row_half<HT>(t, ft1, zp[st][hs], a.z_acc + so, a.half, g, vec4);
                        if constexpr (F::TEMPER) store_row_half<HT>(t, ft1, gls, a.like_grad_acc + so, a.half, g, vec4);
                        if (!anneal) store_row_half<HT>(t, ft1, gp, a.grad_acc + so, a.half, g, vec4);
                    } else if constexpr (F::TEMPER) {
                        if (anneal || swap) gls = load_row_half<HT>(t, ft1, a.like_grad_acc + so, a.half, g, vec4);
                    }
                    if constexpr (F::METRIC) {
                        sd = load_row_half<HT>(t, ft1, a.scale + so, a.half, g, vec4);
                        if (fold) {                                    // the state after the decision into the window's Welford pair
                            f32x4 mean = load_row_half<HT>(t, ft1, a.mean + so, a.half, g, vec4);
                            f32x4 m2 = load_row_half<HT>(t, ft1, a.m2 + so, a.half, g, vec4);
                            lsnf_metric_fold(mean, m2, zs, nf);
                            if (close) {                               // sd' from the folded m2 (on padding columns it reaches no sum and no store);
                                sd = lsnf_metric_close(sd, m2, nf, a.reg);      // the next trajectory begins with it
                                store_row_half<HT>(t, ft1, sd, a.scale + so, a.half, g, vec4);
                                mean = f32x4{0.f, 0.f, 0.f, 0.f}; m2 = f32x4{0.f, 0.f, 0.f, 0.f};
                            }
                            store_row_half<HT>(t, ft1, mean, a.mean + so, a.half, g, vec4);
                            store_row_half<HT>(t, ft1, m2, a.m2 + so, a.half, g, vec4);
                        }
                    }
                    gs = acc ? gp : ga[st][hs];
                    if constexpr (F::TEMPER) {
                        if (anneal) {                                  // every row, accepted or not: the kept gradient at beta_next
                            gs = lsnf_retemper(gs, d, gls);
                            store_row_half<HT>(t, ft1, gs, a.grad_acc + so, a.half, g, vec4);
                        }
                    }
                }
                if constexpr (MOVE) {
                    if (swap || resample) {                            // the other row's quads of the same columns, lane to lane
                        const f32x4 zq = lsnf_exchange_take(zs, ml), gq = lsnf_exchange_take(gs, ml), lq = lsnf_exchange_take(gls, ml);
                        if (lv && mv) {                                // over what the update stored, to the row's own row
                            zs = zq; gs = lsnf_retemper(gq, dn, lq);
                            store_row_half<HT>(t, ft1, zs, a.z_acc + so, a.half, g, vec4);
                            store_row_half<HT>(t, ft1, gs, a.grad_acc + so, a.half, g, vec4);
                            store_row_half<HT>(t, ft1, lq, a.like_grad_acc + so, a.half, g, vec4);
                        }
                    }
                }
                if (a.z_new && lv) {                                   // begin the next trajectory from the (updated, moved) state
                    f32x4 ph, zn;
                    if constexpr (F::METRIC) {
                        const f32x4 sg = lsnf_metric_mul(sd, gs);
#pragma unroll
                        for (int r = 0; r < 4; ++r) ph[r] = xi[st][hs][r] - hn * sg[r];
                        const f32x4 sq = lsnf_metric_mul(sd, ph);
#pragma unroll
                        for (int r = 0; r < 4; ++r) zn[r] = zs[r] + sn * sq[r];
                    } else {                                           // (column by column: the INNER step's note)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            ph[r] = xi[st][hs][r] - hn * gs[r];
                            zn[r] = zs[r] + sn * ph[r];
                        }
                    }
                    store_row_half<HT>(t, ft1, ph, a.mom + so, a.half, g, vec4);
                    store_row_half<HT>(t, ft1, zn, a.z_new + so, a.half, g, vec4);
                }
            }
        }
        if (wave == 0 && g == 0 && live[st]) {
            if constexpr (F::TEMPER)
                if (acc) a.like_u_acc[sample[st]] = el[st];
            if (anneal) {                                              // u_acc of EVERY row re-tempered from the state after the decision;
                if constexpr (F::TEMPER) {                             // log_w takes -(d * el_s); beta <- beta_next
                    const float els = acc ? el[st] : el_old[st];
                    a.u_acc[sample[st]] = lsnf_retemper(acc ? u_prop[st] : u_old[st], d, els);
                    if (!resample) lsnf_temper_weigh(lw[st], lc[st], d, els);
                    reinterpret_cast<float2*>(a.log_w)[sample[st]] = float2{lw[st], lc[st]};
                    a.beta_rows[sample[st]] = bn[st];
                }
            } else if (acc) {
                a.u_acc[sample[st]] = u_prop[st];
            }
            if (a.z_new) a.kin0[sample[st]] = 0.5f * s2;
            if (a.accept_out) a.accept_out[sample[st]] = acc ? 1.0f : 0.0f;
            if (a.log_alpha_out) a.log_alpha_out[sample[st]] = la;
            if constexpr (F::ROWS) {
                if (adapt) {                                           // (with CLOSE and not ADAPT_LAST: the restarted quad)
                    reinterpret_cast<f32x4*>(a.adapt)[sample[st]] = ad[st];
                    a.step_rows[sample[st]] = sn;
                }
            }
            if constexpr (F::METRIC)
                if (fold) a.count[sample[st]] = close ? 0.0f : nf;
            if constexpr (MOVE) {
                if (mv) {                                              // (after the update's own stores of the same words)
                    if constexpr (F::EXCHANGE) uf = lsnf_retemper(up, dn, ep);
                    a.like_u_acc[sample[st]] = ep;
                    a.u_acc[sample[st]] = uf;
                }
            }
            if constexpr (F::EXCHANGE) {
                if (swap) {
                    if (a.swap_out) a.swap_out[sample[st]] = mv ? 1.0f : 0.0f;
                    if (a.log_swap_out) a.log_swap_out[sample[st]] = lr;
                }
            }
        }
    }
}
}  // namespace

// lsnf_small3_hmcr.hip -- Hamiltonian Monte Carlo in z with a step per row and dual-averaging adaptation of it (lsnf_hmc_step_rows,
// include/lsnf_flow_mcmc.h): the kernel text of lsnf_small3_bwd_kernel.h with a per-row leapfrog tail OF ITS OWN as the output section.
// The other eleven HMC units take their tail from lsnf_hmc_tail.h / lsnf_rhmc_tail.h; this level was measured 1 % (INNER) and 2 % (end
// call) slower at 100 rows from that tail's ROWS level in three jobs, with the split and with the column-by-column statement shape
// (profiles/hmc_one_tail_ab.txt), so it keeps the text its kernels were always compiled from.  What lsnf_hmc_tail.h says about the
// phases holds here; against the scalar level (that tail at LSNF_LEVEL_SCALAR) this one differs in:
//   s, hs2       row scalars (step_rows[row], 0.5f * that: exact) in place of the kernel-uniform a.step.  Like u_acc / kin0 every wave
//                loads them through the clamped row[st] in front of the barrier (inner calls: in front of their loads).
//   ADAPT        (flags & 4, end calls only, kernel-uniform) every wave loads the row's quad {log_step_bar, hbar, count, mu} in phase
//                1 and, in phase 2, runs the dual-averaging update from the row's log_alpha -- the same numbers through the same
//                instructions on the four waves, as the decision itself, because the new step s' feeds every wave's half-units of
//                the next trajectory's first half-kick.  Wave 0 alone stores the quad and s', for live rows, after the barrier.
// Without ADAPT a row's outputs are lsnf_small3_hmc_kernel's at step_size = step_rows[row], bit for bit: the same operations in the
// same order (tests/test_gpu_hmc_rows.py).  A fix to the shared tail has to be made here as well.  Everything here is fp32 without fp
// contraction.
#include <stdlib.h>
#include "lsnf_small3.h"
#include "lsnf_dual_avg.h"
#include "lsnf_launch.h"

namespace {
// xi of one half-unit (chain_xi of lsnf_small3.h, in the text this unit always had): a row of the noise tensor, or the in-kernel draw;
// padding columns are 0
template <int HT, class A>
__device__ __forceinline__ f32x4 hmcr_xi(const A& a, const LsnfRngState& rs, int hs, int t, int nt1, int ft1, int g, long row, long sample, int vec4) {
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

// The output section of the per-row HMC form: a: Small3HmcRowsArgs; gx1 / gx2: this wave's half-units of grad(-ll)(z_prop), replaced
// by g_prop; the rest: the kernel's locals of the same names.
template <int HT, int ST, class A>
__device__ __forceinline__ void small3_hmcr_tail(const A& a, f32x4 (&gx1)[ST], f32x4 (&gx2)[ST], const long (&sample)[ST], const bool (&live)[ST],
                                                 const long (&row)[ST], float* RED, bool has1, int nt1, int ft1, int wave, int g, int n, int vec4) {
#pragma clang fp contract(off)
    const bool init = (a.flags & 1u) != 0, inner = (a.flags & 2u) != 0, adapt = (a.flags & 4u) != 0;      // kernel-uniform
    float s[ST], hs2[ST];                                              // per row: fixed before the momentum is drawn, constant in a trajectory
#pragma unroll
    for (int st = 0; st < ST; ++st) { s[st] = a.step_rows[row[st]]; hs2[st] = 0.5f * s[st]; }
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
                f32x4 gg = f32x4{0.f, 0.f, 0.f, 0.f};
                if (a.grad_g) gg = load_row_half<HT>(t, ft1, a.grad_g + ro, a.half, g, vec4);
                const f32x4 gq = hs ? gx2[st] : gx1[st];
                f32x4 ph, zn;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float gp = gg[r] + gq[r];                    // g = grad_g + grad(-ll)
                    ph[r] = pm[r] - s[st] * gp;
                    zn[r] = zp[r] + s[st] * ph[r];
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
    float u_prop[ST], u_old[ST], k_old[ST], uni[ST];                   // per row; read before the barrier: wave 0 stores u_acc / kin0 after it
    f32x4 ad[ST];                                                      // likewise the rows' {log_step_bar, hbar, count, mu}
    // phase 1: this wave's half-units of the rows, its partial sums into RED
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        float sl = 0.0f, sx = 0.0f;
        u_prop[st] = (a.energy_g ? a.energy_g[row[st]] : 0.0f) - a.ll_prop[row[st]];
        u_old[st] = init ? 0.0f : a.u_acc[row[st]];
        k_old[st] = init ? 0.0f : a.kin0[row[st]];
        uni[st] = (a.uniform && !init) ? a.uniform[row[st]] : 0.5f;
        ad[st] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (adapt) ad[st] = reinterpret_cast<const f32x4*>(a.adapt)[row[st]];
#pragma unroll
        for (int hs = 0; hs < 2; ++hs) {
            const int t = hs * HT + nt1;
            const long ro = row[st] * (long)a.nz;
            zp[st][hs] = load_row_half<HT>(t, ft1, a.z_cur + ro, a.half, g, vec4);
            f32x4 gg = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.grad_g) gg = load_row_half<HT>(t, ft1, a.grad_g + ro, a.half, g, vec4);
            f32x4& gp = hs ? gx2[st] : gx1[st];
#pragma unroll
            for (int r = 0; r < 4; ++r) gp[r] = gg[r] + gp[r];         // g_prop = grad_g + grad(-ll)
            za[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f}; ga[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!init) {
                za[st][hs] = load_row_half<HT>(t, ft1, a.z_acc + ro, a.half, g, vec4);
                ga[st][hs] = load_row_half<HT>(t, ft1, a.grad_acc + ro, a.half, g, vec4);
                const f32x4 pm = load_row_half<HT>(t, ft1, a.mom + ro, a.half, g, vec4);
                f32x4 pl;
#pragma unroll
                for (int r = 0; r < 4; ++r) { pl[r] = pm[r] - hs2[st] * gp[r]; sl += pl[r] * pl[r]; }
                // nothing is proposed: the full-step momentum at the proposal is left readable (this lane loaded these columns)
                if (!a.z_new && has1 && live[st]) store_row_half<HT>(t, ft1, pl, a.mom + sample[st] * (long)a.nz, a.half, g, vec4);
            }
            xi[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.z_new) {
                xi[st][hs] = hmcr_xi<HT>(a, rs, hs, t, nt1, ft1, g, row[st], sample[st], vec4);
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
        }
        if (has1 && live[st]) {
#pragma unroll
            for (int hs = 0; hs < 2; ++hs) {
                const int t = hs * HT + nt1;
                const long so = sample[st] * (long)a.nz;
                const f32x4 gp = hs ? gx2[st] : gx1[st];
                if (acc) {
                    store_row_half<HT>(t, ft1, zp[st][hs], a.z_acc + so, a.half, g, vec4);
                    store_row_half<HT>(t, ft1, gp, a.grad_acc + so, a.half, g, vec4);
                }
                if (a.z_new) {                                         // begin the next trajectory from the (updated) state
                    const f32x4 zs = acc ? zp[st][hs] : za[st][hs], gs = acc ? gp : ga[st][hs];
                    f32x4 ph, zn;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        ph[r] = xi[st][hs][r] - hn * gs[r];
                        zn[r] = zs[r] + sn * ph[r];
                    }
                    store_row_half<HT>(t, ft1, ph, a.mom + so, a.half, g, vec4);
                    store_row_half<HT>(t, ft1, zn, a.z_new + so, a.half, g, vec4);
                }
            }
        }
        if (wave == 0 && g == 0 && live[st]) {
            if (acc) a.u_acc[sample[st]] = u_prop[st];
            if (a.z_new) a.kin0[sample[st]] = 0.5f * s2;
            if (a.accept_out) a.accept_out[sample[st]] = acc ? 1.0f : 0.0f;
            if (a.log_alpha_out) a.log_alpha_out[sample[st]] = la;
            if (adapt) {
                reinterpret_cast<f32x4*>(a.adapt)[sample[st]] = ad[st];
                a.step_rows[sample[st]] = sn;
            }
        }
    }
}
}  // namespace

#define LSNF_S3B_KERNEL lsnf_small3_hmcr_kernel
#define LSNF_S3B_ARGS Small3HmcRowsArgs
#define LSNF_S3B_TAIL small3_hmcr_tail<HT, ST>(a, gx1, gx2, sample, live, row, RED, has1, nt1, ft1, wave, g, n, vec4); return;
#include "lsnf_small3_bwd_kernel.h"

namespace {
template <class C, int ST>
hipError_t launch_small3_hmcr_st(const Small3HmcRowsArgs& a, hipStream_t stream) {
    if constexpr (!small3_bwd_built<C, ST>) {
        return hipErrorInvalidValue;                 // (a selection bug)
    } else {
        const size_t lds = (size_t)Small3BwdLds<C, ST>::L_END * sizeof(float);
        return lsnf_launch_kernel<lsnf_small3_hmcr_kernel<C, ST, false>>(lsnf_grid(a.B, ST * S3_SAMPLES), 256, lds, stream, a);
    }
}
}  // namespace

// the per-row HMC form (lsnf_hmc_step_rows): the same stages, the per-row leapfrog tail as the output section; st:
// lsnf_small3_backward_st of the call
hipError_t lsnf_launch_small3_hmc_rows(const LsnfHmcRowsCall& c, int st) {
    const bool inner = (c.chain.flags & 2u) != 0, adapt = (c.chain.flags & 4u) != 0;
    if (!c.act_saved || !c.lv || c.dump || c.g_z_in || c.B < 1 || !c.mom || !c.kin0 || !c.step_rows ||
        (c.lv->rng.enabled && (c.lv->noise || c.chain.uniform)) || (adapt != (c.adapt != nullptr)) || (adapt && (c.chain.flags & 3u)) ||
        ((c.chain.flags & 8u) && !adapt) ||
        (inner && (!c.lv->z_new || c.lv->noise || c.chain.uniform || c.lv->rng.enabled || (c.chain.flags & 1u))))
        return hipErrorInvalidValue;                    // (a selection bug)
    Small3HmcRowsArgs a;
    lsnf_fill_mala(a, c);
    a.mom = c.mom; a.kin0 = c.kin0;
    a.step_rows = c.step_rows; a.adapt = c.adapt; a.da = c.da;
    return lsnf_with_cfg<Small3BwdCfg>(c.g, [&](auto cfg) {
        return lsnf_with_st(st, [&](auto s) { return launch_small3_hmcr_st<decltype(cfg), decltype(s)::value>(a, c.stream); });
    });
}

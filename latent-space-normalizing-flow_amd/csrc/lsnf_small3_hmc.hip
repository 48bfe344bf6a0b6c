// lsnf_small3_hmc.hip -- Hamiltonian Monte Carlo in z (lsnf_hmc_step, include/lsnf_flow_mcmc.h): the latency bf16x3 backward of
// lsnf_small3_bwd.hip with a leapfrog tail as its output section, as a translation unit of its own (the lsnf_small3_mala.hip
// arrangement), so that the kernels of lsnf_small3_bwd.o and lsnf_small3_mala.o are compiled from the text they always were.
//
// The stages run at a point z_prop of a trajectory (the point the forward's stash belongs to); the phase is a kernel-uniform branch:
//   INNER        a leapfrog step inside a trajectory: ph = mom - s g, z_next = z_prop + s ph, mom <- ph.  Per lane and column: no
//                cross-wave sum, no barrier; a lane stores the columns it loaded, so z_next may be z_prop.
//   INIT / end   two phases around one barrier, as the MALA tail.  (1) every wave loads its half-units of z_prop / grad_g / mom /
//                z_acc / grad_acc and the rows' scalars, draws or loads its half-units of xi (xi does not depend on the decision) and
//                leaves its partial row sums of sum pL^2 (pL = mom - (s/2) g_prop) and sum xi^2 in the two RED slots per row and wave;
//                (2) every wave adds the four partials of its rows in wave order -- the same numbers in the same order, so the four
//                waves decide alike --, forms log_alpha = (u_acc - U_prop) + (kin0 - kinL), draws (or has loaded) the row's uniform,
//                and stores its half-units of the state (accepted rows only) and of the next trajectory's first half-kick
//                ph = xi - (s/2) g_state, z_next = z_state + s ph, mom <- ph.  Wave 0 stores the row scalars (u_acc, kin0, accept_out,
//                log_alpha_out).  All loads of a workgroup's rows precede the barrier and a lane stores the columns it loaded.
// The uniform is lsnf_mala_step's (word 0 of Philox at hh = 2 of the noise's counter), xi lsnf_langevin_step's draw; a draw for a
// padding column (beyond nz / 2 of its half) is not counted in sum xi^2.  Everything here is fp32 without fp contraction.
#include <stdlib.h>
#include "lsnf_small3.h"
#include "lsnf_launch.h"

namespace {
// xi of one half-unit: a row of the noise tensor, or the in-kernel draw at (seed, offset, global row, column); padding columns are 0
template <int HT, class A>
__device__ __forceinline__ f32x4 hmc_xi(const A& a, const LsnfRngState& rs, int hs, int t, int nt1, int ft1, int g, long row, long sample, int vec4) {
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

// The output section of the HMC form: a: Small3HmcArgs; gx1 / gx2: this wave's half-units of grad(-ll)(z_prop), replaced by g_prop;
// the rest: the kernel's locals of the same names.
template <int HT, int ST, class A>
__device__ __forceinline__ void small3_hmc_tail(const A& a, f32x4 (&gx1)[ST], f32x4 (&gx2)[ST], const long (&sample)[ST], const bool (&live)[ST],
                                                const long (&row)[ST], float* RED, bool has1, int nt1, int ft1, int wave, int g, int n, int vec4) {
#pragma clang fp contract(off)
    const bool init = (a.flags & 1u) != 0, inner = (a.flags & 2u) != 0;      // kernel-uniform
    const float s = a.step, hs2 = 0.5f * a.step;
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
                    ph[r] = pm[r] - s * gp;
                    zn[r] = zp[r] + s * ph[r];
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
    // phase 1: this wave's half-units of the rows, its partial sums into RED
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        float sl = 0.0f, sx = 0.0f;
        u_prop[st] = (a.energy_g ? a.energy_g[row[st]] : 0.0f) - a.ll_prop[row[st]];
        u_old[st] = init ? 0.0f : a.u_acc[row[st]];
        k_old[st] = init ? 0.0f : a.kin0[row[st]];
        uni[st] = (a.uniform && !init) ? a.uniform[row[st]] : 0.5f;
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
                for (int r = 0; r < 4; ++r) { pl[r] = pm[r] - hs2 * gp[r]; sl += pl[r] * pl[r]; }
                // nothing is proposed: the full-step momentum at the proposal is left readable (this lane loaded these columns)
                if (!a.z_new && has1 && live[st]) store_row_half<HT>(t, ft1, pl, a.mom + sample[st] * (long)a.nz, a.half, g, vec4);
            }
            xi[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.z_new) {
                xi[st][hs] = hmc_xi<HT>(a, rs, hs, t, nt1, ft1, g, row[st], sample[st], vec4);
#pragma unroll
                for (int r = 0; r < 4; ++r) sx += xi[st][hs][r] * xi[st][hs][r];
            }
        }
        if (!has1) { sl = 0.0f; sx = 0.0f; }                           // (a wave without a unit repeats unit 0: counted once)
        sl = group_sum(sl); sx = group_sum(sx);
        if (g == 0) { RED[((st * 4 + wave) * 16 + n) * 2] = sl; RED[((st * 4 + wave) * 16 + n) * 2 + 1] = sx; }
    }
    __syncthreads();
    // phase 2: every wave decides its rows (the same sums in the same order: the same decision), then stores its half-units
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
                        ph[r] = xi[st][hs][r] - hs2 * gs[r];
                        zn[r] = zs[r] + s * ph[r];
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
        }
    }
}
}  // namespace

#define LSNF_S3B_KERNEL lsnf_small3_hmc_kernel
#define LSNF_S3B_ARGS Small3HmcArgs
#define LSNF_S3B_TAIL small3_hmc_tail<HT, ST>(a, gx1, gx2, sample, live, row, RED, has1, nt1, ft1, wave, g, n, vec4); return;
#include "lsnf_small3_bwd_kernel.h"

namespace {
template <class C, int ST>
hipError_t launch_small3_hmc_st(const Small3HmcArgs& a, hipStream_t stream) {
    if constexpr (!small3_bwd_built<C, ST>) {
        return hipErrorInvalidValue;                 // (a selection bug)
    } else {
        const size_t lds = (size_t)Small3BwdLds<C, ST>::L_END * sizeof(float);
        return lsnf_launch_kernel<lsnf_small3_hmc_kernel<C, ST, false>>(lsnf_grid(a.B, ST * S3_SAMPLES), 256, lds, stream, a);
    }
}
}  // namespace

// the HMC form (lsnf_hmc_step): the same stages, the leapfrog tail as the output section; st: lsnf_small3_backward_st of the call
hipError_t lsnf_launch_small3_hmc(const LsnfHmcCall& c, int st) {
    const bool inner = (c.chain.flags & 2u) != 0;
    if (!c.act_saved || !c.lv || c.dump || c.g_z_in || c.B < 1 || !c.mom || !c.kin0 || (c.lv->rng.enabled && (c.lv->noise || c.chain.uniform)) ||
        (inner && (!c.lv->z_new || c.lv->noise || c.chain.uniform || c.lv->rng.enabled || (c.chain.flags & 1u))))
        return hipErrorInvalidValue;                    // (a selection bug)
    Small3HmcArgs a;
    lsnf_fill_mala(a, c);
    a.mom = c.mom; a.kin0 = c.kin0;
    return lsnf_with_cfg<Small3BwdCfg>(c.g, [&](auto cfg) {
        return lsnf_with_st(st, [&](auto s) { return launch_small3_hmc_st<decltype(cfg), decltype(s)::value>(a, c.stream); });
    });
}

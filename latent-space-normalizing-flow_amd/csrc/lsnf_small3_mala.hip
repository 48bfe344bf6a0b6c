// lsnf_small3_mala.hip -- the Metropolis-adjusted Langevin step (lsnf_mala_step, include/lsnf_flow_mcmc.h): the latency bf16x3 backward of
// lsnf_small3_bwd.hip with the accept / reject tail as its output section, as a translation unit of its own (the lsnf_bwd3w.hip
// arrangement), so that the kernels of lsnf_small3_bwd.o are compiled from the text they always were.
//
// The same stages run at a PROPOSAL z_prop (the point the forward's stash belongs to); the output section then decides the proposal
// against a kept chain state (z_acc, grad_acc = grad U(z_acc), u_acc = U(z_acc); U = energy_g - ll), updates the state in place and
// proposes again from it.  Two phases around one barrier: (1) every wave loads its half-units of z_prop / grad_g / z_acc / grad_acc
// and the rows' scalars, and leaves its partial row sums of A = |coef g_prop - d|^2 and Bq = |d + coef g_acc|^2 (d = z_prop - z_acc,
// coef = s^2 / 2) in RED; (2) every wave adds the four partials of its rows in wave order -- the same numbers in the same order, so
// the four waves decide alike --, forms log_alpha = u_acc - U_prop - (A - Bq) / (2 s^2), draws (or has loaded) the row's uniform, and
// stores its half-units of the state (accepted rows only) and of z_next = z_state - coef g_state + s xi.  All loads of a workgroup's
// rows precede the barrier and a lane stores the columns it loaded: z_next may be z_prop.  The uniform is word 0 of Philox at hh = 2
// of the noise's counter (lsnf_device.h), so it is a stream of its own and a pure function of (seed, offset, global row).
#include <stdlib.h>
#include "lsnf_small3.h"
#include "lsnf_launch.h"

namespace {
// MALA form: the next proposal of one half-unit, z_next = zs - coef gs + step xi with the operations and the operation order of the
// plain update of lsnf_small3_bwd_kernel.h (the default fp contraction, as there)
template <int HT, class A>
__device__ __forceinline__ void mala_propose(const A& a, const LsnfRngState& rs, const f32x4 zs, const f32x4 gs, float coef,
                                             int hs, int t, int nt1, int ft1, int g, long row, long sample, int vec4) {
    f32x4 zn;
#pragma unroll
    for (int r = 0; r < 4; ++r) zn[r] = zs[r] - coef * gs[r];
    if (a.noise) {
        const f32x4 nv = load_row_half<HT>(t, ft1, a.noise + row * (long)a.nz, a.half, g, vec4);
#pragma unroll
        for (int r = 0; r < 4; ++r) zn[r] = zn[r] + a.step * nv[r];
    } else if (rs.on) {
        const unsigned long long grow = (unsigned long long)(a.rng.row0 + sample);
        const int f0 = 32 * nt1 + 16 * ft1 + 4 * g;
        unsigned c0 = ((unsigned)hs << 16) | (unsigned)(f0 >> 2), c1 = (unsigned)grow, c2 = rs.c2, c3 = rs.c3hi ^ (unsigned)(grow >> 32);
        lsnf_philox4x32_10(c0, c1, c2, c3, rs.k0, rs.k1);
        float n0, n1, n2, n3;
        lsnf_box_muller(c0, c1, n0, n1);
        lsnf_box_muller(c2, c3, n2, n3);
        zn[0] += a.step * n0; zn[1] += a.step * n1; zn[2] += a.step * n2; zn[3] += a.step * n3;
    }
    store_row_half<HT>(t, ft1, zn, a.z_new + sample * (long)a.nz, a.half, g, vec4);
}

// The output section of the MALA form: a: Small3MalaArgs; gx1 / gx2: this wave's half-units of grad(-ll)(z_prop), replaced by g_prop;
// the rest: the kernel's locals of the same names.
template <int HT, int ST, class A>
__device__ __forceinline__ void small3_mala_tail(const A& a, f32x4 (&gx1)[ST], f32x4 (&gx2)[ST], const long (&sample)[ST], const bool (&live)[ST],
                                                 const long (&row)[ST], float* RED, bool has1, int nt1, int ft1, int wave, int g, int n, int vec4) {
#pragma clang fp contract(off)
    const bool init = (a.flags & 1u) != 0;                             // kernel-uniform
    const LsnfRngState rs = a.rng.enabled ? lsnf_rng_state(a.rng) : LsnfRngState{0u, 0u, 0u, 0u, 0};
    const float coef = 0.5f * a.step * a.step;
    f32x4 zp[ST][2], za[ST][2], ga[ST][2];                            // (g_prop replaces gx1 / gx2)
    float u_prop[ST], u_old[ST], uni[ST];                             // per row; read before the barrier: wave 0 stores u_acc after it
    // phase 1: this wave's half-units of the rows, its partial sums into RED
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        float sa = 0.0f, sb = 0.0f;
        u_prop[st] = (a.energy_g ? a.energy_g[row[st]] : 0.0f) - a.ll_prop[row[st]];
        u_old[st] = init ? 0.0f : a.u_acc[row[st]];
        uni[st] = (a.uniform && !init) ? a.uniform[row[st]] : 0.5f;
#pragma unroll
        for (int hs = 0; hs < 2; ++hs) {
            const int t = hs * HT + nt1;
            const long ro = row[st] * (long)a.nz;
            zp[st][hs] = load_row_half<HT>(t, ft1, a.z_cur + ro, a.half, g, vec4);
            f32x4 gg = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.grad_g) gg = load_row_half<HT>(t, ft1, a.grad_g + ro, a.half, g, vec4);
            za[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f}; ga[st][hs] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!init) {
                za[st][hs] = load_row_half<HT>(t, ft1, a.z_acc + ro, a.half, g, vec4);
                ga[st][hs] = load_row_half<HT>(t, ft1, a.grad_acc + ro, a.half, g, vec4);
            }
            f32x4& gp = hs ? gx2[st] : gx1[st];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                gp[r] = gg[r] + gp[r];                                  // g_prop = grad_g + grad(-ll)
                const float d = zp[st][hs][r] - za[st][hs][r];
                const float fa = coef * gp[r] - d, fb = d + coef * ga[st][hs][r];
                sa += fa * fa; sb += fb * fb;
            }
        }
        if (!has1) { sa = 0.0f; sb = 0.0f; }                           // (a wave without a unit repeats unit 0: counted once)
        sa = group_sum(sa); sb = group_sum(sb);
        if (g == 0) { RED[((st * 4 + wave) * 16 + n) * 2] = sa; RED[((st * 4 + wave) * 16 + n) * 2 + 1] = sb; }
    }
    __syncthreads();
    // phase 2: every wave decides its rows (the same sums in the same order: the same decision), then stores its half-units
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        float la = 0.0f;
        bool acc = true;
        if (!init) {
            float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { s1 += RED[((st * 4 + w) * 16 + n) * 2]; s2 += RED[((st * 4 + w) * 16 + n) * 2 + 1]; }
            la = (u_old[st] - u_prop[st]) - (s1 - s2) / (2.0f * a.step * a.step);
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
                if (a.z_new) mala_propose<HT>(a, rs, acc ? zp[st][hs] : za[st][hs], acc ? gp : ga[st][hs], coef, hs, t, nt1, ft1, g,
                                              row[st], sample[st], vec4);
            }
        }
        if (wave == 0 && g == 0 && live[st]) {
            if (acc) a.u_acc[sample[st]] = u_prop[st];
            if (a.accept_out) a.accept_out[sample[st]] = acc ? 1.0f : 0.0f;
            if (a.log_alpha_out) a.log_alpha_out[sample[st]] = la;
        }
    }
}
}  // namespace

#define LSNF_S3B_KERNEL lsnf_small3_mala_kernel
#define LSNF_S3B_ARGS Small3MalaArgs
#define LSNF_S3B_TAIL small3_mala_tail<HT, ST>(a, gx1, gx2, sample, live, row, RED, has1, nt1, ft1, wave, g, n, vec4); return;
#include "lsnf_small3_bwd_kernel.h"

namespace {
template <class C, int ST>
hipError_t launch_small3_mala_st(const Small3MalaArgs& a, hipStream_t stream) {
    if constexpr (!small3_bwd_built<C, ST>) {
        return hipErrorInvalidValue;                 // (a selection bug)
    } else {
        const size_t lds = (size_t)Small3BwdLds<C, ST>::L_END * sizeof(float);
        return lsnf_launch_kernel<lsnf_small3_mala_kernel<C, ST, false>>(lsnf_grid(a.B, ST * S3_SAMPLES), 256, lds, stream, a);
    }
}
}  // namespace

// the MALA form (lsnf_mala_step): the same stages, the accept / reject tail as the output section; st: lsnf_small3_backward_st of the call
hipError_t lsnf_launch_small3_mala(const LsnfMalaCall& c, int st) {
    if (!c.act_saved || !c.lv || c.dump || c.g_z_in || c.B < 1 || (c.lv->rng.enabled && (c.lv->noise || c.chain.uniform)))
        return hipErrorInvalidValue;                    // (a selection bug)
    Small3MalaArgs a;
    lsnf_fill_mala(a, c);
    return lsnf_with_cfg<Small3BwdCfg>(c.g, [&](auto cfg) {
        return lsnf_with_st(st, [&](auto s) { return launch_small3_mala_st<decltype(cfg), decltype(s)::value>(a, c.stream); });
    });
}

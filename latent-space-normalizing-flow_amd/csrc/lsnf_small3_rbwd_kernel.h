// lsnf_small3_rbwd_kernel.h -- the kernel text of the latency reverse-backward (lsnf_small3_rbwd.hip: the stages, the LDS map, the
// plain and the UPDATE output section), included by the three translation units that instantiate it.  The includer defines, before
// the #include:
//   LSNF_S3R_KERNEL  the kernel template's name          lsnf_small3_rbwd_kernel           | lsnf_small3_rmala_kernel               | lsnf_small3_rhmc_kernel
//   LSNF_S3R_ARGS    its argument struct (may name       Small3RbwdArgs, or Small3RlvArgs  | Small3RmalaArgs                        | Small3RhmcArgs
//                    the template parameter UPDATE)      with UPDATE
//   LSNF_S3R_TAIL    statements in front of the output   (nothing)                         | the accept / reject tail and `return;` | the leapfrog tail and `return;`
//                    section, with the kernel's locals in scope
// lsnf_small3_rbwd.hip gives the first column and is compiled from the same tokens as before this file existed; lsnf_small3_rmala.hip
// the second and lsnf_small3_rhmc.hip the third, both with UPDATE = false (their tails load e1, the first half of eps, themselves: in
// front of their own barrier); lsnf_small3_rhmcr.hip is the third column with a step per row (lsnf_small3_rhmcr_kernel, Small3RhmcRowsArgs),
// lsnf_small3_rhmcm.hip that one with a diagonal metric per row (lsnf_small3_rhmcm_kernel, Small3RhmcMetricArgs), lsnf_small3_rhmct.hip
// that one with a likelihood temperature per row (lsnf_small3_rhmct_kernel, Small3RhmcTemperedArgs), lsnf_small3_rhmcx.hip that one
// with a replica-exchange move between rows (lsnf_small3_rhmcx_kernel, Small3RhmcExchangeArgs), lsnf_small3_rhmcs.hip the tempered one
// with a resampling move between rows (lsnf_small3_rhmcs_kernel, Small3RhmcResampleArgs), lsnf_small3_rhmca.hip that one with the
// schedule search (lsnf_small3_rhmca_kernel, Small3RhmcScheduleArgs).
#pragma once

namespace {

template <int HT_, int WT_>
struct Small3RbwdCfg : LsnfStackCfg<HT_, WT_> {
    using S = LsnfStackCfg<HT_, WT_>;
    static constexpr int F = LSNF_FRAG3_FLOATS;
    static constexpr int OFFB4 = 0;                                       // inside a block of off_b3b_panels (B4, B3, B2, B1)
    static constexpr int OFFB3 = OFFB4 + F * WT_ * 2 * HT_;
    static constexpr int OFFB2 = OFFB3 + F * WT_ * WT_;
    static constexpr int BLOCKB = OFFB2 + F * HT_ * WT_ + F * S::NZT * S::NZT;
    static constexpr int BLOCKT = F * S::NZT * S::NZT;                    // a block of off_t3b_panels
    static constexpr int NU2 = (2 * WT_ + 3) / 4;
};
// LDS map (floats) for ST sample tiles: GTP (g_t | g_p: 2HT B-tiles per sample tile; g_a1 reuses its front once B4 has read it),
// GA2 (WT), G first half (HT), G second half (HT, double-buffered: the coupling of T1's epilogue writes the next block's input
// while other waves still read this block's)
template <class C, int ST>
struct Small3RbwdLds {
    static constexpr int TP = 2 * C::HT * S3_BTILE_FLOATS, HL = C::WT * S3_BTILE_FLOATS, GH = C::HT * S3_BTILE_FLOATS;
    static_assert(C::WT <= 2 * C::HT, "g_a1 is kept in the front of the g_t | g_p tiles");
    // (lsnf_rhmc_tail.h: three partial row sums per wave and row, in these tiles once they are dead after the last block's barrier)
    static_assert(4 * 16 * 3 <= TP, "the partial sums of the HMC tail live in GTP");
    static constexpr int L_GTP = 0;
    static constexpr int L_GA2 = L_GTP + ST * TP;
    static constexpr int L_GVA = L_GA2 + ST * HL;
    static constexpr int L_GVB = L_GVA + ST * GH;
    static constexpr int L_END = L_GVB + 2 * ST * GH;
};

struct Small3RbwdArgs {
    const float* panels;                 // b3b region, block 0
    const float* tpanels;                // t3b region, block 0
    const float* z_out; const float* z_saved; const float* act_saved; const float* g_x; const float* g_obj;
    float* g_z_in;
    int B, nz, half, depth, vec4;
};
// UPDATE form (lsnf_reverse_langevin_step): the base-space Langevin update on the kernel's own result.  g_z_in is then optional.
struct Small3RlvArgs : Small3RbwdArgs {
    const float* noise; float* eps_new; float* g_norm; float* eps_norm;
    float step;
    LsnfRngArgs rng;
};
// MALA form (lsnf_reverse_mala_step): z_out is the proposal eps_prop, eps_new the next proposal eps_next (may be NULL), g_x the caller's
// grad_g; g_z_in / g_norm / eps_norm stay NULL
struct Small3RmalaArgs : Small3RlvArgs {
    const float* energy_g; const float* uniform;
    float* eps_acc; float* grad_acc; float* u_acc; float* accept_out; float* log_alpha_out;
    unsigned flags;                                // LSNF_MALA_INIT (1): accept every row, the state is not read
};
// HMC form (lsnf_reverse_hmc_step): the MALA form's tensors at a point eps_prop of a trajectory; flags: LSNF_HMC_INIT (1), LSNF_HMC_INNER (2)
struct Small3RhmcArgs : Small3RmalaArgs {
    float* mom; float* kin0;                       // the momentum (read and written), the kinetic energy the trajectory began with
};
// per-row HMC form (lsnf_reverse_hmc_step_rows, lsnf_small3_rhmcr.hip): the HMC form's tensors, the step of each row (B; `step` is
// not read) and, with LSNF_HMC_ADAPT (4; LSNF_HMC_ADAPT_LAST: 8), the rows' dual-averaging state (B, 4; 16-byte aligned) and its constants
struct Small3RhmcRowsArgs : Small3RhmcArgs {
    float* step_rows; float* adapt;
    LsnfDualAvgArgs da;
};
// metric HMC form (lsnf_reverse_hmc_step_metric, lsnf_small3_rhmcm.hip): the per-row form's tensors, the rows' scales (B, nz) and, with
// LSNF_HMC_METRIC_FOLD (16; LSNF_HMC_METRIC_CLOSE: 32), the Welford accumulators of the running window and the close's constants
struct Small3RhmcMetricArgs : Small3RhmcRowsArgs {
    float* scale; float* mean; float* m2; float* count;
    LsnfMetricArgs reg;
};
// tempered HMC form (lsnf_reverse_hmc_step_tempered, lsnf_small3_rhmct.hip): the metric form's tensors, the rows' likelihood temperature
// (B), the likelihood's part of the kept state (like_grad_acc: B, nz; like_u_acc: B) and, with LSNF_HMC_ANNEAL (64), the next
// temperature (B) and the Kahan pair of the importance weight (B, 2; 8-byte aligned)
struct Small3RhmcTemperedArgs : Small3RhmcMetricArgs {
    float* beta_rows; const float* beta_next; float* like_grad_acc; float* like_u_acc; float* log_w;
};
// exchanging HMC form (lsnf_reverse_hmc_step_exchange, lsnf_small3_rhmcx.hip): the tempered form's tensors and, with LSNF_HMC_SWAP
// (128), the ladder's length, the pairs' uniforms (B, read at the lower row; NULL: drawn in-kernel) and the move's two optional outputs
struct Small3RhmcExchangeArgs : Small3RhmcTemperedArgs {
    int ladder; const float* swap_uniform; float* swap_out; float* log_swap_out;
};
// resampling HMC form (lsnf_reverse_hmc_step_resample, lsnf_small3_rhmcs.hip): the tempered form's tensors and, with LSNF_HMC_RESAMPLE
// (512), the group's length, the threshold as a fraction of it, the groups' uniforms (B, read at the group's first row; NULL: drawn
// in-kernel) and the move's two optional outputs
struct Small3RhmcResampleArgs : Small3RhmcTemperedArgs {
    int group; float ess_frac; const float* resample_uniform; float* ancestor_out; float* ess_out;
};
// scheduling HMC form (lsnf_reverse_hmc_step_schedule, lsnf_small3_rhmca.hip): the resampling form's tensors and, with
// LSNF_HMC_SCHEDULE (1024), the target of the conditional effective sample size as a fraction and the least step of a searching group
struct Small3RhmcScheduleArgs : Small3RhmcResampleArgs {
    float cess_frac, min_step;
};

__device__ __forceinline__ f32x4 rb_mask4(f32x4 a, unsigned nib) {
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = ((nib >> r) & 1u) ? a[r] : 0.0f;
    return a;
}
__device__ __forceinline__ f32x4 rb_zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// UPDATE = false: g on the reverse's input.  UPDATE = true: the output section is the Langevin update of the reverse's input eps
// (= z_out) with that g -- per element, in this order, each step one fp32 rounding (explicit intrinsics: nothing is re-contracted,
// and a loaded xi and a drawn xi go through the same instructions):
//     t = eps + g ;  u = fma(-coef, t, eps), coef = 0.5f * step * step ;  new = fma(step, xi, u)  (only with noise / rng)
template <class C, int ST, bool UPDATE>
__global__ __launch_bounds__(256, 1) void LSNF_S3R_KERNEL(const LSNF_S3R_ARGS a) {
    constexpr int HT = C::HT, WT = C::WT, NZT = C::NZT, NU2 = C::NU2, LASTU = NU2 - 1;
    using L = Small3RbwdLds<C, ST>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* GTP = smem + L::L_GTP;
    float* GA2 = smem + L::L_GA2;
    float* GA1 = GTP;                                                     // (see Small3RbwdLds)
    float* GVA = smem + L::L_GVA;
    float* GVB = smem + L::L_GVB;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int vec4 = a.vec4;

    // a wave without a unit of its own (HT = 1: waves 2, 3) computes unit 0 again and stores the same values to the same LDS
    // words: no branch in the stages (global stores stay under has1)
    const bool has1 = wave < 2 * HT;
    const int hu1 = has1 ? wave : 0, nt1 = hu1 >> 1, ft1 = hu1 & 1;
    int hw[NU2];
#pragma unroll
    for (int i = 0; i < NU2; ++i) hw[i] = (wave + 4 * i < 2 * WT) ? wave + 4 * i : 0;

    const int last = a.depth - 1;
    long sample[ST]; bool live[ST]; long row[ST];
    size_t wtile[ST]; int lane32[ST];
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        const size_t q = (size_t)blockIdx.x * ST + st;                    // 16-row tile q = half (q & 1) of the 32-sample stash tile q >> 1
        sample[st] = (long)q * S3_SAMPLES + n;
        live[st] = sample[st] < a.B;
        row[st] = live[st] ? sample[st] : (long)a.B - 1;
        wtile[st] = ((long)q * S3_SAMPLES < (long)a.B) ? (q >> 1) : 0;    // (a tile past the batch reads stash tile 0: never stored)
        lane32[st] = 16 * (int)(q & 1) + n + 32 * (g & 1);
    }
    const LsnfActLayout al = lsnf_act_layout(a.B, HT, WT);
    const int nibsh_base = 4 * (g >> 1);                                   // + 8*ft: bit offset of this lane's nibble in a mask word

    // a block's stash slice and block output (this wave's second-half unit), fetched one block ahead of their use
    f32x4 y2[ST], sg[ST]; unsigned m1[NU2][ST], m2[NU2][ST];
    auto fetch_block_state = [&](int blk) {
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            const float* act = a.act_saved + (size_t)blk * al.per_block + wtile[st] * al.per_tile;
            const float* ysrc = (blk == a.depth - 1) ? a.z_out + row[st] * (long)a.nz : a.z_saved + ((size_t)blk * a.B + row[st]) * a.nz;
            y2[st] = load_row_half<HT>(HT + nt1, ft1, ysrc, a.half, g, vec4);
            sg[st] = reinterpret_cast<const f32x4*>(act + (size_t)nt1 * 1024)[(2 * ft1 + (g >> 1)) * 64 + lane32[st]];
            const unsigned* words = reinterpret_cast<const unsigned*>(act + al.mask_off);
#pragma unroll
            for (int i = 0; i < NU2; ++i) {
                const int nt = hw[i] >> 1, ft = hw[i] & 1;
                m1[i][st] = (words[nt * 64 + lane32[st]] >> (nibsh_base + 8 * ft)) & 0xFu;
                m2[i][st] = (words[(WT + nt) * 64 + lane32[st]] >> (nibsh_base + 8 * ft)) & 0xFu;
            }
        }
    };
    // what the gradient needs first goes out first (vmcnt completes in order): the upstream gradient, the first block's stash
    // slice, then the weights in order of use
    float go[ST];
    f32x4 g1[ST], g2[ST];
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        go[st] = a.g_obj ? a.g_obj[row[st]] : 0.0f;
        if (a.g_x) {
            g1[st] = load_row_half<HT>(nt1, ft1, a.g_x + row[st] * (long)a.nz, a.half, g, vec4);
            g2[st] = load_row_half<HT>(HT + nt1, ft1, a.g_x + row[st] * (long)a.nz, a.half, g, vec4);
        } else { g1[st] = rb_zero4(); g2[st] = rb_zero4(); }
    }
    fetch_block_state(0);
    __builtin_amdgcn_sched_barrier(0);
    UFrags<NZT> wt1a = fetch_unit<NZT>(a.tpanels, nt1, ft1, lane);
    UFrags<NZT> wt1b = fetch_unit<NZT>(a.tpanels, HT + nt1, ft1, lane);
    UFrags<2 * HT> wb4[NU2];
    UFrags<WT> wb3[NU2];
#pragma unroll
    for (int i = 0; i < NU2; ++i) wb4[i] = fetch_unit<2 * HT>(a.panels + C::OFFB4, hw[i] >> 1, hw[i] & 1, lane);
#pragma unroll
    for (int i = 0; i < NU2; ++i) wb3[i] = fetch_unit<WT>(a.panels + C::OFFB3, hw[i] >> 1, hw[i] & 1, lane);
    UFrags<WT> wb2 = fetch_unit<WT>(a.panels + C::OFFB2, nt1, ft1, lane);
    __builtin_amdgcn_sched_barrier(0);

    // the upstream gradient as the first block's T1 operand (buffer 0 of the second half)
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        store_half(GVA + st * L::GH + nt1 * S3_BTILE_FLOATS, ft1, g1[st], lane);
        store_half(GVB + st * L::GH + nt1 * S3_BTILE_FLOATS, ft1, g2[st], lane);
    }
    __syncthreads();

    f32x4 gv1[ST], gv2[ST];
    f32x4 e1[UPDATE ? ST : 1];                                            // UPDATE: the first half of this wave's unit of eps (the second is y2)
    for (int blk = 0; blk <= last; ++blk) {
        const int nb = blk < last ? blk + 1 : last;                         // the last block re-fetches its own panels: no loads under a branch
        const float* gb = a.panels + (size_t)blk * C::BLOCKB;
        const float* gbn = a.panels + (size_t)nb * C::BLOCKB;
        const float* tbn = a.tpanels + (size_t)nb * C::BLOCKT;
        float* gvb_cur = GVB + (blk & 1) * ST * L::GH;
        float* gvb_nxt = GVB + ((blk + 1) & 1) * ST * L::GH;

        // ---- T1: g_v = Winv' g; under its last steps: the inverse coupling's Jacobian (CB') ----
        {
#pragma unroll
            for (int st = 0; st < ST; ++st) { gv1[st] = rb_zero4(); gv2[st] = rb_zero4(); }
            auto coupling = [&](int st) {
#pragma clang fp contract(off)
                f32x4 gt, gp, gy;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    gy[r] = gv2[st][r] / sg[st][r];
                    gt[r] = -gv2[st][r];
                    gp[r] = -((1.0f - sg[st][r]) * (gy[r] * y2[st][r] + go[st]));
                }
                g2[st] = gy;
                store_half(GTP + st * L::TP + nt1 * S3_BTILE_FLOATS, ft1, gt, lane);
                store_half(GTP + st * L::TP + (HT + nt1) * S3_BTILE_FLOATS, ft1, gp, lane);
                store_half(gvb_nxt + st * L::GH + nt1 * S3_BTILE_FLOATS, ft1, gy, lane);         // the next block's T1 operand
            };
            // carry: the last k-tile of B2's unit, THIS block's fragments (B2 runs last in a block)
            const bf16x8* cp = unit_ptr<WT>(gb + C::OFFB2, nt1, ft1, lane);
            units_mma_st<NZT, 0, NZT, ST, 2, 48, 3, 0, HT>(gv1, gv2, wt1a, wt1b, unit_ptr<NZT>(tbn, nt1, ft1, lane),
                unit_ptr<NZT>(tbn, HT + nt1, ft1, lane), GVA, L::GH, lane,
                [&](int st) { coupling(st); },
                [&](int q) { refill_last<WT>(wb2, cp, q); }, [](int) {}, gvb_cur);
        }
        __syncthreads();
        // ---- B4: g_a2 = ([W3s W3p][g_t; g_p]) gated by h2 > 0 ----
#pragma unroll
        for (int i = 0; i < NU2; ++i) {
            const int nt = hw[i] >> 1, ft = hw[i] & 1;
            f32x4 ga[ST];
#pragma unroll
            for (int st = 0; st < ST; ++st) ga[st] = rb_zero4();
            auto epi = [&](int st) {
                ga[st] = rb_mask4(ga[st], m2[i][st]);
                store_half(GA2 + st * L::HL + nt * S3_BTILE_FLOATS, ft, ga[st], lane);
            };
            const bf16x8* rf = unit_ptr<2 * HT>(gbn + C::OFFB4, nt, ft, lane);
            if (i == 0) {        // carry: the last k-tile of T1's two units (next block's fragments)
                const bf16x8* c1a = unit_ptr<NZT>(tbn, nt1, ft1, lane);
                const bf16x8* c1b = unit_ptr<NZT>(tbn, HT + nt1, ft1, lane);
                units_mma_st<2 * HT, 0, 2 * HT, ST, 1, 26, 6, 0>(ga, ga, wb4[i], wb4[i], rf, nullptr, GTP, L::TP, lane, epi,
                    [&](int q) { if (q < 3) refill_last<NZT>(wt1a, c1a, q); else refill_last<NZT>(wt1b, c1b, q - 3); }, [](int) {});
            } else {
                const bf16x8* cp = unit_ptr<2 * HT>(gbn + C::OFFB4, hw[i > 0 ? i - 1 : 0] >> 1, hw[i > 0 ? i - 1 : 0] & 1, lane);
                units_mma_st<2 * HT, 0, 2 * HT, ST, 1, 26, 3, 0>(ga, ga, wb4[i], wb4[i], rf, nullptr, GTP, L::TP, lane, epi,
                    [&](int q) { refill_last<2 * HT>(wb4[i > 0 ? i - 1 : 0], cp, q); }, [](int) {});
            }
        }
        __syncthreads();
        // ---- B3: g_a1 = (W2' g_a2) gated by h1 > 0 ----
#pragma unroll
        for (int i = 0; i < NU2; ++i) {
            const int nt = hw[i] >> 1, ft = hw[i] & 1;
            f32x4 ga[ST];
#pragma unroll
            for (int st = 0; st < ST; ++st) ga[st] = rb_zero4();
            auto epi = [&](int st) {
                ga[st] = rb_mask4(ga[st], m1[i][st]);
                store_half(GA1 + st * L::TP + nt * S3_BTILE_FLOATS, ft, ga[st], lane);
            };
            const bf16x8* rf = unit_ptr<WT>(gbn + C::OFFB3, nt, ft, lane);
            if (i == 0) {        // carry: the last k-tile of B4's last unit (next block's fragments)
                const bf16x8* cp = unit_ptr<2 * HT>(gbn + C::OFFB4, hw[LASTU] >> 1, hw[LASTU] & 1, lane);
                units_mma_st<WT, 0, WT, ST, 1, 26, 3, 0>(ga, ga, wb3[i], wb3[i], rf, nullptr, GA2, L::HL, lane, epi,
                    [&](int q) { refill_last<2 * HT>(wb4[LASTU], cp, q); }, [](int) {});
            } else {
                const bf16x8* cp = unit_ptr<WT>(gbn + C::OFFB3, hw[i > 0 ? i - 1 : 0] >> 1, hw[i > 0 ? i - 1 : 0] & 1, lane);
                units_mma_st<WT, 0, WT, ST, 1, 26, 3, 0>(ga, ga, wb3[i], wb3[i], rf, nullptr, GA2, L::HL, lane, epi,
                    [&](int q) { refill_last<WT>(wb3[i > 0 ? i - 1 : 0], cp, q); }, [](int) {});
            }
        }
        __syncthreads();
        // ---- B2: g_y1 = g_v1 (direct) + W1' g_a1.  The next block's stash slice / output rows are requested here ----
        fetch_block_state(nb);                                             // (this block's are consumed: CB' ran in T1, the masks in B4 / B3)
        if constexpr (UPDATE) {
            if (blk == last) {                                             // (kernel-uniform) with the last block's re-fetch of y2 = eps, second half
#pragma unroll
                for (int st = 0; st < ST; ++st) e1[st] = load_row_half<HT>(nt1, ft1, a.z_out + row[st] * (long)a.nz, a.half, g, vec4);
            }
        }
        {
#pragma unroll
            for (int st = 0; st < ST; ++st) g1[st] = gv1[st];
            const bf16x8* cp = unit_ptr<WT>(gbn + C::OFFB3, hw[LASTU] >> 1, hw[LASTU] & 1, lane);
            units_mma_st<WT, 0, WT, ST, 1, 24, 3, 0>(g1, g1, wb2, wb2, unit_ptr<WT>(gbn + C::OFFB2, nt1, ft1, lane), nullptr, GA1, L::TP, lane,
                [&](int st) { store_half(GVA + st * L::GH + nt1 * S3_BTILE_FLOATS, ft1, g1[st], lane); },   // (after the last block: nobody reads it)
                [&](int q) { refill_last<WT>(wb3[LASTU], cp, q); }, [](int) {});
        }
        __syncthreads();
    }

    LSNF_S3R_TAIL

    // ---- output: g on the reverse's input ----
    if constexpr (!UPDATE) {
        if (has1) {
#pragma unroll
            for (int st = 0; st < ST; ++st) {
                if (live[st]) {
                    float* gr = a.g_z_in + sample[st] * (long)a.nz;
                    store_row_half<HT>(nt1, ft1, g1[st], gr, a.half, g, vec4);
                    store_row_half<HT>(HT + nt1, ft1, g2[st], gr, a.half, g, vec4);
                }
            }
        }
    } else {
        // ---- output: the Langevin update of eps (every read of the workgroup's rows of z_out was issued before the last barrier and
        // is of the columns this lane stores: eps_new may be z_out) ----
        const bool norms = a.g_norm || a.eps_norm;                         // kernel-uniform
        const bool noisy = a.noise || a.rng.enabled;
        const LsnfRngState rs = (!a.noise && a.rng.enabled) ? lsnf_rng_state(a.rng) : LsnfRngState{0u, 0u, 0u, 0u, 0};
        const float coef = __fmul_rn(__fmul_rn(0.5f, a.step), a.step);
        float* RED = GTP;                                                  // (dead since the last barrier; ST * 4 * 16 * 2 floats of ST * TP)
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            float gn2 = 0.0f, en2 = 0.0f;
            if (has1) {
                if (live[st] && a.g_z_in) {
                    float* gr = a.g_z_in + sample[st] * (long)a.nz;
                    store_row_half<HT>(nt1, ft1, g1[st], gr, a.half, g, vec4);
                    store_row_half<HT>(HT + nt1, ft1, g2[st], gr, a.half, g, vec4);
                }
#pragma unroll
                for (int hs = 0; hs < 2; ++hs) {                           // this wave's first-half and second-half unit
                    const int t = hs * HT + nt1;
                    const f32x4 gq = hs ? g2[st] : g1[st];
                    const f32x4 ec = hs ? y2[st] : e1[st];
                    f32x4 xi = rb_zero4();
                    if (a.noise) {
                        xi = load_row_half<HT>(t, ft1, a.noise + row[st] * (long)a.nz, a.half, g, vec4);
                    } else if (rs.on) {     // the same draws as every other kernel (lsnf_device.h): lsnf_sample's eps at temperature 1
                        float unused = 0.0f;
                        xi = lsnf_sample4(hs, 32 * nt1 + 16 * ft1 + 4 * g, a.half, (unsigned long long)(a.rng.row0 + sample[st]), rs, 1.0f, unused);
                    }
                    f32x4 en;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        gn2 = __fmaf_rn(gq[r], gq[r], gn2); en2 = __fmaf_rn(ec[r], ec[r], en2);
                        const float u = __fmaf_rn(-coef, __fadd_rn(ec[r], gq[r]), ec[r]);
                        en[r] = noisy ? __fmaf_rn(a.step, xi[r], u) : u;
                    }
                    if (live[st]) store_row_half<HT>(t, ft1, en, a.eps_new + sample[st] * (long)a.nz, a.half, g, vec4);
                }
            }
            if (norms) {                                                   // per-row norms: over the 4 lane groups, then over the waves
                gn2 = group_sum(gn2); en2 = group_sum(en2);
                if (g == 0) { RED[((st * 4 + wave) * 16 + n) * 2] = gn2; RED[((st * 4 + wave) * 16 + n) * 2 + 1] = en2; }
            }
        }
        if (norms) {
            __syncthreads();
            if (wave == 0 && g == 0) {
#pragma unroll
                for (int st = 0; st < ST; ++st) {
                    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
                    for (int w = 0; w < 4; ++w) { s1 += RED[((st * 4 + w) * 16 + n) * 2]; s2 += RED[((st * 4 + w) * 16 + n) * 2 + 1]; }
                    if (live[st]) {
                        if (a.g_norm) a.g_norm[sample[st]] = sqrtf(s1);
                        if (a.eps_norm) a.eps_norm[sample[st]] = sqrtf(s2);
                    }
                }
            }
        }
    }
}

// (shapes that do not fit are not instantiated; the LDS footprint does not depend on the depth, and ST = 1 always fits)
template <class C, int ST>
constexpr bool small3_rbwd_built = (size_t)Small3RbwdLds<C, ST>::L_END * sizeof(float) <= 160 * 1024;
static_assert(small3_rbwd_built<Small3RbwdCfg<1, 1>, 1> && small3_rbwd_built<Small3RbwdCfg<2, 2>, 1> && small3_rbwd_built<Small3RbwdCfg<2, 4>, 1>);

}  // namespace

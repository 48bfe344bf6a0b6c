// lsnf_fwd3.hip -- the fused forward of lsnf_fwd.hip with its GEMMs on the bf16 matrix pipe at fp32 accuracy.
//
// Same math, same interface and same register layout as lsnf_fwd.hip (replaces reference model.py:473-483 +
// train.py:317-319); what changes is how a product  acc += W^T x  is evaluated.  fp32 MFMA
// (v_mfma_f32_32x32x2_f32) peaks at 157 TFLOP/s on MI355X, the bf16 MFMA (v_mfma_f32_32x32x16_bf16) at 2.5 PFLOP/s,
// 16x.  Both operands are split error-free into three bf16 terms,
//       w = w1 + w2 + w3,   x = x1 + x2 + x3      (each term the round-to-nearest bf16 of what is left),
// and the product keeps the six terms of weight >= 2^-18:
//       w x ~= w1 x1 + w1 x2 + w2 x1 + w2 x2 + w1 x3 + w3 x1,
// every bf16 x bf16 product being exact in the MFMA's fp32 accumulator.  The dropped terms are <= 2^-26 |w||x|,
// below the 2^-24 rounding of an fp32 product: the log-prob error against float64 is the same 2-3e-7 as the fp32
// MFMA path's (tools/study/split_bf16_accuracy.py, tests/test_gpu_forward.py) -- this is NOT a reduced-precision
// mode.  Six MFMAs of K = 16 replace eight of K = 2 x 8: 2.6x the fp32 MFMA rate (tools/micro/mfma_bf16.hip);
// the weights are split once in lsnf_prepare (plan region off_f3b_panels, 6 KiB per 32x32 block instead of 4),
// the activations on the fly (4.5 VALU per element: v_cvt_pk_bf16_f32, shift/and, v_pk_add_f32).
//
// Work decomposition: one workgroup per CU (the two 48 KiB weight buffers do not fit twice) of 8 waves (batches above
// 32 768 rows) or 4 waves, wave = 32 samples; weights stream L2 -> LDS by LDS-DMA in panel pairs exactly as in lsnf_fwd.hip.  Because the k-slot j of
// lane-half h in k-step s is accumulator register 8*s + j (lsnf_layout.h), an output tile converted to bf16 pairs in
// register order is directly the next GEMM's B operand.
#include <stdlib.h>
#include "lsnf_l16.h"
#include "lsnf_launch.h"

namespace {



template <int HT_, int WT_>
struct Fwd3Cfg : LsnfStackCfg<HT_, WT_> {
    using S = LsnfStackCfg<HT_, WT_>;
    static constexpr int F = L16_FRAG_FLOATS;
    static constexpr int OFF3_S2 = F * S::P1 * S::KT1;
    static constexpr int OFF3_S3 = OFF3_S2 + F * S::P2 * S::KT2;
    static constexpr int OFF3_S4 = OFF3_S3 + F * S::P3 * S::KT3;
    static constexpr int BLOCK3 = OFF3_S4 + F * S::P4 * S::KT4;
    static constexpr int SLOT3 = 2 * S::MAXKT * F;            // LDS floats of one panel pair
    static constexpr int CONST_FLOATS = S::FWD_CONST;
};

struct Fwd3Args {
    const float* consts; const float* panels3;
    const float* z_in; const float* objective;
    float* z_out; float* logdet_out; float* ll_out; float* z_saved; float* act_saved;
    int B, nz, half, n_blocks, vec4;
    double* stats;
    unsigned long long* stamps;        // LSNF_STAMPS diagnostic build only: [waves & 2047][64] clock stamps
    const unsigned* guard;             // fp16x2 kernel: the plan's guard words ([0]: weights outside fp16's range), read only
    int hdump_tiled;                   // h1 / h2 in the tiled form (lsnf_l16.h l16_store_tiled) instead of row-major
    float* hdump; int width;           // L16 kernels: NULL, or the parameter-gradient dump (LsnfDumpLayout): h1, h2 of every block
    int fixup;                         // bf16x3 L16 kernel: 1 = run as the fix-up pass of an fp16x2 launch: a workgroup
                                       // recomputes its rows only if one of its waves left LSNF_F16_SENTINEL_BITS in
                                       // logdet_out (lsnf_layout.h); the flag travels in the launch's own output
};

#ifdef LSNF_STAMPS   // in-kernel clock = d(s_memtime) / d(s_memrealtime) x 100 MHz (tools/stamps_fwd3.py)
#define F3_STAMP(i, INSN)                                                                               \
    do { __builtin_amdgcn_sched_barrier(0);                                                             \
         unsigned long long t_; asm volatile(INSN " %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory");  \
         __builtin_amdgcn_sched_barrier(0);                                                             \
         if (a.stamps && lane == 0) a.stamps[(((size_t)blockIdx.x * F3_WAVES + wave) & 2047) * 64 + (i)] = t_; } while (0)
#else
#define F3_STAMP(i, INSN) do {} while (0)
#endif

// =====================================================================================================================
// The kernel, on v_mfma_f32_16x16x32_bf16 ("L16" lane layout of lsnf_layout.h: a wave's 32 samples are two sample
// tiles st of 16; lane = (n = lane & 15, g = lane >> 4); register (2*ft + st)*4 + r of a 32-feature activation tile
// holds feature 16*ft + 4*g + r of sample 16*st + n).  Same flops, LDS traffic and register count as on 32x32x16 -- but on
// real data the chip sustains a higher clock under this MFMA shape (tools/micro/mfma_bf16_shapes.hip: +12 %).
// =====================================================================================================================
template <class C, int F3_WAVES>
__global__ __launch_bounds__(64 * F3_WAVES, 1) void lsnf_fwd3b_kernel(const Fwd3Args a) {
    constexpr int THREADS = 64 * F3_WAVES;
    constexpr int HT = C::HT, WT = C::WT, NZT = C::NZT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* cst = smem;
    float* buf0 = smem + a.n_blocks * C::CONST_FLOATS;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int n = lane & 15, g = lane >> 4;

    F3_STAMP(0, "s_memtime");
    F3_STAMP(50, "s_memrealtime");
    const int wbase = (blockIdx.x * F3_WAVES + wave) * 32;            // first row of this wave (B <= 2^28: 32-bit row indices)
#if LSNF_L16_PARTS == 3
    if (a.fixup) {                                // fix-up pass of the fp16 forward: only workgroups in which a wave raised its flag
        unsigned* fl = reinterpret_cast<unsigned*>(smem);
        unsigned f = 0u;
        if (wbase < a.B) f = __builtin_bit_cast(unsigned, a.logdet_out[(long)wbase]) == LSNF_F16_SENTINEL_BITS ? 1u : 0u;
        if (lane == 0) fl[wave] = f;
        __syncthreads();
        unsigned any = 0u;
#pragma unroll
        for (int w = 0; w < F3_WAVES; ++w) any |= fl[w];
        __syncthreads();                          // (smem is reused below)
        if (any == 0u) return;                    // workgroup-uniform
    }
#else
    if (a.guard[0] != 0u) {                       // weights outside fp16's range (prepare): leave every row to the fix-up pass
        if (lane == 0 && wbase < a.B) a.logdet_out[wbase] = __builtin_bit_cast(float, LSNF_F16_SENTINEL_BITS);
        return;
    }
    // Range guard.  An operand x with |x| >= 65520 splits into x1 = +-inf, x2 = x - x1 = -+inf, and every output of the
    // GEMM that consumes it becomes NaN (w*inf - w*inf, or 0*inf where w = 0): looking at ONE output register per
    // sample tile after each stage sees it -- before the ReLU, which would swallow the NaN (v_max_f32(NaN, 0) = 0).
    bool bad = false;
#endif
    Pipe3<F3_WAVES> pipe;
    pipe.buf0 = buf0; pipe.slot = C::SLOT3; pipe.wave = wave; pipe.lane = lane;
    pipe.template prime<first_kib(C::P1, C::KT1)>(a.panels3);

    int sample[2], rows[2]; bool live[2];
#pragma unroll
    for (int st = 0; st < 2; ++st) { sample[st] = wbase + 16 * st + n; live[st] = sample[st] < a.B; rows[st] = live[st] ? sample[st] : a.B - 1; }

    f32x16 x[NZT];
#pragma unroll
    for (int t = 0; t < NZT; ++t) x[t] = l16_load_tile<HT>(t, a.z_in, rows, a.nz, a.half, g, a.vec4);
    __builtin_amdgcn_sched_barrier(0);
    // (the constant blocks are copied AFTER the row loads have gone out: the copy waits for its loads in order, one memory
    //  round trip that the rows would otherwise start behind)
    for (int i = tid; i < a.n_blocks * C::CONST_FLOATS; i += THREADS) cst[i] = a.consts[i];
    float ell[2];
#pragma unroll
    for (int st = 0; st < 2; ++st) ell[st] = a.objective ? a.objective[rows[st]] : 0.0f;

    const LsnfActLayout al = lsnf_act_layout(a.B, HT, WT);
    const LsnfDumpLayout dl = lsnf_dump_layout(a.B, a.nz, a.width);
    const bool w4 = (a.width & 3) == 0;
    const size_t wtile = (size_t)blockIdx.x * F3_WAVES + wave;
    for (int blk = 0; blk < a.n_blocks; ++blk) {
        float* act = (a.act_saved && wtile * 32 < (size_t)a.B)
                         ? a.act_saved + (size_t)blk * al.per_block + wtile * al.per_tile : nullptr;
        const float* cb = cst + blk * C::CONST_FLOATS;
        const float* gblk = a.panels3 + (size_t)blk * C::BLOCK3;
        const bool more = blk + 1 < a.n_blocks;
        const float* gnext = more ? gblk + C::BLOCK3 : nullptr;
#if LSNF_L16_PARTS == 3
        auto keep = [](f32x16 acc, int) { return acc; };
        auto relu = [](f32x16 acc, int) { return lsnf_relu16(acc); };
#else
        auto keep = [&](f32x16 acc, int t) { if (t == 0) bad = bad || acc[0] != acc[0] || acc[4] != acc[4]; return acc; };
        auto relu = [&](f32x16 acc, int t) { if (t == 0) bad = bad || acc[0] != acc[0] || acc[4] != acc[4]; return lsnf_relu16(acc); };
#endif

        // ---- S1: v = Wa^T x + ca  (model.py:244,268,187) ----
        f32x16 v[NZT];
        {
            Split3 xs[2 * NZT];
            l16_split_tiles<NZT>(x, xs);
            l16_gemm_stage3<C::P1, C::KT1, first_kib(C::P2, C::KT2)>(
                pipe, gblk, gblk + C::OFF3_S2, v, xs, [&](int t) { return l16_bias_init(cb + 32 * t, g); }, keep);
        }
        // f_width 128 with two waves per SIMD (256 registers): the four split tiles of h1 / h2 (96 registers), four finished and two
        // running accumulators of S3 / S4 do not fit beside v (64): hipcc spills ~49 registers to scratch there.  Tried instead, and
        // removed: v1 / v2 parked in this wave's OWN z_out rows between S2's split and the end of the block -- that had zero scratch,
        // but 262 MB of extra row traffic per launch at B = 65 536: it measured 186 us against 153 us with hipcc's spills (bf16x3;
        // fp16x2 133 vs 92; two alternations on one box).  The compiler's choice of WHAT to spill was the cheaper one.
        if (!more) {     // last block: the v1 half is final (model.py:422) -- its stores drain under the MFMAs of S2..S4
#pragma unroll
            for (int t = 0; t < HT; ++t) l16_store_tile<HT>(t, v[t], a.z_out, sample, live, a.nz, a.half, g, a.vec4);
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) { ell[st] = ell[st] + cb[32 * C::NP + 0]; ell[st] = ell[st] + cb[32 * C::NP + 1]; }
        // ---- S2: h1 = relu(actnorm(v1 @ W1))  (model.py:326-328,307) ----
        f32x16 h1[WT];
        {
            Split3 vs[2 * HT];
            l16_split_tiles<HT>(v, vs);
            l16_gemm_stage3<C::P2, C::KT2, first_kib(C::P3, C::KT3)>(
                pipe, gblk + C::OFF3_S2, gblk + C::OFF3_S3, h1, vs,
                [&](int t) { return l16_bias_init(cb + 32 * (C::P1 + t), g); }, relu);
        }
        if (act) {
#pragma unroll
            for (int t = 0; t < WT; ++t) l16_store_masks(reinterpret_cast<unsigned*>(act + al.mask_off) + t * 64, h1[t], n, g);
        }
        if (a.hdump) {           // kernel-uniform: h1 for the batch contraction dW2' = h1^T g_a2 (lsnf_params.hip)
#pragma unroll
            for (int t = 0; t < WT; ++t) {
                if (a.hdump_tiled) { if (wtile * 32 < (size_t)a.B) l16_store_tiled(h1[t], a.hdump + (size_t)blk * dl.per_block + dl.off_h1, wtile, a.width, t, n, g); }
                else l16_store_plain(h1[t], a.hdump + (size_t)blk * dl.per_block + dl.off_h1, sample, live, a.width, t, g, w4);
            }
        }
        // ---- S3: h2 = relu(actnorm(h1 @ W2))  (model.py:326-328,308) ----
        f32x16 h2[WT];
        {
            Split3 hs[2 * WT];
            l16_split_tiles<WT>(h1, hs);
            l16_gemm_stage3<C::P3, C::KT3, first_kib(C::P4, C::KT4)>(
                pipe, gblk + C::OFF3_S3, gblk + C::OFF3_S4, h2, hs,
                [&](int t) { return l16_bias_init(cb + 32 * (C::P1 + C::P2 + t), g); }, relu);
        }
        if (act) {
#pragma unroll
            for (int t = 0; t < WT; ++t) l16_store_masks(reinterpret_cast<unsigned*>(act + al.mask_off) + (WT + t) * 64, h2[t], n, g);
        }
        if (a.hdump) {
#pragma unroll
            for (int t = 0; t < WT; ++t) {
                if (a.hdump_tiled) { if (wtile * 32 < (size_t)a.B) l16_store_tiled(h2[t], a.hdump + (size_t)blk * dl.per_block + dl.off_h2, wtile, a.width, t, n, g); }
                else l16_store_plain(h2[t], a.hdump + (size_t)blk * dl.per_block + dl.off_h2, sample, live, a.width, t, g, w4);
            }
        }
        // ---- S4: shift t / pre-sigmoid p = fc_zeros(h2), de-interleaved (model.py:347-349,411-413) ----
        f32x16 tp[2 * HT];
        {
            Split3 hs[2 * WT];
            l16_split_tiles<WT>(h2, hs);
            l16_gemm_stage3<C::P4, C::KT4, first_kib(C::P1, C::KT1)>(
                pipe, gblk + C::OFF3_S4, gnext, tp, hs,
                [&](int t) { return l16_bias_init(cb + 32 * (C::P1 + C::P2 + C::P3 + t), g); }, keep);
        }
        // ---- coupling + per-sample log-scale reduction (model.py:414-418), concat (:422) ----
        float lsum[2] = {0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            x[t] = v[t];
            f32x16 sg;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float sig, l2;
                lsnf_sigmoid_log2(tp[HT + t][r], sig, l2);
                x[HT + t][r] = (v[HT + t][r] + tp[t][r]) * sig;
                sg[r] = sig;
                lsum[(r >> 2) & 1] += l2;                      // register (2*ft + st)*4 + r': sample tile st = bit 2
            }
            if (act) l16_store_sigma(act, t, sg, n, g);
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) ell[st] = ell[st] + -0.6931471805599453f * l16_group_sum(lsum[st]);
        if (a.z_saved != nullptr && more) {
#pragma unroll
            for (int t = 0; t < NZT; ++t)
                l16_store_tile<HT>(t, x[t], a.z_saved + (size_t)blk * a.B * a.nz, sample, live, a.nz, a.half, g, a.vec4);
        }
    }

    // ---- epilogue: z_out, logdet, ll = -0.5*sum z^2 + log(2pi) + logdet (train.py:317-319) ----
    float ss[2] = {0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < NZT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) ss[(r >> 2) & 1] += x[t][r] * x[t][r];
#pragma unroll
    for (int t = HT; t < NZT; ++t) l16_store_tile<HT>(t, x[t], a.z_out, sample, live, a.nz, a.half, g, a.vec4);
#if LSNF_L16_PARTS == 2
    // an operand at or beyond fp16's range (NaN compares false: it propagates by itself): this wave's results are not to
    // be trusted -- its first logdet element carries the flag, the bf16x3 fix-up pass queued behind recomputes the workgroup
    const bool wave_bad = __builtin_amdgcn_ballot_w64(bad) != 0ull;
#endif
    float ll[2];
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        ll[st] = (-0.5f * l16_group_sum(ss[st]) + 1.8378770664093453f) + ell[st];
        if (live[st] && g == 0) {
            int smp = sample[st];
            asm volatile("" : "+v"(smp));       // (keeps hipcc from forming the two store addresses in the prologue and carrying
                                                //  them -- 4 registers -- through the whole stack: they were the last scratch spill)
            float ld = ell[st];
#if LSNF_L16_PARTS == 2
            if (wave_bad && st == 0 && n == 0) ld = __builtin_bit_cast(float, LSNF_F16_SENTINEL_BITS);
#endif
            a.logdet_out[smp] = ld;
            if (a.ll_out) a.ll_out[smp] = ll[st];
        }
    }
    if (a.stats) {   // kernel-uniform: batch sums of ll and logdet, one pair of fp64 atomics per workgroup
        double dl = 0.0, dd = 0.0;
#pragma unroll
        for (int st = 0; st < 2; ++st)
            if (live[st] && g == 0) { dl += (double)ll[st]; dd += (double)ell[st]; }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { dl += __shfl_xor(dl, o, 64); dd += __shfl_xor(dd, o, 64); }
        __syncthreads();
        double* red = reinterpret_cast<double*>(buf0);
        if (lane == 0) { red[2 * wave] = dl; red[2 * wave + 1] = dd; }
        __syncthreads();
        if (wave == 0) {         // (all 64 lanes: lsnf_publish_stats is a wave-level protocol)
            double tl = 0.0, td = 0.0;
            for (int w = 0; w < F3_WAVES; ++w) { tl += red[2 * w]; td += red[2 * w + 1]; }
            lsnf_publish_stats(a.stats, tl, td, a.B, lane);
        }
    }
    F3_STAMP(41, "s_memtime");
    F3_STAMP(51, "s_memrealtime");
}

template <class C>
size_t fwd3_lds(int n_blocks) { return ((size_t)n_blocks * C::CONST_FLOATS + 2 * (size_t)C::SLOT3) * sizeof(float); }

template <class C, int F3_WAVES>
hipError_t launch_fwd3_w(const Fwd3Args& a, hipStream_t stream) {
    return lsnf_launch_kernel<lsnf_fwd3b_kernel<C, F3_WAVES>>(lsnf_grid(a.B, 32 * F3_WAVES), 64 * F3_WAVES, fwd3_lds<C>(a.n_blocks), stream, a);
}
template <class C>
hipError_t launch_fwd3(const Fwd3Args& a, hipStream_t stream) {
    return lsnf_eight_waves(a.B) ? launch_fwd3_w<C, 8>(a, stream) : launch_fwd3_w<C, 4>(a, stream);
}
}  // namespace

#ifndef LSNF_FWD3_ENTRY
#define LSNF_FWD3_ENTRY lsnf_launch_forward3
#define LSNF_FWD3_COVERS lsnf_forward3_covers
#endif
// Does LSNF_FWD3_ENTRY take this call (host only, no HIP calls; lsnf_api.hip selects by it)?  The constants of n_blocks blocks
// and a panel pair fit in 160 KiB of LDS; no in-kernel batch sums in the fix-up pass (a partial recomputation cannot repair
// them), nor ever in the fp16x2 kernel.
bool LSNF_FWD3_COVERS(const LsnfForwardCall& c, int fixup) {
#if LSNF_L16_PARTS == 3
    if (fixup && c.stats) return false;
#else
    if (c.stats) return false;
#endif
    return lsnf_with_cfg<Fwd3Cfg>(c.g, [&](auto cfg) { return fwd3_lds<decltype(cfg)>(c.n_blocks) <= 160 * 1024; });
}

hipError_t LSNF_FWD3_ENTRY(const LsnfForwardCall& c, int fixup) {
    if (!LSNF_FWD3_COVERS(c, fixup)) return hipErrorInvalidValue;    // (a selection bug)
    Fwd3Args a;
    lsnf_fill_forward(a, c);
    a.hdump_tiled = c.hdump_tiled; a.hdump = lsnf_hdump_at(c); a.width = c.g.width;
    a.fixup = fixup; a.guard = lsnf_guard_words(c);
#if LSNF_L16_PARTS == 3
    a.panels3 = lsnf_f3b_panels_at(c);
#else
    a.panels3 = lsnf_f2h_panels_at(c);
#endif
    a.stamps = lsnf_stamps_buffer();
    return lsnf_with_cfg<Fwd3Cfg>(c.g, [&](auto cfg) { return launch_fwd3<decltype(cfg)>(a, c.stream); });
}

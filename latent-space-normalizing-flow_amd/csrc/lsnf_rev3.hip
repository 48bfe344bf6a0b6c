// lsnf_rev3.hip -- throughput reverse (sampling) pass on the bf16 matrix pipe: the bf16x3 split and L16 lane layout of
// lsnf_fwd3.hip's 16x16x32 kernel applied to lsnf_rev.hip (replaces reference model.py:484-498 / :424-456).
// Per block, last to first, a wave owning 32 samples and all features:
//   R2,R3,R4 : h = f(z1) -> [t; p]                                (forward panels S2..S4, 16x16x32 operand order)
//   CI       : z2 = z2 / sigmoid(p) - t ; objective -= sum log sigmoid(p)     (model.py:436-438)
//   I1       : z = ([z1,z2] @ W^-1) * exp(-3 logs) - b ; objective -= log|det W| + sum 3 logs  (:193-196, 270, 246)
#include <stdlib.h>
#include "lsnf_l16.h"
#include "lsnf_launch.h"

namespace {

template <int HT_, int WT_>
struct Rev3Cfg : LsnfStackCfg<HT_, WT_> {
    using S = LsnfStackCfg<HT_, WT_>;
    static constexpr int F = L16_FRAG_FLOATS;
    static constexpr int OFF3_S2 = F * S::P1 * S::KT1;
    static constexpr int OFF3_S3 = OFF3_S2 + F * S::P2 * S::KT2;
    static constexpr int OFF3_S4 = OFF3_S3 + F * S::P3 * S::KT3;
    static constexpr int BLOCK3 = OFF3_S4 + F * S::P4 * S::KT4;
    static constexpr int BLOCKI = F * S::NZT * S::NZT;
    static constexpr int CONST_PER_BLOCK = S::FWD_CONST + S::INV_CONST;
    static constexpr int SLOT3 = 2 * S::MAXKT * F;
};

struct Rev3Args {
    const float* fwd_consts; const float* inv_consts; const float* panels3b; const float* ipanels3b;
    const float* z_in; const float* objective; float* z_out; float* objective_out;
    int B, nz, half, depth, vec4;
    const unsigned* guard; int fixup;        // fp16 range guard, as in lsnf_fwd3.hip (Fwd3Args); the flag travels in z_out[first row of the wave][0]
};
struct Rev3SampleArgs : Rev3Args { LsnfSampleArgs s; };      // lsnf_sample: z_in / objective are unused (NULL)

// SAMPLE: the rows are drawn where they would be loaded (lsnf_sample); every other instruction is lsnf_reverse's.  As the
// fix-up pass of the fp16 reverse it redraws the rows of the workgroups it recomputes: the draw is a pure function.
template <class C, int NW, bool SAMPLE>
__global__ __launch_bounds__(64 * NW, 1) void lsnf_rev3_kernel(const std::conditional_t<SAMPLE, Rev3SampleArgs, Rev3Args> a) {
    constexpr int HT = C::HT, WT = C::WT, NZT = C::NZT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* cst = smem;                                         // depth * CONST_PER_BLOCK
    float* buf0 = smem + a.depth * C::CONST_PER_BLOCK;         // 2 x SLOT3
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int vec4 = a.vec4;
    const long wbase = ((long)blockIdx.x * NW + wave) * 32;           // first row of this wave
#if LSNF_L16_PARTS == 3
    if (a.fixup) {                                // fix-up pass of the fp16 reverse: only workgroups in which a wave raised its flag
        unsigned* fl = reinterpret_cast<unsigned*>(smem);
        unsigned f = 0u;
        if (wbase < a.B) f = __builtin_bit_cast(unsigned, a.z_out[wbase * (long)a.nz]) == LSNF_F16_SENTINEL_BITS ? 1u : 0u;
        if (lane == 0) fl[wave] = f;
        __syncthreads();
        unsigned any = 0u;
#pragma unroll
        for (int w = 0; w < NW; ++w) any |= fl[w];
        __syncthreads();                          // (smem is reused below)
        if (any == 0u) return;                    // workgroup-uniform
    }
#else
    if (a.guard[0] != 0u) {                       // weights outside fp16's range (prepare): leave every row to the fix-up pass
        if (lane == 0 && wbase < a.B) a.z_out[wbase * (long)a.nz] = __builtin_bit_cast(float, LSNF_F16_SENTINEL_BITS);
        return;
    }
    bool bad = false;                             // an operand beyond fp16's range turns every output of its GEMM into NaN
#endif

    const int last = a.depth - 1;
    Pipe3<NW> pipe;
    pipe.buf0 = buf0; pipe.slot = C::SLOT3; pipe.wave = wave; pipe.lane = lane;
    pipe.template prime<first_kib(C::P2, C::KT2)>(a.panels3b + (size_t)last * C::BLOCK3 + C::OFF3_S2);

    const long base = ((long)blockIdx.x * NW + wave) * 32;
    long sample[2], rows[2]; bool live[2];
#pragma unroll
    for (int st = 0; st < 2; ++st) { sample[st] = base + 16 * st + n; live[st] = sample[st] < a.B; rows[st] = live[st] ? sample[st] : (long)a.B - 1; }

    f32x16 x[NZT];
    float llp[2] = {0.0f, 0.0f};                                      // SAMPLE: -0.5 * sum eps^2 + log(2 pi) of the two rows
    if constexpr (SAMPLE) {
        const LsnfRngState rs = lsnf_rng_state(a.s.rng);
        const unsigned long long grow[2] = {(unsigned long long)(a.s.rng.row0 + sample[0]), (unsigned long long)(a.s.rng.row0 + sample[1])};
        float ss[2] = {0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < NZT; ++t) x[t] = l16_sample_tile<HT>(t, grow, a.half, g, rs, a.s.temperature, ss);
#pragma unroll
        for (int st = 0; st < 2; ++st) llp[st] = -0.5f * l16_group_sum(ss[st]) + LSNF_LOG_2PI;
    } else {
#pragma unroll
        for (int t = 0; t < NZT; ++t) x[t] = l16_load_tile<HT>(t, a.z_in, rows, a.nz, a.half, g, vec4);
    }
    __builtin_amdgcn_sched_barrier(0);
    // (the constant blocks are copied AFTER the row loads have gone out: the copy waits for its loads in order, one memory
    //  round trip that the rows would otherwise start behind)
    for (int i = tid; i < a.depth * C::CONST_PER_BLOCK; i += 64 * NW) {
        const int blk = i / C::CONST_PER_BLOCK, r = i % C::CONST_PER_BLOCK;
        cst[i] = r < C::FWD_CONST ? a.fwd_consts[blk * C::FWD_CONST + r] : a.inv_consts[blk * C::INV_CONST + (r - C::FWD_CONST)];
    }
    if constexpr (SAMPLE) {              // (behind the constants: their copy waits for every access before it)
        if (a.s.eps_out) {
#pragma unroll
            for (int t = 0; t < NZT; ++t) l16_store_tile<HT>(t, x[t], a.s.eps_out, sample, live, a.nz, a.half, g, vec4);
        }
    }
    float obj[2];
#pragma unroll
    for (int st = 0; st < 2; ++st) obj[st] = a.objective ? a.objective[rows[st]] : 0.0f;
#if LSNF_L16_PARTS == 3
    auto keep = [](f32x16 acc, int) { return acc; };
    auto relu = [](f32x16 acc, int) { return lsnf_relu16(acc); };
#else
    auto keep = [&](f32x16 acc, int t) { if (t == 0) bad = bad || acc[0] != acc[0] || acc[4] != acc[4]; return acc; };
    auto relu = [&](f32x16 acc, int t) { if (t == 0) bad = bad || acc[0] != acc[0] || acc[4] != acc[4]; return lsnf_relu16(acc); };
#endif

    for (int blk = last; blk >= 0; --blk) {
        const float* cb = cst + blk * C::CONST_PER_BLOCK;
        const float* ci = cb + C::FWD_CONST;
        const float* gf = a.panels3b + (size_t)blk * C::BLOCK3;
        const float* gi = a.ipanels3b + (size_t)blk * C::BLOCKI;
        const float* gnext = blk > 0 ? a.panels3b + (size_t)(blk - 1) * C::BLOCK3 + C::OFF3_S2 : nullptr;

        // ---- R2: h1 = relu(W1'^T z1 + c1) ----
        f32x16 h1[WT];
        {
            Split3 zs[2 * HT];
            l16_split_tiles<HT>(x, zs);
            l16_gemm_stage3<C::P2, C::KT2, first_kib(C::P3, C::KT3)>(
                pipe, gf + C::OFF3_S2, gf + C::OFF3_S3, h1, zs, [&](int t) { return l16_bias_init(cb + 32 * (C::P1 + t), g); }, relu);
        }
        // ---- R3 ----
        f32x16 h2[WT];
        {
            Split3 hs[2 * WT];
            l16_split_tiles<WT>(h1, hs);
            l16_gemm_stage3<C::P3, C::KT3, first_kib(C::P4, C::KT4)>(
                pipe, gf + C::OFF3_S3, gf + C::OFF3_S4, h2, hs,
                [&](int t) { return l16_bias_init(cb + 32 * (C::P1 + C::P2 + t), g); }, relu);
        }
        // ---- R4: [t; p] ----
        f32x16 tp[2 * HT];
        {
            Split3 hs[2 * WT];
            l16_split_tiles<WT>(h2, hs);
            l16_gemm_stage3<C::P4, C::KT4, first_kib(NZT, NZT)>(
                pipe, gf + C::OFF3_S4, gi, tp, hs,
                [&](int t) { return l16_bias_init(cb + 32 * (C::P1 + C::P2 + C::P3 + t), g); }, keep);
        }
        // ---- inverse coupling (model.py:436-438) ----
        float lsum[2] = {0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float sig, lsig;
                lsnf_sigmoid_logsig(tp[HT + t][r], sig, lsig);
                x[HT + t][r] = x[HT + t][r] / sig - tp[t][r];
                lsum[(r >> 2) & 1] += lsig;
            }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            obj[st] = obj[st] - l16_group_sum(lsum[st]);
            obj[st] = obj[st] - cb[32 * C::NP + 1];   // logdet - log|det W|       (model.py:196)
            obj[st] = obj[st] - cb[32 * C::NP + 0];   // logdet - sum(3 logs)      (model.py:273-276, reverse)
        }
        // ---- I1: z = Winv'^T [z1; z2] + cinv ----
        {
            Split3 us[2 * NZT];
            l16_split_tiles<NZT>(x, us);
            f32x16 xn[NZT];
            l16_gemm_stage3<NZT, NZT, first_kib(C::P2, C::KT2)>(
                pipe, gi, gnext, xn, us, [&](int t) { return l16_bias_init(ci + 32 * t, g); }, keep);
#pragma unroll
            for (int t = 0; t < NZT; ++t) x[t] = xn[t];
        }
    }
#if LSNF_L16_PARTS == 2
    // this wave met an operand beyond fp16's range: element [first row][0] of its output (register 0 of tile 0 on lane 0)
    // carries the flag for the bf16x3 fix-up pass queued behind this kernel
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0) x[0][0] = __builtin_bit_cast(float, LSNF_F16_SENTINEL_BITS);
#endif
#pragma unroll
    for (int t = 0; t < NZT; ++t) l16_store_tile<HT>(t, x[t], a.z_out, sample, live, a.nz, a.half, g, vec4);
    if (a.objective_out) {
#pragma unroll
        for (int st = 0; st < 2; ++st)
            if (live[st] && g == 0) a.objective_out[sample[st]] = obj[st];
    }
    if constexpr (SAMPLE) {
        if (a.s.ll_out) {
#pragma unroll
            for (int st = 0; st < 2; ++st)
                if (live[st] && g == 0) a.s.ll_out[sample[st]] = llp[st] - obj[st];
        }
    }
}

template <class C>
size_t rev3_lds(int depth) { return ((size_t)depth * C::CONST_PER_BLOCK + 2 * (size_t)C::SLOT3) * sizeof(float); }

template <class C, int NW, bool SAMPLE, class Args>
hipError_t launch_rev3_w(const Args& a, hipStream_t stream) {
    return lsnf_launch_kernel<lsnf_rev3_kernel<C, NW, SAMPLE>>(lsnf_grid(a.B, 32 * NW), 64 * NW, rev3_lds<C>(a.depth), stream, a);
}
template <class C, bool SAMPLE, class Args>
hipError_t launch_rev3(const Args& a, hipStream_t stream) {
    // (the sampling form of the f_width > 64 geometry stays on 4 waves: at 8 waves -- 256 registers per lane -- the words it carries
    //  for ll_out would go to scratch; what a wave computes does not depend on NW)
    if constexpr (SAMPLE && C::WT == 4) {
        return launch_rev3_w<C, 4, SAMPLE>(a, stream);
    } else {
        return lsnf_eight_waves(a.B) ? launch_rev3_w<C, 8, SAMPLE>(a, stream) : launch_rev3_w<C, 4, SAMPLE>(a, stream);
    }
}
}  // namespace

#ifndef LSNF_REV3_ENTRY
#define LSNF_REV3_ENTRY lsnf_launch_reverse3
#define LSNF_REV3_COVERS lsnf_reverse3_covers
#endif
// Does LSNF_REV3_ENTRY take this geometry (host only, no HIP calls; lsnf_api.hip selects by it)?  The constants of the whole
// stack and a panel pair fit in 160 KiB of LDS.
bool LSNF_REV3_COVERS(const LsnfReverseCall& c) {
    return lsnf_with_cfg<Rev3Cfg>(c.g, [&](auto cfg) { return rev3_lds<decltype(cfg)>(c.g.depth) <= 160 * 1024; });
}

hipError_t LSNF_REV3_ENTRY(const LsnfReverseCall& c, int fixup) {
    if (!LSNF_REV3_COVERS(c)) return hipErrorInvalidValue;      // (a selection bug)
    Rev3SampleArgs a;
    lsnf_fill_reverse(a, c);
    a.guard = lsnf_guard_words(c); a.fixup = fixup;
#if LSNF_L16_PARTS == 3
    a.panels3b = c.plan + c.g.off_f3b_panels; a.ipanels3b = c.plan + c.g.off_i3b_panels;
#else
    a.panels3b = c.plan + c.g.off_f2h_panels; a.ipanels3b = c.plan + c.g.off_i2h_panels;
#endif
    return lsnf_with_sample<Rev3Args>(a, c.smp, [&](auto sample, const auto& args) {
        return lsnf_with_cfg<Rev3Cfg>(c.g, [&](auto cfg) { return launch_rev3<decltype(cfg), decltype(sample)::value>(args, c.stream); });
    });
}

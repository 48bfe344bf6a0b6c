// lsnf_small_rev.hip -- latency-oriented reverse (sampling) pass for small / medium batches.
// Same math and ABI entry point (lsnf_reverse dispatches on B) as lsnf_rev.hip, which replaces reference
// model.py:484-498 / :424-456; work decomposition of lsnf_small.h.
// Per block, last to first (x = [z1|z2] in LDS tiles X):
//   R2,R3,R4 : h = f(z1) -> [t; p]                                (forward panels S2..S4)
//   CI       : z2 = z2 / sigmoid(p) - t ; objective -= sum log sigmoid(p)     (model.py:436-438)
//   I1       : z = ([z1,z2] @ W^-1) * exp(-3 logs) - b ; objective -= log|det W| + sum 3 logs  (:193-196, 270, 246)
#include "lsnf_small.h"
#include "lsnf_launch.h"

namespace {

template <int HT_, int WT_>
struct SmallRevCfg : LsnfStackCfg<HT_, WT_> {
    using S = LsnfStackCfg<HT_, WT_>;
    using S::HT; using S::WT; using S::NZT;
    static constexpr int CONST_PER_BLOCK = S::FWD_CONST + S::INV_CONST;
    using R2 = SmallStage<WT, HT>;
    using R3 = SmallStage<WT, WT>;
    using R4 = SmallStage<2 * HT, WT>;
    using I1 = SmallStage<NZT, NZT, 1>;                        // unsplit: writes final tiles
    static constexpr int T_X = 0;                              // 2 x NZT ping-pong
    static constexpr int T_H1 = T_X + 2 * NZT;
    static constexpr int T_H2 = T_H1 + R2::OUT_TILES;
    static constexpr int T_TP = T_H2 + R3::OUT_TILES;
    static constexpr int T_U = T_TP + R4::OUT_TILES;           // NZT: [z1 | z2 after the inverse coupling] (final)
    static constexpr int T_END = T_U + NZT;
    static constexpr int AUX_FLOATS = 64 * (HT + 1);
};

struct SmallRevArgs {
    const float* fwd_consts; const float* fwd_panels; const float* inv_consts; const float* inv_panels;
    const float* z_in; const float* objective; float* z_out; float* objective_out;
    int B, nz, half, depth, vec4;
};

struct SmallRevSampleArgs : SmallRevArgs { LsnfSampleArgs s; };      // lsnf_sample: z_in / objective are unused (NULL)

// SAMPLE: the rows are drawn where they would be loaded (lsnf_sample); every other instruction is lsnf_reverse's.
template <class C, bool SAMPLE>
__global__ __launch_bounds__(LSNF_WG_THREADS, 1) void lsnf_small_rev_kernel(const std::conditional_t<SAMPLE, SmallRevSampleArgs, SmallRevArgs> a) {
    constexpr int HT = C::HT, NZT = C::NZT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tiles = smem;
    float* aux = smem + (size_t)C::T_END * LSNF_TILE_FLOATS;
    float* cst = aux + C::AUX_FLOATS;                                // depth * CONST_PER_BLOCK
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, m = lane & 31, h = lane >> 5;
    const int vec4 = a.vec4;
    auto T = [&](int t) { return tiles + (size_t)t * LSNF_TILE_FLOATS; };

    const int last = a.depth - 1;
    // weights two stages ahead, issued between the running stage's MFMA groups (lsnf_small.h, SmallFetch)
    auto f2 = C::R2::fetch(a.fwd_panels + (size_t)last * C::FWD_BLOCK + C::OFF_S2, wave, lane);
    auto f3 = C::R3::fetch(a.fwd_panels + (size_t)last * C::FWD_BLOCK + C::OFF_S3, wave, lane);
    for (int i = tid; i < a.depth * C::CONST_PER_BLOCK; i += LSNF_WG_THREADS) {
        const int blk = i / C::CONST_PER_BLOCK, r = i % C::CONST_PER_BLOCK;
        cst[i] = r < C::FWD_CONST ? a.fwd_consts[blk * C::FWD_CONST + r] : a.inv_consts[blk * C::INV_CONST + (r - C::FWD_CONST)];
    }
    const long sample = (long)blockIdx.x * LSNF_SMALL_SAMPLES + m;
    const bool live = sample < a.B;
    const long row = live ? sample : (long)a.B - 1;
    if constexpr (SAMPLE) {
        if (wave < NZT) {                                            // wave w draws tile w of the row, as it would load it
            const LsnfRngState rs = lsnf_rng_state(a.s.rng);
            float ss = 0.0f;
            const f32x16 e = lsnf_sample_tile<HT>(wave, (unsigned long long)(a.s.rng.row0 + sample), a.half, h, rs, a.s.temperature, ss);
            small_store_tile(T(C::T_X + (last & 1) * NZT + wave), e, lane);
            if (a.s.eps_out && live) lsnf_store_tile<HT>(wave, e, a.s.eps_out + sample * (long)a.nz, a.half, h, vec4);
            ss = lsnf_pair_sum(ss);
            if (h == 0) aux[32 * wave + m] = ss;                     // (aux is free until the first inverse coupling: 3 barriers on)
        }
    } else {
        if (wave < NZT) small_store_tile(T(C::T_X + (last & 1) * NZT + wave),
                                         lsnf_load_tile<HT>(wave, a.z_in + row * (long)a.nz, a.half, h, vec4), lane);
    }
    float obj = 0.0f;                                                // carried by wave 0
    if (wave == 0) obj = a.objective ? a.objective[row] : 0.0f;
    __syncthreads();
    float llp = 0.0f;                                                // SAMPLE: -0.5 * sum eps^2 + log(2 pi), carried by wave 0
    if constexpr (SAMPLE) {
        if (wave == 0) {
            float ss = 0.0f;
#pragma unroll
            for (int w = 0; w < NZT; ++w) ss += aux[32 * w + m];
            llp = -0.5f * ss + LSNF_LOG_2PI;
        }
    }

    for (int blk = last; blk >= 0; --blk) {
        const float* cb = cst + blk * C::CONST_PER_BLOCK;
        const float* ci = cb + C::FWD_CONST;
        const float* gf = a.fwd_panels + (size_t)blk * C::FWD_BLOCK;
        const float* gi = a.inv_panels + (size_t)blk * C::INV_BLOCK;
        float* X = T(C::T_X + (blk & 1) * NZT);
        float* Xn = T(C::T_X + ((blk + 1) & 1) * NZT);
        float* H1 = T(C::T_H1); float* H2 = T(C::T_H2); float* TP = T(C::T_TP); float* U = T(C::T_U);
        auto tile = [&](const float* base, int t) { return small_load_tile(base + (size_t)t * LSNF_TILE_FLOATS, lane); };

        auto p4 = C::R4::begin_fetch(gf + C::OFF_S4, wave, lane);
        C::R2::run(f2, H1, wave, lane, [&](int kt) { return tile(X, kt); },
                   [&](int nt) { return lsnf_bias_init(cb + 32 * (C::P1 + nt), h); }, p4);
        __syncthreads();
        auto pi = C::I1::begin_fetch(gi, wave, lane);
        C::R3::run(f3, H2, wave, lane,
                   [&](int kt) { return small_gather_tile<C::R2::KS, true>(H1 + (size_t)kt * C::R2::KS * LSNF_TILE_FLOATS, lane); },
                   [&](int nt) { return lsnf_bias_init(cb + 32 * (C::P1 + C::P2 + nt), h); }, pi);
        __syncthreads();
        const float* gfn = a.fwd_panels + (size_t)(blk > 0 ? blk - 1 : 0) * C::FWD_BLOCK;   // block 0 re-fetches its own panels
        auto p2 = C::R2::begin_fetch(gfn + C::OFF_S2, wave, lane);
        C::R4::run(p4.f, TP, wave, lane,
                   [&](int kt) { return small_gather_tile<C::R3::KS, true>(H2 + (size_t)kt * C::R3::KS * LSNF_TILE_FLOATS, lane); },
                   [&](int nt) { return lsnf_bias_init(cb + 32 * (C::P1 + C::P2 + C::P3 + nt), h); }, p2);
        f2 = p2.f;
        __syncthreads();
        // inverse coupling on waves 0..HT-1; waves HT..2HT-1 forward z1
        if (wave < HT) {
            const int j = wave;
            const f32x16 t = small_gather_tile<C::R4::KS, false>(TP + (size_t)j * C::R4::KS * LSNF_TILE_FLOATS, lane);
            const f32x16 p = small_gather_tile<C::R4::KS, false>(TP + (size_t)(HT + j) * C::R4::KS * LSNF_TILE_FLOATS, lane);
            f32x16 z2 = tile(X, HT + j);
            float lsum = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float sig, lsig;
                lsnf_sigmoid_logsig(p[r], sig, lsig);
                z2[r] = z2[r] / sig - t[r];
                lsum += lsig;
            }
            small_store_tile(U + (size_t)(HT + j) * LSNF_TILE_FLOATS, z2, lane);
            aux[64 * j + lane] = lsum;
        } else if (wave < 2 * HT) {
            const int j = wave - HT;
            small_store_tile(U + (size_t)j * LSNF_TILE_FLOATS, tile(X, j), lane);
        }
        __syncthreads();
        if (wave == 0) {
            float ls = 0.0f;
#pragma unroll
            for (int j = 0; j < HT; ++j) ls += aux[64 * j + lane];
            obj = obj - lsnf_pair_sum(ls);
            obj = obj - cb[32 * C::NP + 1];   // logdet - log|det W|       (model.py:196)
            obj = obj - cb[32 * C::NP + 0];   // logdet - sum(3 logs)      (model.py:273-276, reverse)
        }
        auto p3 = C::R3::begin_fetch(gfn + C::OFF_S3, wave, lane);
        C::I1::run(pi.f, Xn, wave, lane, [&](int kt) { return tile(U, kt); }, [&](int nt) { return lsnf_bias_init(ci + 32 * nt, h); }, p3);
        f3 = p3.f;
        __syncthreads();
    }
    float* Xf = T(C::T_X + (1 & 1) * NZT);      // block 0 wrote X[(0+1)&1]
    if (wave < NZT && live)
        lsnf_store_tile<HT>(wave, small_load_tile(Xf + (size_t)wave * LSNF_TILE_FLOATS, lane), a.z_out + sample * (long)a.nz,
                            a.half, h, vec4);
    if (wave == 0 && live && h == 0 && a.objective_out) a.objective_out[sample] = obj;
    if constexpr (SAMPLE) {
        if (wave == 0 && live && h == 0 && a.s.ll_out) a.s.ll_out[sample] = llp - obj;
    }
}

template <class C>
size_t small_rev_lds(int depth) { return ((size_t)C::T_END * LSNF_TILE_FLOATS + C::AUX_FLOATS + (size_t)depth * C::CONST_PER_BLOCK) * sizeof(float); }

template <class C, bool SAMPLE, class Args>
hipError_t launch_small_rev(const Args& a, hipStream_t stream) {
    return lsnf_launch_kernel<lsnf_small_rev_kernel<C, SAMPLE>>(lsnf_grid(a.B, LSNF_SMALL_SAMPLES), LSNF_WG_THREADS, small_rev_lds<C>(a.depth), stream, a);
}
}  // namespace

// Does the kernel take this geometry (host only, no HIP calls; lsnf_api.hip selects by it)?  The constants of the whole stack
// fit in 160 KiB of LDS.
bool lsnf_small_reverse_covers(const LsnfReverseCall& c) {
    return lsnf_with_cfg<SmallRevCfg>(c.g, [&](auto cfg) { return small_rev_lds<decltype(cfg)>(c.g.depth) <= 160 * 1024; });
}

hipError_t lsnf_launch_small_reverse(const LsnfReverseCall& c) {
    if (!lsnf_small_reverse_covers(c)) return hipErrorInvalidValue;      // (a selection bug)
    SmallRevSampleArgs a;
    lsnf_fill_reverse(a, c);
    a.fwd_panels = c.plan + c.g.off_fwd_panels; a.inv_panels = c.plan + c.g.off_inv_panels;
    return lsnf_with_sample<SmallRevArgs>(a, c.smp, [&](auto sample, const auto& args) {
        return lsnf_with_cfg<SmallRevCfg>(c.g, [&](auto cfg) { return launch_small_rev<decltype(cfg), decltype(sample)::value>(args, c.stream); });
    });
}

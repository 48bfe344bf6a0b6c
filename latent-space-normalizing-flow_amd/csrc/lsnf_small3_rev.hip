// lsnf_small3_rev.hip -- latency reverse (sampling) pass on the bf16 matrix pipe: the L16 / bf16x3 scheme of
// lsnf_small3_fwd.hip (workgroups of ST sample tiles of 16 rows, producer-side split, weights re-loaded in place one block ahead:
// lsnf_small3.h units_mma_st) for reference model.py:484-498 / :424-456.
// Per block, last to first; wave w owns the half-units z1[w], z2[w] of the running latent (registers):
//   R2,R3,R4 : h = f(z1) -> t[w], p[w]                              (forward panels S2..S4, 16x16x32 operand order)
//   CI       : z2 = z2 / sigmoid(p) - t ; objective -= sum log sigmoid(p)     (model.py:436-438), in registers: R4's epilogue
//   I1       : z = ([z1,z2] @ W^-1) * exp(-3 logs) - b ; objective -= log|det W| + sum 3 logs  (:193-196, 270, 246);
//              its epilogue publishes the new z1 (the next block's R2 operand) into the OTHER z1 buffer: four barriers per block
// KEEP (lsnf_reverse_keep / lsnf_sample_keep): the pass also leaves what the backward of the reverse (lsnf_small3_rbwd.hip) and the
// parameter gradients read of the FORWARD at x -- the coupling MLP's input is the first half of the block's OUTPUT (model.py:422), so
// the [z1; z2] at the top of reverse block b is forward block b's output, R2 / R3's h are h1 / h2 and R4's sigmoid is the stash's.
#include <stdlib.h>
#include "lsnf_small3.h"
#include "lsnf_launch.h"

namespace {

template <int HT_, int WT_>
struct Small3RevCfg : LsnfStackCfg<HT_, WT_> {
    using S = LsnfStackCfg<HT_, WT_>;
    static constexpr int F = LSNF_FRAG3_FLOATS;
    static constexpr int OFF3_S2 = F * S::P1 * S::KT1;
    static constexpr int OFF3_S3 = OFF3_S2 + F * S::P2 * S::KT2;
    static constexpr int OFF3_S4 = OFF3_S3 + F * S::P3 * S::KT3;
    static constexpr int BLOCK3 = OFF3_S4 + F * S::P4 * S::KT4;
    static constexpr int BLOCKI = F * S::NZT * S::NZT;
    static constexpr int CONST_PER_BLOCK = S::FWD_CONST + S::INV_CONST;
    static constexpr int NU2 = (2 * WT_ + 3) / 4;
};
// LDS map (floats) for ST sample tiles: z1 tiles (HT per sample tile, double-buffered: I1 publishes the next block's z1 while it
// reads this block's), z2 tiles after the inverse coupling (HT), H1, H2 (WT each), reductions, constants
template <class C, int ST>
struct Small3RevLds {
    static constexpr int GH = C::HT * S3_BTILE_FLOATS, HL = C::WT * S3_BTILE_FLOATS;
    static constexpr int L_Z1 = 0;
    static constexpr int L_Z2 = L_Z1 + 2 * ST * GH;
    static constexpr int L_H1 = L_Z2 + ST * GH;
    static constexpr int L_H2 = L_H1 + ST * HL;
    static constexpr int L_RED = L_H2 + ST * HL;
    static constexpr int L_CONST = L_RED + ST * 4 * 16;
};

struct Small3RevArgs {
    const float* fwd_consts; const float* inv_consts; const float* panels3b; const float* ipanels3b;
    const float* z_in; const float* objective; float* z_out; float* objective_out;
    int B, nz, half, depth, vec4;
};

struct Small3RevSampleArgs : Small3RevArgs { LsnfSampleArgs s; };      // lsnf_sample: z_in / objective are unused (NULL)
// KEEP: each pointer NULL or the tensor lsnf_forward documents (z_saved; act_saved: LsnfActLayout, absolute block; hdump: LsnfDumpLayout
// of block 0, h1 / h2 row-major)
struct Small3RevKeep { float* z_saved; float* act_saved; float* hdump; int width; };
struct Small3RevKeepArgs : Small3RevArgs { Small3RevKeep k; };
struct Small3RevSampleKeepArgs : Small3RevSampleArgs { Small3RevKeep k; };
template <bool SAMPLE, bool KEEP>
using small3_rev_args_t = std::conditional_t<KEEP, std::conditional_t<SAMPLE, Small3RevSampleKeepArgs, Small3RevKeepArgs>,
                                             std::conditional_t<SAMPLE, Small3RevSampleArgs, Small3RevArgs>>;

// SAMPLE: the rows are drawn where they would be loaded (lsnf_sample): each wave draws the two half-units it owns, behind its
// weight fetches; every other instruction is lsnf_reverse's.  -0.5 * sum eps^2 takes the objective's way through RED, in the
// prologue (RED is free until the final reduction), into a second accumulator that wave 0 carries.
// KEEP: stores only, each under its own pointer, in the stage epilogues (under the next sample tile's MFMAs): the ReLU masks and h1 /
// h2 rows from R2 / R3, sigma from R4, the block outputs from I1 -- what lsnf_small3_fwd.hip's EXTRAS form keeps, same layouts.
template <class C, int ST, bool SAMPLE, bool KEEP = false>
__global__ __launch_bounds__(256, 1) void lsnf_small3_rev_kernel(const small3_rev_args_t<SAMPLE, KEEP> a) {
    constexpr int HT = C::HT, WT = C::WT, NZT = C::NZT, NU2 = C::NU2, LASTU = NU2 - 1;
    using L = Small3RevLds<C, ST>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Z1 = smem + L::L_Z1;
    float* Z2 = smem + L::L_Z2;
    float* H1B = smem + L::L_H1;
    float* H2B = smem + L::L_H2;
    float* RED = smem + L::L_RED;
    float* cst = smem + L::L_CONST;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int vec4 = a.vec4;

    // (a wave without a unit of its own computes unit 0 again and stores the same values to the same LDS words: no branch in the stages)
    const bool has1 = wave < 2 * HT;
    const int hu1 = has1 ? wave : 0, nt1 = hu1 >> 1, ft1 = hu1 & 1;
    int hw[NU2]; bool hasw[NU2];
#pragma unroll
    for (int i = 0; i < NU2; ++i) { hasw[i] = wave + 4 * i < 2 * WT; hw[i] = hasw[i] ? wave + 4 * i : 0; }

    const int last = a.depth - 1;
    const float* gf_last = a.panels3b + (size_t)last * C::BLOCK3;
    const float* gi_last = a.ipanels3b + (size_t)last * C::BLOCKI;
    long sample[ST]; bool live[ST]; long row[ST];
    f32x4 z1[ST], z2[ST];
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        sample[st] = ((long)blockIdx.x * ST + st) * S3_SAMPLES + n;
        live[st] = sample[st] < a.B;
        row[st] = live[st] ? sample[st] : (long)a.B - 1;
        if constexpr (!SAMPLE) {
            // this wave's half-units of the input (requested before the weights and the constants: vmcnt completes in order)
            z1[st] = load_row_half<HT>(nt1, ft1, a.z_in + row[st] * (long)a.nz, a.half, g, vec4);
            z2[st] = load_row_half<HT>(HT + nt1, ft1, a.z_in + row[st] * (long)a.nz, a.half, g, vec4);
        }
    }
    float obj[ST];                                                        // per-wave partial of the running objective
#pragma unroll
    for (int st = 0; st < ST; ++st) obj[st] = (wave == 0 && a.objective) ? a.objective[row[st]] : 0.0f;
    __builtin_amdgcn_sched_barrier(0);
    UFrags<HT> w2[NU2];
    UFrags<WT> w3[NU2];
#pragma unroll
    for (int i = 0; i < NU2; ++i) w2[i] = fetch_unit<HT>(gf_last + C::OFF3_S2, hw[i] >> 1, hw[i] & 1, lane);
#pragma unroll
    for (int i = 0; i < NU2; ++i) w3[i] = fetch_unit<WT>(gf_last + C::OFF3_S3, hw[i] >> 1, hw[i] & 1, lane);
    UFrags<WT> w4t = fetch_unit<WT>(gf_last + C::OFF3_S4, nt1, ft1, lane);
    UFrags<WT> w4p = fetch_unit<WT>(gf_last + C::OFF3_S4, HT + nt1, ft1, lane);
    UFrags<NZT> wia = fetch_unit<NZT>(gi_last, nt1, ft1, lane);
    UFrags<NZT> wib = fetch_unit<NZT>(gi_last, HT + nt1, ft1, lane);
    __builtin_amdgcn_sched_barrier(0);
    for (int i = tid; i < a.depth * C::CONST_PER_BLOCK; i += 256) {
        const int blk = i / C::CONST_PER_BLOCK, r = i % C::CONST_PER_BLOCK;
        cst[i] = r < C::FWD_CONST ? a.fwd_consts[blk * C::FWD_CONST + r] : a.inv_consts[blk * C::INV_CONST + (r - C::FWD_CONST)];
    }
    if constexpr (SAMPLE) {
        const LsnfRngState rs = lsnf_rng_state(a.s.rng);
        const int f0 = 32 * nt1 + 16 * ft1 + 4 * g;
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            const unsigned long long grow = (unsigned long long)(a.s.rng.row0 + sample[st]);
            float ss = 0.0f;
            z1[st] = lsnf_sample4(0, f0, a.half, grow, rs, a.s.temperature, ss);
            z2[st] = lsnf_sample4(1, f0, a.half, grow, rs, a.s.temperature, ss);
            if (a.s.eps_out && has1 && live[st]) {
                float* er = a.s.eps_out + sample[st] * (long)a.nz;
                store_row_half<HT>(nt1, ft1, z1[st], er, a.half, g, vec4);
                store_row_half<HT>(HT + nt1, ft1, z2[st], er, a.half, g, vec4);
            }
            if (a.s.ll_out) {                  // kernel-uniform
                ss = has1 ? group_sum(ss) : 0.0f;
                if (g == 0) RED[(st * 4 + wave) * 16 + n] = ss;
            }
        }
    }
#pragma unroll
    for (int st = 0; st < ST; ++st) store_half(Z1 + st * L::GH + nt1 * S3_BTILE_FLOATS, ft1, z1[st], lane);   // buffer 0
    float lsum[ST];                                                       // running sum of log sigmoid(p) over all blocks
#pragma unroll
    for (int st = 0; st < ST; ++st) lsum[st] = 0.0f;
    __syncthreads();
    // KEEP: stash addressing (lsnf_small3.h) and the layouts of the stash and of the parameter-gradient dump
    size_t wtile[ST]; int lane32[ST]; bool tile_ok[ST];
    LsnfActLayout al = {}; LsnfDumpLayout dl = {}; bool w4 = false;
    if constexpr (KEEP) {
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            const StashTile t = stash_tile((size_t)blockIdx.x * ST + st, a.B, n, g);
            wtile[st] = t.wtile; tile_ok[st] = t.ok; lane32[st] = t.lane32;
        }
        al = lsnf_act_layout(a.B, HT, WT);
        dl = lsnf_dump_layout(a.B, a.nz, a.k.width);
        w4 = (a.k.width & 3) == 0;
    }
    float llp[ST];                                                        // SAMPLE: -0.5 * sum eps^2 + log(2 pi), carried by wave 0
#pragma unroll
    for (int st = 0; st < ST; ++st) llp[st] = 0.0f;
    if constexpr (SAMPLE) {
        if (a.s.ll_out && wave == 0) {
#pragma unroll
            for (int st = 0; st < ST; ++st)
                llp[st] = -0.5f * (RED[(st * 4 + 0) * 16 + n] + RED[(st * 4 + 1) * 16 + n] + RED[(st * 4 + 2) * 16 + n] + RED[(st * 4 + 3) * 16 + n]) + LSNF_LOG_2PI;
        }
    }

    for (int blk = last; blk >= 0; --blk) {
        const float* cb = cst + blk * C::CONST_PER_BLOCK;
        const float* ci = cb + C::FWD_CONST;
        const float* gi = a.ipanels3b + (size_t)blk * C::BLOCKI;
        const int nb = blk > 0 ? blk - 1 : 0;                              // block 0 re-fetches its own panels: no loads under a branch
        const float* gfn = a.panels3b + (size_t)nb * C::BLOCK3;
        const float* gin = a.ipanels3b + (size_t)nb * C::BLOCKI;
        float* z1_cur = Z1 + ((last - blk) & 1) * ST * L::GH;
        float* z1_nxt = Z1 + ((last - blk + 1) & 1) * ST * L::GH;
        float* act[ST]; float* hd[ST];                                     // KEEP: this block's stash tile / h1, h2 row of each sample tile
        if constexpr (KEEP) {
#pragma unroll
            for (int st = 0; st < ST; ++st) {
                act[st] = (a.k.act_saved && tile_ok[st]) ? a.k.act_saved + (size_t)blk * al.per_block + wtile[st] * al.per_tile : nullptr;
                hd[st] = (a.k.hdump && live[st]) ? a.k.hdump + (size_t)blk * dl.per_block + sample[st] * (long)a.k.width : nullptr;
            }
        }

        // ---- R2: h1 = relu(W1'^T z1 + c1) ----
#pragma unroll
        for (int i = 0; i < NU2; ++i) {
            const int nt = hw[i] >> 1, ft = hw[i] & 1;
            f32x4 h[ST];
            const f32x4 bh = unit_bias(cb + 32 * (C::P1 + nt), ft, g);
#pragma unroll
            for (int st = 0; st < ST; ++st) h[st] = bh;
            auto epi = [&](int st) {
                h[st] = relu4(h[st]);
                store_half(H1B + st * L::HL + nt * S3_BTILE_FLOATS, ft, h[st], lane);
                if constexpr (KEEP) {
                    if (hasw[i]) {
                        if (hd[st]) store_plain_half(h[st], hd[st] + dl.off_h1, a.k.width, nt, ft, g, w4);
                        if (act[st]) stash_relu_mask(act[st], al.mask_off, nt, lane32[st], ft, h[st], lane);
                    }
                }
            };
            const bf16x8* rf = unit_ptr<HT>(gfn + C::OFF3_S2, nt, ft, lane);
            if (i == 0) {        // carry: the last k-tile of I1's two units, THIS block's fragments (I1 runs last in the block)
                const bf16x8* ca = unit_ptr<NZT>(gi, nt1, ft1, lane);
                const bf16x8* cbp = unit_ptr<NZT>(gi, HT + nt1, ft1, lane);
                units_mma_st<HT, 0, HT, ST, 1, 28, 6, 0>(h, h, w2[i], w2[i], rf, nullptr, z1_cur, L::GH, lane, epi,
                    [&](int q) { if (q < 3) refill_last<NZT>(wia, ca, q); else refill_last<NZT>(wib, cbp, q - 3); }, [](int) {});
            } else {
                const bf16x8* cp = unit_ptr<HT>(gfn + C::OFF3_S2, hw[i > 0 ? i - 1 : 0] >> 1, hw[i > 0 ? i - 1 : 0] & 1, lane);
                units_mma_st<HT, 0, HT, ST, 1, 28, 3, 0>(h, h, w2[i], w2[i], rf, nullptr, z1_cur, L::GH, lane, epi,
                    [&](int q) { refill_last<HT>(w2[i > 0 ? i - 1 : 0], cp, q); }, [](int) {});
            }
        }
        __syncthreads();
        // ---- R3: h2 ----
#pragma unroll
        for (int i = 0; i < NU2; ++i) {
            const int nt = hw[i] >> 1, ft = hw[i] & 1;
            f32x4 h[ST];
            const f32x4 bh = unit_bias(cb + 32 * (C::P1 + C::P2 + nt), ft, g);
#pragma unroll
            for (int st = 0; st < ST; ++st) h[st] = bh;
            auto epi = [&](int st) {
                h[st] = relu4(h[st]);
                store_half(H2B + st * L::HL + nt * S3_BTILE_FLOATS, ft, h[st], lane);
                if constexpr (KEEP) {
                    if (hasw[i]) {
                        if (hd[st]) store_plain_half(h[st], hd[st] + dl.off_h2, a.k.width, nt, ft, g, w4);
                        if (act[st]) stash_relu_mask(act[st], al.mask_off, WT + nt, lane32[st], ft, h[st], lane);
                    }
                }
            };
            const bf16x8* rf = unit_ptr<WT>(gfn + C::OFF3_S3, nt, ft, lane);
            if (i == 0) {
                const bf16x8* cp = unit_ptr<HT>(gfn + C::OFF3_S2, hw[LASTU] >> 1, hw[LASTU] & 1, lane);
                units_mma_st<WT, 0, WT, ST, 1, 28, 3, 0>(h, h, w3[i], w3[i], rf, nullptr, H1B, L::HL, lane, epi,
                    [&](int q) { refill_last<HT>(w2[LASTU], cp, q); }, [](int) {});
            } else {
                const bf16x8* cp = unit_ptr<WT>(gfn + C::OFF3_S3, hw[i > 0 ? i - 1 : 0] >> 1, hw[i > 0 ? i - 1 : 0] & 1, lane);
                units_mma_st<WT, 0, WT, ST, 1, 28, 3, 0>(h, h, w3[i], w3[i], rf, nullptr, H1B, L::HL, lane, epi,
                    [&](int q) { refill_last<WT>(w3[i > 0 ? i - 1 : 0], cp, q); }, [](int) {});
            }
        }
        __syncthreads();
        // ---- R4 + inverse coupling (its epilogue): z2 = z2 / sigmoid(p) - t ----
        {
            f32x4 tt_[ST], pp[ST];
            const f32x4 bt = unit_bias(cb + 32 * (C::P1 + C::P2 + C::P3 + nt1), ft1, g);
            const f32x4 bp = unit_bias(cb + 32 * (C::P1 + C::P2 + C::P3 + HT + nt1), ft1, g);
#pragma unroll
            for (int st = 0; st < ST; ++st) { tt_[st] = bt; pp[st] = bp; }
            const bf16x8* c3 = unit_ptr<WT>(gfn + C::OFF3_S3, hw[LASTU] >> 1, hw[LASTU] & 1, lane);
            units_mma_st<WT, 0, WT, ST, 2, 60, 3, 0>(tt_, pp, w4t, w4p, unit_ptr<WT>(gfn + C::OFF3_S4, nt1, ft1, lane),
                unit_ptr<WT>(gfn + C::OFF3_S4, HT + nt1, ft1, lane), H2B, L::HL, lane,
                [&](int st) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float sig, lsig;
                        lsnf_sigmoid_logsig(pp[st][r], sig, lsig);
                        z2[st][r] = z2[st][r] / sig - tt_[st][r];
                        lsum[st] += lsig;
                        if constexpr (KEEP) pp[st][r] = sig;              // (kept for the stash)
                    }
                    store_half(Z2 + st * L::GH + nt1 * S3_BTILE_FLOATS, ft1, z2[st], lane);
                    if constexpr (KEEP) {
                        if (has1 && act[st]) stash_sigma(act[st], nt1, ft1, g, lane32[st], pp[st]);
                    }
                },
                [&](int q) { refill_last<WT>(w3[LASTU], c3, q); }, [](int) {});
        }
        if (wave == 0) {
#pragma unroll
            for (int st = 0; st < ST; ++st) {
                obj[st] = obj[st] - cb[32 * C::NP + 1];   // logdet - log|det W|       (model.py:196)
                obj[st] = obj[st] - cb[32 * C::NP + 0];   // logdet - sum(3 logs)      (model.py:273-276, reverse)
            }
        }
        __syncthreads();
        // ---- I1: z = Winv'^T [z1; z2] + cinv; the new z1 goes to the other z1 buffer under the last steps ----
        {
            const f32x4 b1 = unit_bias(ci + 32 * nt1, ft1, g), b2 = unit_bias(ci + 32 * (HT + nt1), ft1, g);
#pragma unroll
            for (int st = 0; st < ST; ++st) { z1[st] = b1; z2[st] = b2; }
            const bf16x8* c4t = unit_ptr<WT>(gfn + C::OFF3_S4, nt1, ft1, lane);
            const bf16x8* c4p = unit_ptr<WT>(gfn + C::OFF3_S4, HT + nt1, ft1, lane);
            units_mma_st<NZT, 0, NZT, ST, 2, 24, 6, 0, HT>(z1, z2, wia, wib, unit_ptr<NZT>(gin, nt1, ft1, lane), unit_ptr<NZT>(gin, HT + nt1, ft1, lane),
                z1_cur, L::GH, lane,
                [&](int st) {
                    store_half(z1_nxt + st * L::GH + nt1 * S3_BTILE_FLOATS, ft1, z1[st], lane);   // (after block 0: nobody reads it)
                    if constexpr (KEEP) {            // [z1; z2] is forward block blk-1's output: slice blk-1 of z_saved
                        if (a.k.z_saved && blk > 0 && has1 && live[st]) {
                            float* zr = a.k.z_saved + ((size_t)(blk - 1) * a.B + sample[st]) * a.nz;
                            store_row_half<HT>(nt1, ft1, z1[st], zr, a.half, g, vec4);
                            store_row_half<HT>(HT + nt1, ft1, z2[st], zr, a.half, g, vec4);
                        }
                    }
                },
                [&](int q) { if (q < 3) refill_last<WT>(w4t, c4t, q); else refill_last<WT>(w4p, c4p, q - 3); }, [](int) {}, Z2);
        }
        __syncthreads();
    }
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        if (has1 && live[st]) {
            float* zr = a.z_out + sample[st] * (long)a.nz;
            store_row_half<HT>(nt1, ft1, z1[st], zr, a.half, g, vec4);
            store_row_half<HT>(HT + nt1, ft1, z2[st], zr, a.half, g, vec4);
        }
    }
    bool want_obj = a.objective_out != nullptr;       // kernel-uniform
    if constexpr (SAMPLE) want_obj = want_obj || a.s.ll_out != nullptr;
    if (want_obj) {
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            const float o = obj[st] - (has1 ? group_sum(lsum[st]) : 0.0f);
            if (g == 0) RED[(st * 4 + wave) * 16 + n] = o;
        }
        __syncthreads();
        if (wave == 0 && g == 0) {
#pragma unroll
            for (int st = 0; st < ST; ++st)
                if (live[st]) {
                    const float o = RED[(st * 4 + 0) * 16 + n] + RED[(st * 4 + 1) * 16 + n] + RED[(st * 4 + 2) * 16 + n] + RED[(st * 4 + 3) * 16 + n];
                    if (a.objective_out) a.objective_out[sample[st]] = o;
                    if constexpr (SAMPLE) {
                        if (a.s.ll_out) a.s.ll_out[sample[st]] = llp[st] - o;
                    }
                }
        }
    }
}

template <class C, int ST>
size_t small3_rev_lds(int depth) { return ((size_t)Small3RevLds<C, ST>::L_CONST + (size_t)depth * C::CONST_PER_BLOCK) * sizeof(float); }
// (shapes that cannot fit for any depth are not instantiated)
template <class C, int ST>
constexpr bool small3_rev_built = (size_t)(Small3RevLds<C, ST>::L_CONST + C::CONST_PER_BLOCK) * sizeof(float) <= 160 * 1024 && !(ST == 4 && C::WT > 2);

template <class C, int ST, bool SAMPLE, bool KEEP, class Args>
hipError_t launch_small3_rev_st(const Args& a, hipStream_t stream) {
    if constexpr (!small3_rev_built<C, ST>) {
        return hipErrorInvalidValue;                 // (a selection bug)
    } else {
        return lsnf_launch_kernel<lsnf_small3_rev_kernel<C, ST, SAMPLE, KEEP>>(lsnf_grid(a.B, ST * S3_SAMPLES), 256, small3_rev_lds<C, ST>(a.depth), stream, a);
    }
}
// the instantiation of (geometry, st) in the form `args` is the argument type of
template <bool SAMPLE, bool KEEP, class Args>
hipError_t launch_small3_rev(const LsnfReverseCall& c, int st, const Args& args) {
    return lsnf_with_cfg<Small3RevCfg>(c.g, [&](auto cfg) {
        return lsnf_with_st(st, [&](auto s) { return launch_small3_rev_st<decltype(cfg), decltype(s)::value, SAMPLE, KEEP>(args, c.stream); });
    });
}
}  // namespace

// Rows per workgroup (16 x ST) for this call, 0 if the kernel does not take it (lsnf_api.hip selects by it): what
// lsnf_small3_st_wanted asks for; a shape whose constants of the whole stack do not fit in 160 KiB of LDS gives way to the next
// smaller one.
int lsnf_small3_reverse_st(const LsnfReverseCall& c) {
    return lsnf_with_cfg<Small3RevCfg>(c.g, [&](auto cfg) {
        using C = decltype(cfg);
        const int st = lsnf_small3_st_wanted(c.B), depth = c.g.depth;
        if (st >= 4 && small3_rev_built<C, 4> && small3_rev_lds<C, 4>(depth) <= 160 * 1024) return 4;
        if (st >= 2 && small3_rev_built<C, 2> && small3_rev_lds<C, 2>(depth) <= 160 * 1024) return 2;
        if (small3_rev_built<C, 1> && small3_rev_lds<C, 1>(depth) <= 160 * 1024) return 1;
        return 0;
    });
}

// st: lsnf_small3_reverse_st of the call.  A call that keeps something (z_saved / act_saved / hdump) runs the KEEP form.
hipError_t lsnf_launch_small3_reverse(const LsnfReverseCall& c, int st) {
    Small3RevSampleArgs a;
    lsnf_fill_reverse(a, c);
    a.panels3b = c.plan + c.g.off_f3b_panels; a.ipanels3b = c.plan + c.g.off_i3b_panels;
    if (c.z_saved || c.act_saved || c.hdump) {
        const Small3RevKeep k = {c.z_saved, c.act_saved, c.hdump, c.g.width};
        if (c.smp) {
            Small3RevSampleKeepArgs ak;
            static_cast<Small3RevArgs&>(ak) = a; ak.s = *c.smp; ak.k = k;
            return launch_small3_rev<true, true>(c, st, ak);
        }
        Small3RevKeepArgs ak;
        static_cast<Small3RevArgs&>(ak) = a; ak.k = k;
        return launch_small3_rev<false, true>(c, st, ak);
    }
    return lsnf_with_sample<Small3RevArgs>(a, c.smp, [&](auto sample, const auto& args) {
        return launch_small3_rev<decltype(sample)::value, false>(c, st, args);
    });
}

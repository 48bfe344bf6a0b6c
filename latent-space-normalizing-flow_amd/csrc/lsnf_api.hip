// lsnf_api.hip -- the C ABI of liblsnf_flow.so (declared in include/lsnf_flow.h).
// Argument validation happens here, on the host, BEFORE any kernel is launched: operand shapes
// and alignments are checked against what the kernels and their grids assume.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include <stdlib.h>
#ifndef LSNF_SMALL_MAX_DEFAULT
#define LSNF_SMALL_MAX_DEFAULT 16384
#endif

#include "../../include/lsnf_flow.h"
#include "../../include/lsnf_flow_mcmc.h"
#include "lsnf_launch.h"      // the call descriptors, the launchers and their coverage predicates

namespace {
thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    return fail(LSNF_E_HIP, "%s: %s", what, hipGetErrorString(e));
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
// vector width of the latent-row accesses: every (B, nz) tensor of the call must allow it (NULL pointers do)
int row_vector_width(const LsnfGeo& g, std::initializer_list<const void*> rows) {
    bool a16 = true, a8 = true;
    for (const void* p : rows) { a16 = a16 && aligned16(p); a8 = a8 && aligned8(p); }
    if (g.half % 4 == 0 && a16) return 4;
    if (g.half % 2 == 0 && a8) return 2;
    return 1;
}

// arithmetic of the GEMMs (LSNF_MATH=fp32|bf16x3|bf16x3_phased|fp16x2 overrides the default).  The two knobs are
// process-wide settings read by every call: atomics, so that a setter on one thread and a launch on another do not race
// (a launch sees the old or the new value, never a torn one).
std::atomic<int> g_math{-1};
int math_mode() {
    int m = g_math.load(std::memory_order_relaxed);
    if (m < 0) {
        const char* e = getenv("LSNF_MATH");
        m = (e && !strcmp(e, "bf16x3")) ? LSNF_MATH_BF16X3 : (e && !strcmp(e, "bf16x3_phased")) ? LSNF_MATH_BF16X3_PHASED
          : (e && !strcmp(e, "fp16x2")) ? LSNF_MATH_FP16X2 : (e && !strcmp(e, "fp32")) ? LSNF_MATH_FP32 : LSNF_MATH_DEFAULT;
        int expected = -1;
        g_math.compare_exchange_strong(expected, m, std::memory_order_relaxed);
        m = g_math.load(std::memory_order_relaxed);
    }
    return m;
}
// rows at or below which the small-batch (latency) kernels are used: LSNF_SMALL_BATCH_AUTO = the measured crossover of
// the arithmetic mode in force -- ONE threshold for the forward, the backward, the Langevin step and the reverse, so the
// kernel family that wrote an activation stash is the family that reads it (LSNF_SMALL_MAX overrides; 0 disables them)
std::atomic<int> g_small_max{-3};                 // -3: not initialised; LSNF_SMALL_BATCH_AUTO; or the rows set by the caller
int small_batch_setting() {
    int v = g_small_max.load(std::memory_order_relaxed);
    if (v == -3) {
        const char* e = getenv("LSNF_SMALL_MAX");
        int init = e ? atoi(e) : LSNF_SMALL_BATCH_AUTO;
        if (init < 0) init = LSNF_SMALL_BATCH_AUTO;
        int expected = -3;
        g_small_max.compare_exchange_strong(expected, init, std::memory_order_relaxed);
        v = g_small_max.load(std::memory_order_relaxed);
    }
    return v;
}
int small_batch_max() {
    const int v = small_batch_setting();
    if (v != LSNF_SMALL_BATCH_AUTO) return v;
    // fp16x2: its throughput forward is the faster one from ~12 K rows (profiles/r01_i_crossover.txt: 40.8 vs 41.9 us at
    // 12 288, 42.5 vs 51.6 at 16 384); every other mode: ~18-20 K (profiles/r01_g_crossover.txt)
    return math_mode() == LSNF_MATH_FP16X2 ? 12288 : LSNF_SMALL_MAX_DEFAULT;
}
// modes whose latency / backward / reverse kernels are the bf16x3 "L16" ones
bool l16_math() { const int m = math_mode(); return m == LSNF_MATH_BF16X3 || m == LSNF_MATH_FP16X2 || m == LSNF_MATH_BF16X3_PHASED; }

// ---- argument rules: each rule of the ABI is stated ONCE, in Check; an entry point is the list of the rules it applies, in the
// order it checks them, followed by its descriptor.  A rule returns true when it refuses the call: lsnf_last_error() then reads
// "<entry>: ..." and rc is the code to return.  The tensor names in a message are the entry point's own wording: a parameter.
typedef std::initializer_list<const void*> Ptrs;
bool all_aligned(Ptrs ps, uintptr_t mask) {      // (NULL is aligned: an optional tensor that is absent breaks no rule)
    for (const void* p : ps) if (reinterpret_cast<uintptr_t>(p) & mask) return false;
    return true;
}
struct Check {
    const char* entry;
    int rc = 0;
    bool empty = false;                  // batch(): no rows, nothing to launch (pointers of empty tensors may be NULL)
    LsnfGeo g;                           // geometry()

    bool refused(int code, const char* fmt, ...) {
        const int n = snprintf(g_err, sizeof(g_err), "%s: ", entry);
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(g_err + n, sizeof(g_err) - n, fmt, ap);
        va_end(ap);
        rc = code;
        return true;
    }
    // a rule of one entry point alone (aliasing, a scalar's range): stated where it applies
    template <class... A> bool refuse(bool violated, const char* fmt, A... a) { return violated && refused(LSNF_E_ARG, fmt, a...); }

    bool geometry(int nz, int width, int depth, int coupling) {
        if (lsnf_geo_init(&g, nz, width, depth, coupling))
            rc = fail(LSNF_E_GEOMETRY, "unsupported geometry nz=%d width=%d depth=%d coupling=%d "
                      "(need nz even in [2,128], width in [1,128], depth in [1,%d], coupling 0 or 1)",
                      nz, width, depth, coupling, LSNF_MAX_DEPTH);
        return rc != 0;
    }
    bool batch(int B, int least = 0) {
        empty = B == 0;
        return refuse(B < least || B > (1 << 28), "B=%d out of range", B);
    }
    bool required(bool all_given) { return refuse(!all_given, "NULL argument"); }
    bool aligned16(const char* names, Ptrs ps) { return refuse(!all_aligned(ps, 15u), "%s must be 16-byte aligned", names); }
    bool aligned4(const char* names, Ptrs ps) { return refuse(!all_aligned(ps, 3u), "%s must be 4-byte aligned", names); }
    // in-kernel noise (LsnfRng): instead of a noise tensor, never beside one.  lsnf_sample and lsnf_sample_keep look at row0 first,
    // the Langevin steps at offset_dev first.
    bool rng(const void* noise, const LsnfRng* r, bool row0_first) {
        if (refuse(noise && r, "pass either a noise tensor or an rng, not both")) return true;
        if (!r) return false;
        auto row0 = [&] { return refuse(r->row0 < 0, "rng->row0 must be >= 0"); };
        auto offset = [&] { return refuse(!aligned8(r->offset_dev), "rng->offset_dev must be 8-byte aligned"); };
        return row0_first ? row0() || offset() : offset() || row0();
    }
    // the depth * 12 parameter pointers (each given and 4-byte aligned) and, with them, the gradient pointers (a NULL one skips
    // its tensor): one walk, so the first offending index speaks whichever table it is in
    bool tables(const float* const* params, const float* const* grads, bool one_message) {
        for (int i = 0; i < g.depth * LSNF_PARAMS_PER_BLOCK; ++i) {
            const bool p_bad = !params[i] || !all_aligned({params[i]}, 3u), g_bad = grads && !all_aligned({grads[i]}, 3u);
            const int block = i / LSNF_PARAMS_PER_BLOCK, slot = i % LSNF_PARAMS_PER_BLOCK;
            if (one_message ? refuse(p_bad || g_bad, "parameter/gradient pointer %d is NULL or misaligned", i)
                            : refuse(p_bad, "parameter pointer %d (block %d, slot %d) is NULL or misaligned", i, block, slot) ||
                              refuse(g_bad, "gradient pointer %d (block %d, slot %d) is misaligned", i, block, slot))
                return true;
        }
        return false;
    }
    // params_workspace of a forward / keeping reverse: the workspace of the lsnf_backward_params call that follows, into which the
    // kernel dumps h1 / h2 of every block.  Returns where the dump goes (NULL: no workspace, or refused -- rc tells)
    float* params_workspace(float* ws, bool with_companions, const char* companions) {
        if (!ws || refuse(!l16_math(), "params_workspace needs a bf16x3-family math mode (lsnf_params_fast_path() == 1)") ||
            refuse(!with_companions, "params_workspace goes with %s", companions) || aligned16("params_workspace", {ws}))
            return nullptr;
        return ws + lsnf_params_workspace_dump(g.nz, g.width, g.depth);
    }
    // From LSNF_X3_MIN_ROWS rows the batch contraction of lsnf_params3.hip may read the dump and asks the workspace's tag word which
    // form h1 / h2 have: tiled (whole 1 KiB stores) when the bf16x3 throughput forward writes them, row-major otherwise
    bool tag_workspace(float* ws, int B, int tiled, hipStream_t stream) {
        if (!ws || B < LSNF_X3_MIN_ROWS) return false;
        const hipDeviceptr_t tag = (hipDeviceptr_t)(ws + lsnf_params_workspace_tag(g.nz, g.width, g.depth, B));
        return hipMemsetD32Async(tag, tiled, 1, stream) != hipSuccess && refused(LSNF_E_HIP, "hipMemsetD32Async(workspace tag) failed");
    }
    // a tiled dump (dump_may_tile below) is read and written with 16-byte row accesses
    bool tiled_rows(bool tiled, const char* with, int B, Ptrs z) {
        return refuse(tiled && !all_aligned(z, 15u), "with %s at B=%d, z_in / z_out / z_saved must be 16-byte aligned", with, B);
    }
    // the descriptor head; rows: every (B, nz) tensor of the call
    void head(LsnfCall& c, const float* plan, int B, void* stream, Ptrs rows) const {
        c.g = g; c.plan = plan; c.B = B; c.vec4 = row_vector_width(g, rows); c.stream = (hipStream_t)stream;
    }
};
LsnfRngArgs rng_args(const LsnfRng* r) {
    return r ? LsnfRngArgs{r->seed, r->offset, r->offset_dev, r->row0, 1} : LsnfRngArgs{0ull, 0ull, nullptr, 0ll, 0};
}

// ---- the rules of a Markov-chain step (lsnf_mala_step, lsnf_reverse_mala_step, lsnf_hmc_step, lsnf_reverse_hmc_step), stated once: an
// entry point describes its call -- its tensors under its own names -- and applies scalars(), its own rules (the two HMC entries:
// phases()), aliases(), the empty-batch return, pointers().
struct Named { const char* name; const void* p; };
struct Needed { const char* name; const void* p; bool when = true; const char* why = "(NULL)"; };      // "<name> is required <why>", when `when`
template <class T>
struct Table {                           // a view of a table of the entry point
    const T* first; const T* last;
    template <size_t N> Table(const T (&t)[N]) : first(t), last(t + N) {}
    const T* begin() const { return first; }
    const T* end() const { return last; }
};
struct ChainStep {
    Table<Named> reads, writes;          // every tensor the call reads / writes (a tensor it does both to: with the writes)
    const Named* next; const Named* point;       // the one pair that may alias: the next point (of writes) over the point (of reads)
    Table<Needed> needed;                // the pointers a non-empty call must bring, in the order they are asked for
    unsigned known;                      // the flags the entry point knows
    bool init, inner;                    // init: no uniform is needed; inner: the call draws and decides nothing
    const char* unless;                  // the flags under which no uniform is needed, by name
    const void* plan; const void* act_saved; const void* noise; const void* uniform; const LsnfRng* rng;
    float step_size; unsigned flags;

    bool scalars(Check& ck) const {
        return ck.refuse(uniform && rng, "pass either a uniform tensor or an rng, not both") || ck.rng(noise, rng, /*row0_first=*/false) ||
               ck.refuse(!std::isfinite(step_size) || step_size == 0.0f, "step_size must be finite and non-zero (got %g)", (double)step_size) ||
               ck.refuse(flags & ~known, "unknown flag bits 0x%x", flags & ~known);
    }
    // no output may be a tensor the call reads, or another output -- but the next point may be the point (every read of a workgroup's
    // rows precedes its stores, and a lane stores the columns it loaded)
    bool aliases(Check& ck) const {
        for (const Named& w : writes) {
            if (!w.p) continue;
            for (const Named& r : reads)
                if (w.p == r.p && !(&w == next && &r == point)) return ck.refuse(true, "%s must not alias %s", w.name, r.name);
            for (const Named& o : writes)
                if (&o != &w && w.p == o.p) return ck.refuse(true, "%s must not alias %s", w.name, o.name);
        }
        return false;
    }
    // the phases of a trajectory (LSNF_HMC_INIT, LSNF_HMC_INNER; `init` / `inner` above): an inner leapfrog step draws nothing and
    // decides nothing
    bool phases(Check& ck, const void* accept_out, const void* log_alpha_out) const {
        return ck.refuse(init && inner, "flags: LSNF_HMC_INIT and LSNF_HMC_INNER exclude each other") ||
               ck.refuse(inner && noise, "noise is not taken with LSNF_HMC_INNER (an inner step draws nothing)") ||
               ck.refuse(inner && uniform, "uniform is not taken with LSNF_HMC_INNER (an inner step draws nothing)") ||
               ck.refuse(inner && rng, "rng is not taken with LSNF_HMC_INNER (an inner step draws nothing)") ||
               ck.refuse(inner && accept_out, "accept_out must be NULL with LSNF_HMC_INNER (an inner step decides nothing)") ||
               ck.refuse(inner && log_alpha_out, "log_alpha_out must be NULL with LSNF_HMC_INNER (an inner step decides nothing)");
    }
    bool pointers(Check& ck) const {
        for (const Needed& n : needed)
            if (ck.refuse(n.when && !n.p, "%s is required %s", n.name, n.why)) return true;
        const bool tensors = !inner && !rng;     // the call draws from tensors: the uniform, and the noise iff it proposes
        if (ck.refuse(tensors && !init && !uniform, "uniform is required without an rng (unless %s)", unless) ||
            ck.refuse(tensors && next->p && !noise, "noise is required with %s when no rng is given", next->name) ||
            ck.refuse(tensors && !next->p && noise, "noise goes with %s: nothing is proposed without it", next->name) ||
            ck.aligned16("plan", {plan}) || ck.aligned16("act_saved", {act_saved}))
            return true;
        for (const Named& r : reads)
            if (ck.aligned4(r.name, {r.p})) return true;
        for (const Named& w : writes)
            if (ck.aligned4(w.name, {w.p})) return true;
        return false;
    }
};

// The rules a step per row adds (lsnf_hmc_step_rows, lsnf_reverse_hmc_step_rows), stated once.  flags(): with the scalars, before the
// empty-batch return (da is host memory); pointers(): with the pointers of a non-empty call.
struct RowSteps {
    const float* step_rows; const float* adapt; const LsnfDualAvg* da; unsigned flags;
    bool adapting() const { return (flags & LSNF_HMC_ADAPT) != 0; }
    bool scalars(Check& ck) const {
        if (ck.refuse(adapting() && (flags & (LSNF_HMC_INIT | LSNF_HMC_INNER)),
                      "flags: LSNF_HMC_ADAPT goes with an end call (neither LSNF_HMC_INIT nor LSNF_HMC_INNER)") ||
            ck.refuse((flags & LSNF_HMC_ADAPT_LAST) && !adapting(), "flags: LSNF_HMC_ADAPT_LAST goes with LSNF_HMC_ADAPT") ||
            ck.refuse(adapting() && !da, "da is required with LSNF_HMC_ADAPT") ||
            ck.refuse(!adapting() && (adapt || da), "adapt and da must be NULL without LSNF_HMC_ADAPT"))
            return true;
        if (!da) return false;
        const float f[] = {da->target_accept, da->gamma, da->t0, da->kappa, da->step_min, da->step_max};
        for (float v : f)
            if (ck.refuse(!std::isfinite(v), "da: every field must be finite (got %g)", (double)v)) return true;
        return ck.refuse(!(da->target_accept > 0.0f && da->target_accept < 1.0f), "da->target_accept must lie in (0, 1) (got %g)", (double)da->target_accept) ||
               ck.refuse(!(da->gamma > 0.0f), "da->gamma must be positive (got %g)", (double)da->gamma) ||
               ck.refuse(!(da->t0 + 1.0f > 0.0f), "da->t0 + 1 must be positive (got t0 = %g)", (double)da->t0) ||
               ck.refuse(!(da->step_min > 0.0f), "da->step_min must be positive (got %g)", (double)da->step_min) ||
               ck.refuse(da->step_max < da->step_min, "da->step_max must not be below da->step_min (got %g < %g)", (double)da->step_max, (double)da->step_min);
    }
    bool pointers(Check& ck) const {
        return ck.refuse(adapting() && !adapt, "adapt is required with LSNF_HMC_ADAPT") || ck.aligned16("adapt", {adapt});
    }
    LsnfDualAvgArgs args() const {
        return da ? LsnfDualAvgArgs{da->target_accept, da->gamma, da->t0, da->kappa, logf(da->step_min), logf(da->step_max)}
                  : LsnfDualAvgArgs{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    }
};

// The rules a metric per row adds (lsnf_hmc_step_metric, lsnf_reverse_hmc_step_metric), stated once, beside RowSteps' and applied after
// them: scalars() before the empty-batch return (reg is host memory), pointers() with the pointers of a non-empty call.  scale_rows
// itself is among the entry point's `needed` and `writes` (required, 4-byte aligned, an output for the aliasing rule).
struct RowMetric {
    const float* mean; const float* m2; const float* count; const LsnfMetricReg* reg; unsigned flags;
    bool folding() const { return (flags & LSNF_HMC_METRIC_FOLD) != 0; }
    bool scalars(Check& ck) const {
        if (ck.refuse(folding() && (flags & (LSNF_HMC_INIT | LSNF_HMC_INNER)),
                      "flags: LSNF_HMC_METRIC_FOLD goes with an end call (neither LSNF_HMC_INIT nor LSNF_HMC_INNER)") ||
            ck.refuse((flags & LSNF_HMC_METRIC_CLOSE) && !folding(), "flags: LSNF_HMC_METRIC_CLOSE goes with LSNF_HMC_METRIC_FOLD") ||
            ck.refuse(folding() && !reg, "reg is required with LSNF_HMC_METRIC_FOLD") ||
            ck.refuse(!folding() && (mean || m2 || count || reg),
                      "mean_rows, m2_rows, count_rows and reg must be NULL without LSNF_HMC_METRIC_FOLD"))
            return true;
        if (!reg) return false;
        const float f[] = {reg->n0, reg->var0, reg->scale_min, reg->scale_max};
        for (float v : f)
            if (ck.refuse(!std::isfinite(v), "reg: every field must be finite (got %g)", (double)v)) return true;
        return ck.refuse(!(reg->n0 >= 0.0f), "reg->n0 must not be negative (got %g)", (double)reg->n0) ||
               ck.refuse(!(reg->var0 >= 0.0f), "reg->var0 must not be negative (got %g)", (double)reg->var0) ||
               ck.refuse(!(reg->scale_min > 0.0f), "reg->scale_min must be positive (got %g)", (double)reg->scale_min) ||
               ck.refuse(reg->scale_max < reg->scale_min, "reg->scale_max must not be below reg->scale_min (got %g < %g)",
                         (double)reg->scale_max, (double)reg->scale_min);
    }
    bool pointers(Check& ck) const {
        return ck.refuse(folding() && !(mean && m2 && count), "mean_rows, m2_rows and count_rows are required with LSNF_HMC_METRIC_FOLD");
    }
    LsnfMetricArgs args() const { return reg ? LsnfMetricArgs{reg->n0, reg->var0, reg->scale_min, reg->scale_max} : LsnfMetricArgs{0.f, 0.f, 0.f, 0.f}; }
};

// The rules a likelihood temperature per row adds (lsnf_hmc_step_tempered, lsnf_reverse_hmc_step_tempered), stated once, beside
// RowMetric's and applied after them: scalars() before the empty-batch return, pointers() with the pointers of a non-empty call.
// beta_rows, like_grad_acc and like_u_acc themselves are among the entry point's `needed` and `writes`; the temperatures are device
// memory and are not looked at on the host.
struct RowTemper {
    const float* beta_next; const float* log_w; unsigned flags;
    bool annealing() const { return (flags & LSNF_HMC_ANNEAL) != 0; }
    bool scalars(Check& ck) const {
        return ck.refuse(annealing() && (flags & LSNF_HMC_INNER),
                         "flags: LSNF_HMC_ANNEAL goes with LSNF_HMC_INIT or an end call, not with LSNF_HMC_INNER") ||
               ck.refuse(!annealing() && (beta_next || log_w), "beta_next and log_w must be NULL without LSNF_HMC_ANNEAL");
    }
    bool pointers(Check& ck) const {
        return ck.refuse(annealing() && !(beta_next && log_w), "beta_next and log_w are required with LSNF_HMC_ANNEAL") ||
               ck.refuse(!aligned8(log_w), "log_w must be 8-byte aligned");
    }
};

// The rules a replica-exchange move adds (lsnf_hmc_step_exchange, lsnf_reverse_hmc_step_exchange), stated once, beside RowTemper's and
// applied after them: scalars() before the empty-batch return, pointers() with the pointers of a non-empty call.  swap_uniform is among
// the entry point's `reads`, swap_out and log_swap_out among its `writes`.
struct RowExchange {
    int ladder; int B; const float* swap_uniform; const float* swap_out; const float* log_swap_out; const LsnfRng* rng; unsigned flags;
    bool swapping() const { return (flags & LSNF_HMC_SWAP) != 0; }
    bool scalars(Check& ck) const {
        return ck.refuse((flags & LSNF_HMC_SWAP_ODD) && !swapping(), "flags: LSNF_HMC_SWAP_ODD goes with LSNF_HMC_SWAP") ||
               ck.refuse(swapping() && (flags & (LSNF_HMC_INIT | LSNF_HMC_INNER)),
                         "flags: LSNF_HMC_SWAP goes with an end call (neither LSNF_HMC_INIT nor LSNF_HMC_INNER)") ||
               ck.refuse(swapping() && (flags & (LSNF_HMC_ADAPT | LSNF_HMC_METRIC_FOLD | LSNF_HMC_METRIC_CLOSE | LSNF_HMC_ANNEAL)),
                         "flags: LSNF_HMC_SWAP excludes LSNF_HMC_ADAPT, LSNF_HMC_METRIC_FOLD, LSNF_HMC_METRIC_CLOSE and LSNF_HMC_ANNEAL") ||
               ck.refuse(swapping() && !(ladder == 2 || ladder == 4 || ladder == 8 || ladder == 16),
                         "ladder must be 2, 4, 8 or 16 with LSNF_HMC_SWAP (got %d)", ladder) ||
               ck.refuse(swapping() && B % ladder != 0, "B=%d is not a multiple of ladder=%d", B, ladder) ||
               ck.refuse(!swapping() && (swap_uniform || swap_out || log_swap_out),
                         "swap_uniform, swap_out and log_swap_out must be NULL without LSNF_HMC_SWAP") ||
               ck.refuse(swap_uniform && rng, "swap_uniform goes with a noise tensor, not with an rng (the pair's uniform is drawn in-kernel)");
    }
    bool pointers(Check& ck) const {
        return ck.refuse(swapping() && !rng && !swap_uniform, "swap_uniform is required with LSNF_HMC_SWAP when no rng is given");
    }
};

// The rules a resampling move adds (lsnf_hmc_step_resample, lsnf_reverse_hmc_step_resample), stated once, beside RowTemper's and
// applied after them: scalars() before the empty-batch return, pointers() with the pointers of a non-empty call.  resample_uniform is
// among the entry point's `reads`, ancestor_out and ess_out among its `writes`.  (LSNF_HMC_SWAP is not among these entries' flags.)
struct RowResample {
    int group; int B; const float* resample_uniform; const float* ancestor_out; const float* ess_out; const LsnfRng* rng; unsigned flags;
    bool resampling() const { return (flags & LSNF_HMC_RESAMPLE) != 0; }
    bool scalars(Check& ck) const {
        return ck.refuse(resampling() && (flags & (LSNF_HMC_INIT | LSNF_HMC_INNER)),
                         "flags: LSNF_HMC_RESAMPLE goes with an end call (neither LSNF_HMC_INIT nor LSNF_HMC_INNER)") ||
               ck.refuse(resampling() && !(flags & LSNF_HMC_ANNEAL), "flags: LSNF_HMC_RESAMPLE goes with LSNF_HMC_ANNEAL") ||
               ck.refuse(resampling() && (flags & (LSNF_HMC_ADAPT | LSNF_HMC_METRIC_FOLD | LSNF_HMC_METRIC_CLOSE)),
                         "flags: LSNF_HMC_RESAMPLE excludes LSNF_HMC_ADAPT, LSNF_HMC_METRIC_FOLD and LSNF_HMC_METRIC_CLOSE") ||
               ck.refuse(resampling() && !(group == 2 || group == 4 || group == 8 || group == 16),
                         "group must be 2, 4, 8 or 16 with LSNF_HMC_RESAMPLE (got %d)", group) ||
               ck.refuse(resampling() && B % group != 0, "B=%d is not a multiple of group=%d", B, group) ||
               ck.refuse(!resampling() && (resample_uniform || ancestor_out || ess_out),
                         "resample_uniform, ancestor_out and ess_out must be NULL without LSNF_HMC_RESAMPLE") ||
               ck.refuse(resample_uniform && rng,
                         "resample_uniform goes with a noise tensor, not with an rng (the group's uniform is drawn in-kernel)");
    }
    bool pointers(Check& ck) const {
        return ck.refuse(resampling() && !rng && !resample_uniform,
                         "resample_uniform is required with LSNF_HMC_RESAMPLE when no rng is given");
    }
};

// The rules a schedule search adds (lsnf_hmc_step_schedule, lsnf_reverse_hmc_step_schedule), stated once, beside RowResample's and
// applied after them: all of them are scalars, refused before the empty-batch return.  `group` serves the search and the resampling
// move; RowResample's own rules (LSNF_HMC_RESAMPLE not on LSNF_HMC_INIT among them) hold unchanged.
struct RowSchedule {
    int group; int B; float cess_frac; float min_step; unsigned flags;
    bool scheduling() const { return (flags & LSNF_HMC_SCHEDULE) != 0; }
    bool scalars(Check& ck) const {
        return ck.refuse(scheduling() && (flags & LSNF_HMC_INNER),
                         "flags: LSNF_HMC_SCHEDULE goes with LSNF_HMC_INIT or an end call, not with LSNF_HMC_INNER") ||
               ck.refuse(scheduling() && !(flags & LSNF_HMC_ANNEAL), "flags: LSNF_HMC_SCHEDULE goes with LSNF_HMC_ANNEAL") ||
               ck.refuse(scheduling() && (flags & (LSNF_HMC_ADAPT | LSNF_HMC_METRIC_FOLD | LSNF_HMC_METRIC_CLOSE)),
                         "flags: LSNF_HMC_SCHEDULE excludes LSNF_HMC_ADAPT, LSNF_HMC_METRIC_FOLD and LSNF_HMC_METRIC_CLOSE") ||
               ck.refuse(scheduling() && !(group == 2 || group == 4 || group == 8 || group == 16),
                         "group must be 2, 4, 8 or 16 with LSNF_HMC_SCHEDULE (got %d)", group) ||
               ck.refuse(scheduling() && B % group != 0, "B=%d is not a multiple of group=%d", B, group) ||
               ck.refuse(scheduling() && !(cess_frac > 0.0f && cess_frac < 1.0f),
                         "cess_frac must lie in (0, 1) with LSNF_HMC_SCHEDULE (got %g)", (double)cess_frac) ||
               ck.refuse(scheduling() && !(std::isfinite(min_step) && min_step >= 0.0f),
                         "min_step must be finite and not negative with LSNF_HMC_SCHEDULE (got %g)", (double)min_step);
    }
};

// ---- kernel selection: each operation decides on the host, from the kernels' coverage predicates, which kernel(s) a call
// runs, BEFORE anything is launched; the entry point then launches exactly that.  A launcher reached outside what it covers
// is a selection bug and fails the call (LSNF_E_HIP, the kernel named in lsnf_last_error()); nothing falls through to another
// kernel.
enum Kernel {
    K_NONE, K_FWD, K_FWD3, K_FWD3Q, K_FWD2H_FIXUP, K_SMALL_FWD, K_SMALL3_FWD,
    K_REV, K_REV3, K_REV2H_FIXUP, K_SMALL_REV, K_SMALL3_REV,
    K_BWD, K_BWD3, K_SMALL_BWD, K_SMALL3_BWD,
    K_SMALL3_RBWD, K_SMALL3_RLV, K_SMALL3_MALA, K_SMALL3_RMALA, K_SMALL3_HMC, K_SMALL3_RHMC,
    K_SMALL3_HMCR, K_SMALL3_RHMCR, K_SMALL3_HMCM, K_SMALL3_RHMCM, K_SMALL3_HMCT, K_SMALL3_RHMCT, K_SMALL3_HMCX, K_SMALL3_RHMCX,
    K_SMALL3_HMCS, K_SMALL3_RHMCS, K_SMALL3_HMCA, K_SMALL3_RHMCA,
};
const char* const kKernelName[] = {
    "no kernel takes this call", "lsnf_fwd_kernel", "lsnf_fwd3b_kernel", "lsnf_fwd3q_kernel",
    "lsnf_fwd2h_kernel + lsnf_fwd3b_kernel fix-up", "lsnf_small_fwd_kernel", "lsnf_small3_fwd_kernel",
    "lsnf_rev_kernel", "lsnf_rev3_kernel", "lsnf_rev2h_kernel + lsnf_rev3_kernel fix-up", "lsnf_small_rev_kernel",
    "lsnf_small3_rev_kernel",
    "lsnf_bwd_z_kernel", "lsnf_bwd3_kernel", "lsnf_small_bwd_kernel", "lsnf_small3_bwd_kernel",
    "lsnf_small3_rbwd_kernel", "lsnf_small3_rbwd_kernel (update form)", "lsnf_small3_mala_kernel", "lsnf_small3_rmala_kernel",
    "lsnf_small3_hmc_kernel", "lsnf_small3_rhmc_kernel",
    "lsnf_small3_hmcr_kernel", "lsnf_small3_rhmcr_kernel", "lsnf_small3_hmcm_kernel", "lsnf_small3_rhmcm_kernel",
    "lsnf_small3_hmct_kernel", "lsnf_small3_rhmct_kernel", "lsnf_small3_hmcx_kernel", "lsnf_small3_rhmcx_kernel",
    "lsnf_small3_hmcs_kernel", "lsnf_small3_rhmcs_kernel", "lsnf_small3_hmca_kernel", "lsnf_small3_rhmca_kernel",
};
struct Pick { Kernel k; int st = 0; };     // st: rows per workgroup / 16 of the small3 kernels

int launch_fail(hipError_t e, const char* entry, Kernel k) {
    if (k == K_NONE) return fail(LSNF_E_HIP, "%s: %s", entry, kKernelName[k]);
    return fail(LSNF_E_HIP, "%s: %s: %s", entry, kKernelName[k], hipGetErrorString(e));
}
// the tail of every selecting entry point: what the launch(es) of its pick answered
int report(const char* entry, Pick p, hipError_t e) { return p.k == K_NONE || e != hipSuccess ? launch_fail(e, entry, p.k) : LSNF_OK; }

// Forward.  Up to small_max rows the latency kernels (the bf16-pipe one for the bf16x3 family, 16 x ST rows per workgroup; the
// fp32-MFMA one, 32 rows, otherwise), above it the throughput kernels (weights shared through LDS):
//  - fp16x2 (opt-in): two fp16 terms per operand, three MFMAs per product (lsnf_fwd2h.hip), followed by the bf16x3 kernel as a
//    fix-up pass that recomputes the workgroups in which a wave met an operand outside fp16's range (the flag travels in
//    logdet_out) and exits at once elsewhere.  Not for in-place calls (the fix-up re-reads the inputs) and not with in-kernel
//    batch sums (a partial recomputation cannot repair them): those run the bf16x3 kernel directly;
//  - bf16x3: the vector work software-pipelined under 16x16x32 MFMAs (lsnf_fwd3p.hip) where it applies;
//  - the bf16x3 family: the error-free split on the bf16 matrix pipe (lsnf_fwd3.hip);
//  - the fp32-MFMA kernel -- not with the parameter-gradient dump, which only the bf16 kernels write.
Pick select_forward(const LsnfForwardCall& c, int small_max) {
    const int math = math_mode();
    if (c.B <= small_max) {
        if (l16_math())
            if (int st = lsnf_small3_forward_st(c)) return {K_SMALL3_FWD, st};
        return {!c.hdump && lsnf_small_forward_covers(c) ? K_SMALL_FWD : K_NONE};
    }
    if (math == LSNF_MATH_FP16X2 && !c.stats && c.z_in != c.z_out && (c.objective == nullptr || c.objective != c.logdet_out) &&
        lsnf_forward2h_covers(c, /*fixup=*/0) && lsnf_forward3_covers(c, /*fixup=*/1))
        return {K_FWD2H_FIXUP};
    if (math == LSNF_MATH_BF16X3 && (!c.hdump || c.hdump_tiled) && lsnf_forward3q_covers(c)) return {K_FWD3Q};
    if (l16_math() && lsnf_forward3_covers(c, /*fixup=*/0)) return {K_FWD3};
    return {c.hdump ? K_NONE : K_FWD};
}
// the launch(es) of a forward pick
hipError_t launch_forward(Pick p, const LsnfForwardCall& c) {
    switch (p.k) {
    case K_SMALL3_FWD: return lsnf_launch_small3_forward(c, p.st);
    case K_SMALL_FWD: return lsnf_launch_small_forward(c);
    case K_FWD2H_FIXUP: {
        LsnfForwardCall pair = c;
        pair.stats = nullptr; pair.hdump_tiled = 0;      // (both launches of the fp16x2 pair: no in-kernel batch sums, the dump row-major)
        const hipError_t e = lsnf_launch_forward2h(pair, /*fixup=*/0);
        return e != hipSuccess ? e : lsnf_launch_forward3(pair, /*fixup=*/1);
    }
    case K_FWD3Q: return lsnf_launch_forward3q(c);
    case K_FWD3: return lsnf_launch_forward3(c, /*fixup=*/0);
    case K_FWD: return lsnf_launch_forward(c);
    default: return hipSuccess;
    }
}

// Reverse (sampling).  It neither writes nor reads a stash, so under the automatic threshold the bf16x3 family takes its own
// crossover: the 64-row latency form is the faster one up to ~28 K rows (profiles/r03_latency_reverse.txt: 34.2 vs 57.9 us at
// 16 384, 67.3 vs 60.6 at 32 768); above it the throughput kernel (lsnf_rev3.hip; fp16x2: lsnf_rev2h.hip + the bf16x3 fix-up
// pass, as in the forward).  The latency form also stands in where the throughput form does not fit (it is faster than the
// fp32 throughput reverse), and the throughput form where the latency form does not.  Otherwise the fp32-MFMA kernels of the
// batch size's family.
Pick select_reverse(const LsnfReverseCall& c) {
    const int small_max = small_batch_max();
    if (l16_math()) {
        const int math = math_mode();
        int lat_max = small_max;
        if (small_batch_setting() == LSNF_SMALL_BATCH_AUTO && math != LSNF_MATH_FP16X2 && lat_max < 24576) lat_max = 24576;
        if (c.B > lat_max) {
            if (math == LSNF_MATH_FP16X2 && c.z_in != c.z_out && (c.objective == nullptr || c.objective != c.objective_out) &&
                lsnf_reverse2h_covers(c) && lsnf_reverse3_covers(c))
                return {K_REV2H_FIXUP};
            if (lsnf_reverse3_covers(c)) return {K_REV3};
        }
        if (lat_max > 0)
            if (int st = lsnf_small3_reverse_st(c)) return {K_SMALL3_REV, st};
        if (c.B > small_max && c.B <= lat_max && lsnf_reverse3_covers(c)) return {K_REV3};
    }
    if (c.B > small_max) return {K_REV};
    return {lsnf_small_reverse_covers(c) ? K_SMALL_REV : K_NONE};
}
// Sampling (lsnf_sample) is the reverse's kernels in their sampling form (c.smp), so the reverse's selection -- same families,
// same crossovers -- for a call whose inputs alias nothing: lsnf_sample leaves z_in / objective NULL (under fp16x2 the fix-up
// pass redraws the rows of the workgroups it recomputes).
// the launch(es) of a reverse / sampling pick
hipError_t launch_reverse(Pick p, const LsnfReverseCall& c) {
    switch (p.k) {
    case K_REV2H_FIXUP: {
        const hipError_t e = lsnf_launch_reverse2h(c, /*fixup=*/0);
        return e != hipSuccess ? e : lsnf_launch_reverse3(c, /*fixup=*/1);
    }
    case K_REV3: return lsnf_launch_reverse3(c, /*fixup=*/0);
    case K_SMALL3_REV: return lsnf_launch_small3_reverse(c, p.st);
    case K_SMALL_REV: return lsnf_launch_small_reverse(c);
    case K_REV: return lsnf_launch_reverse(c);
    default: return hipSuccess;
    }
}

// The stash-keeping forms (lsnf_reverse_keep, lsnf_sample_keep) exist for the latency bf16x3 kernel alone.  ONE rule, for the query
// and both entry points: a bf16x3-family mode, B within the common threshold (the family that writes a stash is the family the
// forward would have picked: the parameter-gradient dump is then row-major) and a workgroup shape of that kernel for the call.  Under it
// select_reverse picks the same kernel for the plain call, so the outputs of the two are the same bits.
bool reverse_keep_covers(const LsnfReverseCall& c) {
    return l16_math() && c.B <= small_batch_max() && lsnf_small3_reverse_st(c) != 0;
}
// A checked reverse / sampling call (the descriptor filled but for the three tensors below) to its launch: the plain selection, or
// -- keep: lsnf_reverse_keep, lsnf_sample_keep -- the rules of the three optional tensors (as lsnf_forward's), the coverage rule,
// the workspace tag and the one kernel that keeps a stash.
int reverse_launch(Check& ck, LsnfReverseCall& c, bool keep, float* z_saved, float* act_saved, float* params_workspace) {
    if (!keep) {
        const Pick p = select_reverse(c);
        return report(ck.entry, p, launch_reverse(p, c));
    }
    const float* eps_out = c.smp ? c.smp->eps_out : nullptr;
    // (an in-place call would overwrite the last block's output, which every backward must be given as z_out: the stash would be useless)
    if (ck.aligned4("tensors", {z_saved}) || ck.aligned16("act_saved", {act_saved}) ||
        ck.refuse(z_saved && (z_saved == c.z_in || z_saved == c.z_out || z_saved == eps_out), "z_saved must not alias another tensor of the call") ||
        ck.refuse((z_saved || act_saved) && c.z_in && c.z_in == c.z_out,
                  "z_out must not alias z_in when z_saved / act_saved are kept (the backward reads z_in)"))
        return ck.rc;
    c.z_saved = z_saved; c.act_saved = act_saved;
    c.hdump = ck.params_workspace(params_workspace, act_saved && (c.g.depth == 1 || z_saved), "act_saved and z_saved");
    if (ck.rc ||
        ck.refuse(c.smp && (act_saved || z_saved) && !eps_out, "act_saved / z_saved need eps_out (the last block's output, which the backward reads)") ||
        ck.refuse(!reverse_keep_covers(c), "only the latency bf16x3 reverse keeps a stash: needs a bf16x3-family math mode and B=%d <= the "
                  "small-batch threshold %d (lsnf_reverse_keep_covers)", c.B, small_batch_max()) ||
        ck.tag_workspace(params_workspace, c.B, /*tiled=*/0, c.stream))      // (this kernel's h1 / h2 are row-major)
        return ck.rc;
    const Pick p = {K_SMALL3_REV, lsnf_small3_reverse_st(c)};
    return report(ck.entry, p, launch_reverse(p, c));
}
// lsnf_reverse and lsnf_reverse_keep
int reverse_entry(const char* entry, bool keep, const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_in,
                  const float* objective, float* z_out, float* objective_out, float* z_saved, float* act_saved, float* params_workspace,
                  void* stream) {
    Check ck{entry};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B)) return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (ck.required(plan && z_in && z_out) || ck.aligned16("plan", {plan}) || ck.aligned4("tensors", {z_in, z_out, objective, objective_out}))
        return ck.rc;
    LsnfReverseCall c;
    ck.head(c, plan, B, stream, {z_in, z_out, z_saved});
    c.z_in = z_in; c.objective = objective; c.z_out = z_out; c.objective_out = objective_out;
    return reverse_launch(ck, c, keep, z_saved, act_saved, params_workspace);
}
// lsnf_sample and lsnf_sample_keep: the reverse's kernels in their sampling form (c.smp)
int sample_entry(const char* entry, bool keep, const float* plan, int nz, int width, int depth, int coupling, int B, const LsnfRng* rng,
                 float temperature, float* z_out, float* objective_out, float* eps_out, float* ll_out, float* z_saved, float* act_saved,
                 float* params_workspace, void* stream) {
    Check ck{entry};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || ck.refuse(!rng, "rng is required") || ck.rng(nullptr, rng, /*row0_first=*/true) ||
        ck.refuse(!std::isfinite(temperature) || temperature < 0.0f, "temperature must be finite and >= 0 (got %g)", (double)temperature))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (ck.required(plan && z_out) || ck.aligned16("plan", {plan}) || ck.aligned4("tensors", {z_out, objective_out, eps_out, ll_out}) ||
        ck.refuse(eps_out == z_out, "eps_out must not alias z_out"))
        return ck.rc;
    const LsnfSampleArgs smp = {rng_args(rng), temperature, eps_out, ll_out};
    LsnfReverseCall c;                   // (z_in / objective stay NULL: the kernels draw the rows)
    ck.head(c, plan, B, stream, {z_out, eps_out, z_saved});
    c.z_out = z_out; c.objective_out = objective_out; c.smp = &smp;
    return reverse_launch(ck, c, keep, z_saved, act_saved, params_workspace);
}

// Backward (lsnf_backward_z, lsnf_langevin_step, lsnf_backward_params): from the activation stash on the bf16 matrix pipe when
// the call brings one under a bf16x3-family mode (lsnf_small3_bwd.hip / lsnf_bwd3.hip: both take every such call), otherwise
// the recomputing fp32-MFMA kernels -- the latency or the throughput family by the common threshold, so that the family that
// wrote a stash is the family that reads it.
Pick select_backward(const LsnfBackwardCall& c) {
    const bool small = c.B <= small_batch_max();
    if (c.act_saved && l16_math()) return small ? Pick{K_SMALL3_BWD, lsnf_small3_backward_st(c)} : Pick{K_BWD3};
    if (!small) return {K_BWD};
    return {lsnf_small_backward_covers(c) ? K_SMALL_BWD : K_NONE};
}
hipError_t launch_backward(Pick p, const LsnfBackwardCall& c) {
    switch (p.k) {
    case K_SMALL3_BWD: return lsnf_launch_small3_backward_z(c, p.st);
    case K_BWD3: return lsnf_launch_backward3_z(c);
    case K_SMALL_BWD: return lsnf_launch_small_backward_z(c);
    case K_BWD: return lsnf_launch_backward_z(c);
    default: return hipSuccess;
    }
}
int backward_launch(const char* entry, const LsnfBackwardCall& c) {      // lsnf_backward_z, lsnf_langevin_step
    const Pick p = select_backward(c);
    return report(entry, p, launch_backward(p, c));
}

// Backward of the reverse pass (lsnf_reverse_backward_z): one kernel (lsnf_small3_rbwd.hip) whose bf16x3 arithmetic is not narrower
// than fp32, so it serves every math mode; its workgroup shape follows the batch size alone (more rounds of workgroups above
// 16 384 rows), not the small-batch threshold -- it reads the stash of whichever forward family the threshold selected.
Pick select_reverse_backward(const LsnfReverseBackwardCall& c) { return {K_SMALL3_RBWD, lsnf_small3_reverse_backward_st(c)}; }
// The base-space Langevin step (lsnf_reverse_langevin_step) is that kernel with the update as its output section: the same one
// kernel under every math mode and batch size, the same workgroup shape as the plain backward of the call.
Pick select_reverse_langevin(const LsnfReverseLangevinCall& c) { return {K_SMALL3_RLV, lsnf_small3_reverse_backward_st(c)}; }
// The Metropolis-adjusted step (lsnf_mala_step) is the latency bf16x3 backward with the accept / reject tail as its output section
// (lsnf_small3_mala.hip): like the two above, one kernel under every math mode and batch size, whatever the small-batch threshold.
Pick select_mala(const LsnfMalaCall& c) { return {K_SMALL3_MALA, lsnf_small3_backward_st(c)}; }
// Its base-space form (lsnf_reverse_mala_step) is the reverse-backward with that tail (lsnf_small3_rmala.hip): one kernel again, the
// workgroup shape of the plain reverse-backward of the call.
Pick select_reverse_mala(const LsnfReverseMalaCall& c) { return {K_SMALL3_RMALA, lsnf_small3_reverse_backward_st(c)}; }
// Hamiltonian Monte Carlo in z (lsnf_hmc_step) is the same backward with the leapfrog tail (lsnf_small3_hmc.hip): one kernel under
// every math mode, batch size and phase of a trajectory, the workgroup shape of the plain backward of the call.
Pick select_hmc(const LsnfHmcCall& c) { return {K_SMALL3_HMC, lsnf_small3_backward_st(c)}; }
// Its base-space form (lsnf_reverse_hmc_step) is the reverse-backward with the leapfrog tail (lsnf_small3_rhmc.hip): one kernel under
// every math mode, batch size and phase, the workgroup shape of the plain reverse-backward of the call.
Pick select_reverse_hmc(const LsnfReverseHmcCall& c) { return {K_SMALL3_RHMC, lsnf_small3_reverse_backward_st(c)}; }
// The two with a step per row (lsnf_hmc_step_rows, lsnf_reverse_hmc_step_rows): the same kernel texts with the per-row tail
// (lsnf_small3_hmcr.hip, lsnf_small3_rhmcr.hip), the same instantiations, the same rule for the workgroup shape.
Pick select_hmc_rows(const LsnfHmcRowsCall& c) { return {K_SMALL3_HMCR, lsnf_small3_backward_st(c)}; }
Pick select_reverse_hmc_rows(const LsnfReverseHmcRowsCall& c) { return {K_SMALL3_RHMCR, lsnf_small3_reverse_backward_st(c)}; }
// The two with a metric per row (lsnf_hmc_step_metric, lsnf_reverse_hmc_step_metric): lsnf_small3_hmcm.hip, lsnf_small3_rhmcm.hip, likewise.
Pick select_hmc_metric(const LsnfHmcMetricCall& c) { return {K_SMALL3_HMCM, lsnf_small3_backward_st(c)}; }
Pick select_reverse_hmc_metric(const LsnfReverseHmcMetricCall& c) { return {K_SMALL3_RHMCM, lsnf_small3_reverse_backward_st(c)}; }
// The two with a likelihood temperature per row (lsnf_hmc_step_tempered, lsnf_reverse_hmc_step_tempered): lsnf_small3_hmct.hip,
// lsnf_small3_rhmct.hip, likewise.
Pick select_hmc_tempered(const LsnfHmcTemperedCall& c) { return {K_SMALL3_HMCT, lsnf_small3_backward_st(c)}; }
Pick select_reverse_hmc_tempered(const LsnfReverseHmcTemperedCall& c) { return {K_SMALL3_RHMCT, lsnf_small3_reverse_backward_st(c)}; }
// The two with a replica-exchange move (lsnf_hmc_step_exchange, lsnf_reverse_hmc_step_exchange): lsnf_small3_hmcx.hip,
// lsnf_small3_rhmcx.hip, likewise.
Pick select_hmc_exchange(const LsnfHmcExchangeCall& c) { return {K_SMALL3_HMCX, lsnf_small3_backward_st(c)}; }
Pick select_reverse_hmc_exchange(const LsnfReverseHmcExchangeCall& c) { return {K_SMALL3_RHMCX, lsnf_small3_reverse_backward_st(c)}; }
// The two with a resampling move (lsnf_hmc_step_resample, lsnf_reverse_hmc_step_resample): lsnf_small3_hmcs.hip,
// lsnf_small3_rhmcs.hip, likewise.
Pick select_hmc_resample(const LsnfHmcResampleCall& c) { return {K_SMALL3_HMCS, lsnf_small3_backward_st(c)}; }
Pick select_reverse_hmc_resample(const LsnfReverseHmcResampleCall& c) { return {K_SMALL3_RHMCS, lsnf_small3_reverse_backward_st(c)}; }
// The two with a schedule search (lsnf_hmc_step_schedule, lsnf_reverse_hmc_step_schedule): lsnf_small3_hmca.hip, lsnf_small3_rhmca.hip.
Pick select_hmc_schedule(const LsnfHmcScheduleCall& c) { return {K_SMALL3_HMCA, lsnf_small3_backward_st(c)}; }
Pick select_reverse_hmc_schedule(const LsnfReverseHmcScheduleCall& c) { return {K_SMALL3_RHMCA, lsnf_small3_reverse_backward_st(c)}; }

// Batch contraction of the parameter gradients (LsnfContraction): on the bf16 matrix pipe where lsnf_params3.hip covers the
// call (use_x3); from 4 096 rows the fp32-MFMA kernel through LDS, with the widest row loads the rows allow -- every row the
// tasks read starts 16-byte aligned iff nz, width and half are multiples of 4 (z tensors: the caller's alignment is folded
// into vec4; the dump rows start at 16-byte aligned offsets of the 16-byte aligned workspace); the plain kernel below that
// (and with LSNF_TN_PLAIN set: experiment knob of tools/tn_probe.py).
int select_contraction(const LsnfGeo& g, int B, bool use_x3, int vec4) {
    static const bool knob_plain = getenv("LSNF_TN_PLAIN") != nullptr;
    if (use_x3) return LSNF_CONTRACT_X3;
    if (B < 4096 || knob_plain) return LSNF_CONTRACT_PLAIN;
    if (vec4 == 4 && g.nz % 4 == 0 && g.width % 4 == 0 && g.half % 4 == 0) return LSNF_CONTRACT_LDS4;
    if (vec4 >= 2 && g.nz % 2 == 0 && g.width % 2 == 0 && g.half % 2 == 0) return LSNF_CONTRACT_LDS2;
    return LSNF_CONTRACT_LDS1;
}

// The fast path's h dump is tiled iff the bf16x3 / bf16x3_phased throughput forward writes it and the contraction of
// lsnf_params3.hip covers the call; that contraction is the one reader that asks the workspace's tag, and it needs 16-byte
// aligned z tensors.  Where this returns true, lsnf_forward(params_workspace) and lsnf_backward_params(act_saved) therefore
// both refuse z tensors that are not 16-byte aligned: a backward that re-decided on pointers of another alignment than the
// forward's would hand a tiled dump to the fp32 contraction, which reads it row-major.
bool dump_may_tile(const LsnfGeo& g, int B, int small_max) {
    const int math = math_mode();
    LsnfContractCall any;                // (the contraction's rule for the call's shape: no tensors, NULL is 16-byte aligned)
    any.g = g; any.B = B;
    return B > small_max && (math == LSNF_MATH_BF16X3 || math == LSNF_MATH_BF16X3_PHASED) && lsnf_dump_can_tile(g.nz, g.width) &&
           lsnf_contract_x3_covers(any);
}
// lsnf_backward_params (det = 0) and lsnf_backward_params_det (det = 1): one validation, one selection, one set of alignment rules
int backward_params_entry(const char* entry, int det, const float* plan, const float* const* params_host, float* const* grads_host, int nz, int width,
                          int depth, int coupling, int B, const float* z_in, const float* z_out, const float* z_saved,
                          const float* act_saved, const float* g_z1, const float* g_logdet, int ll_mode, float ll_scale,
                          float* g_z_in, float* workspace, void* stream) {
    Check ck{entry};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B, 1) ||
        ck.required(plan && params_host && grads_host && z_in && z_out && workspace && (depth == 1 || z_saved)) ||
        ck.aligned16("plan/workspace", {plan, workspace}) || ck.tables(params_host, grads_host, /*one_message=*/true) ||
        ck.aligned4("tensors", {z_in, z_out, z_saved, g_z1, g_logdet, g_z_in}) || ck.aligned16("act_saved", {act_saved}))
        return ck.rc;
    const LsnfGeo& g = ck.g;
    // Fast path (act_saved given, bf16x3-family math): the forward of this evaluation kept the activation stash and wrote h1 / h2
    // into this workspace's dump (lsnf_forward(params_workspace)); the backward FROM THE STASH, on the bf16 matrix pipe, adds
    // g_v, g_a1, g_a2, g_t, g_p -- no recomputation of the coupling MLP (1.0x instead of 1.5x the forward's matrix work, at
    // 2.6x the matrix rate).  Otherwise: the recomputing fp32-MFMA backward writes all seven tensors itself.
    // Large batches on the fast path: the contraction runs on the bf16 matrix pipe, operands read once (lsnf_params3.hip;
    // LSNF_TN_X3=0 keeps the fp32-MFMA kernels), and the throughput backward then writes its g arrays in the tiled form (whole
    // 1 KiB stores instead of 16 rows x 64 bytes; g_v as its first half only: the second half is g_t)
    if (!l16_math()) act_saved = nullptr;
    if (ck.tiled_rows(act_saved && dump_may_tile(g, B, small_batch_max()), "act_saved", B, {z_in, z_out, z_saved})) return ck.rc;
    // workspace: G = sum_b dL/dlogdet_b (one double in floats 0-1: in float32 the per-wave atomics lost up to ~1e-5 of it, and
    // G * 3 / G * W^-T cancel against the data terms of the actnorm.logs / 1x1-conv gradients), the folded gradients (zeroed:
    // both accumulate by atomics), then the dump the backward writes
    const size_t folded = lsnf_params_workspace_dump(nz, width, depth);
    LsnfBackwardCall b;
    // (z_in too: the batch contraction of block 0 reads its rows with the same vector width)
    ck.head(b, plan, B, stream, {z_in, z_out, g_z_in, z_saved, g_z1});
    LsnfContractCall c;
    static_cast<LsnfCall&>(c) = b;       // (the same head)
    b.z_out = z_out; b.z_saved = z_saved; b.act_saved = act_saved; b.g_z1 = g_z1; b.g_logdet = g_logdet;
    b.ll_mode = ll_mode; b.ll_scale = ll_scale; b.g_z_in = g_z_in;
    // (det: G is summed in a fixed order by lsnf_fold_reduce_kernel; the kernels' atomic sum goes to the spare floats 2-3)
    b.dump = workspace + folded; b.gl_total = reinterpret_cast<double*>(workspace + (det ? 2 : 0));
    c.params_host = params_host; c.grads_host = grads_host; c.z_in = z_in; c.z_out = z_out; c.z_saved = z_saved; c.workspace = workspace;
    c.det = det; c.g_logdet = g_logdet; c.ll_mode = ll_mode; c.ll_scale = ll_scale;
    const Pick p = select_backward(b);
    const bool use_x3 = act_saved && lsnf_contract_x3_covers(c);
    const int contraction = select_contraction(g, B, use_x3, b.vec4);
    b.dump_tiled = c.g_tiled = (use_x3 && p.k == K_BWD3 && lsnf_dump_can_tile(nz, width)) ? 1 : 0;
    if (p.k == K_NONE) return launch_fail(hipSuccess, entry, p.k);
    // (det: the reduce kernel writes every element of the fold; only the header is accumulated into)
    hipError_t e = hipMemsetAsync(workspace, 0, sizeof(float) * (det ? 4 : folded), b.stream);
    if (e != hipSuccess) return hip_fail(e, det ? "lsnf_backward_params_det: hipMemsetAsync(workspace)" : "lsnf_backward_params: hipMemsetAsync(workspace)");
    e = launch_backward(p, b);
    if (e != hipSuccess) return launch_fail(e, entry, p.k);
    e = lsnf_launch_params_contract(c, contraction);
    if (e != hipSuccess)
        return hip_fail(e, det ? "lsnf_backward_params_det: contraction / lsnf_fold_reduce_kernel / lsnf_unfold_kernel"
                               : contraction == LSNF_CONTRACT_X3 ? "lsnf_backward_params: lsnf_contract_x3_kernel / lsnf_unfold_kernel"
                                                                 : "lsnf_backward_params: lsnf_tn_gemm kernel / lsnf_unfold_kernel");
    return LSNF_OK;
}

}  // namespace

extern "C" {

int lsnf_abi_version(void) { return LSNF_ABI_VERSION; }

int lsnf_set_small_batch_max(int rows) {
    if (rows == -1) return small_batch_max();                      // query: the threshold in force
    const int prev = small_batch_setting();                        // what was SET: rows, or LSNF_SMALL_BATCH_AUTO
    if (rows >= 0 || rows == LSNF_SMALL_BATCH_AUTO) g_small_max.store(rows, std::memory_order_relaxed);
    return prev;
}
int lsnf_set_math_mode(int mode) {
    const int prev = math_mode();
    if (mode == LSNF_MATH_FP32 || mode == LSNF_MATH_BF16X3 || mode == LSNF_MATH_FP16X2 || mode == LSNF_MATH_BF16X3_PHASED)
        g_math.store(mode, std::memory_order_relaxed);
    return prev;
}
const char* lsnf_last_error(void) { return g_err; }

int lsnf_device_arch(int device, char* buf, size_t buflen) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n)
        return fail(LSNF_E_NODEVICE, "no HIP device %d (count %d)", device, n);
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceProperties");
    if (buf && buflen) { strncpy(buf, prop.gcnArchName, buflen - 1); buf[buflen - 1] = 0; }
    return LSNF_OK;
}

size_t lsnf_plan_floats(int nz, int width, int depth, int coupling) {
    LsnfGeo g;
    if (lsnf_geo_init(&g, nz, width, depth, coupling)) return 0;
    return g.total_floats;
}

size_t lsnf_prepare_scratch_bytes(int nz, int width, int depth) {
    (void)width;
    if (nz < 2 || nz > 128 || depth < 1 || depth > LSNF_MAX_DEPTH) return 0;
    return lsnf_prep_scratch_bytes(nz, depth);
}

int lsnf_prepare(const float* const* params_host, int nz, int width, int depth, int coupling, float* plan,
                 void* scratch, void* stream) {
    Check ck{"lsnf_prepare"};
    if (ck.geometry(nz, width, depth, coupling) || ck.required(params_host && plan && scratch) ||
        ck.aligned16("plan/scratch", {plan, scratch}) || ck.tables(params_host, nullptr, /*one_message=*/false))
        return ck.rc;
    LsnfPrepareCall c;
    c.g = ck.g; c.params_host = params_host; c.plan = plan; c.scratch = scratch; c.stream = (hipStream_t)stream;
    hipError_t e = lsnf_launch_prepare(c);
    if (e != hipSuccess) return hip_fail(e, "lsnf_prepare launch");
    return LSNF_OK;
}

size_t lsnf_actnorm_init_workspace_bytes(int nz, int width, int depth, int coupling, int B) {
    LsnfGeo g;
    if (lsnf_geo_init(&g, nz, width, depth, coupling) || B < 1 || B > (1 << 28)) return 0;
    return lsnf_init_workspace_bytes(g, B);
}

int lsnf_actnorm_init(float* const* params_host, int nz, int width, int depth, int coupling, int B, const float* z_in,
                      void* workspace, void* stream) {
    Check ck{"lsnf_actnorm_init"};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B, 1) || ck.required(params_host && z_in && workspace) ||
        ck.aligned16("workspace", {workspace}) || ck.aligned4("z_in", {z_in}) || ck.tables(params_host, nullptr, /*one_message=*/false))
        return ck.rc;
    LsnfInitCall c;
    c.g = ck.g; c.params_host = params_host; c.B = B; c.z_in = z_in; c.workspace = workspace; c.stream = (hipStream_t)stream;
    hipError_t e = lsnf_launch_actnorm_init(c);
    if (e != hipSuccess) return hip_fail(e, "lsnf_actnorm_init launch");
    return LSNF_OK;
}

constexpr unsigned kAdamFlags = LSNF_ADAM_AMSGRAD | LSNF_ADAM_DECOUPLED | LSNF_ADAM_MAXIMIZE | LSNF_ADAM_EMA | LSNF_ADAM_SKIP_NONFINITE;

size_t lsnf_adam_state_bytes(int nz, int width, int depth, int coupling) {
    return lsnf_adam_state_bytes_ex(nz, width, depth, coupling, 0);
}

size_t lsnf_adam_state_bytes_ex(int nz, int width, int depth, int coupling, unsigned flags) {
    LsnfGeo g;
    if (lsnf_geo_init(&g, nz, width, depth, coupling) || (flags & ~kAdamFlags)) return 0;
    return lsnf_adam_bytes(g, flags);
}

// the one body of lsnf_adam_step and lsnf_adam_step_ex; `who` names the entry point in the messages
static int adam_step(const char* who, float* const* params_host, const float* const* grads_host, int nz, int width, int depth,
                     int coupling, void* state, const LsnfAdamOptions& o, void* stream) {
    Check ck{who};
    auto finite_nonneg = [&](double v, const char* name) { return ck.refuse(!std::isfinite(v) || v < 0.0, "%s must be finite and >= 0", name); };
    auto unit = [](double v) { return v >= 0.0 && v < 1.0; };
    if (ck.geometry(nz, width, depth, coupling) || ck.refuse(o.flags & ~kAdamFlags, "unknown flag bits 0x%x", o.flags & ~kAdamFlags) ||
        ck.refuse((o.flags & LSNF_ADAM_EMA) && !unit(o.ema_decay), "ema_decay must lie in [0, 1)") ||
        ck.required(params_host && grads_host && state) || ck.aligned16("state", {state}) ||
        ck.aligned4("lr_dev / grad_norm_out", {o.lr_dev, o.grad_norm_out}) || finite_nonneg(o.lr, "lr") || finite_nonneg(o.eps, "eps") ||
        finite_nonneg(o.weight_decay, "weight_decay") || ck.refuse(!unit(o.beta1) || !unit(o.beta2), "betas must lie in [0, 1)") ||
        ck.refuse(std::isnan(o.max_norm), "max_norm is NaN") || ck.tables(params_host, grads_host, /*one_message=*/false))
        return ck.rc;
    LsnfAdamCall c;
    c.g = ck.g; c.params_host = params_host; c.grads_host = grads_host; c.state = state;
    c.lr = o.lr; c.beta1 = o.beta1; c.beta2 = o.beta2; c.eps = o.eps; c.weight_decay = o.weight_decay; c.max_norm = o.max_norm;
    c.ema_decay = (o.flags & LSNF_ADAM_EMA) ? o.ema_decay : 0.0; c.flags = o.flags;
    c.lr_dev = o.lr_dev; c.grad_norm_out = o.grad_norm_out; c.stream = (hipStream_t)stream;
    hipError_t e = lsnf_launch_adam(c);
    if (e != hipSuccess) return hip_fail(e, "lsnf_adam_step launch");
    return LSNF_OK;
}

int lsnf_adam_step(float* const* params_host, const float* const* grads_host, int nz, int width, int depth, int coupling,
                   void* state, double lr, const float* lr_dev, double beta1, double beta2, double eps, double weight_decay,
                   double max_norm, float* grad_norm_out, void* stream) {
    LsnfAdamOptions o;
    o.struct_bytes = sizeof(o); o.flags = 0; o.lr = lr; o.lr_dev = lr_dev; o.beta1 = beta1; o.beta2 = beta2; o.eps = eps;
    o.weight_decay = weight_decay; o.max_norm = max_norm; o.ema_decay = 0.0; o.grad_norm_out = grad_norm_out;
    return adam_step("lsnf_adam_step", params_host, grads_host, nz, width, depth, coupling, state, o, stream);
}

int lsnf_adam_step_ex(float* const* params_host, const float* const* grads_host, int nz, int width, int depth, int coupling,
                      void* state, const LsnfAdamOptions* options, void* stream) {
    if (!options) return fail(LSNF_E_ARG, "lsnf_adam_step_ex: NULL options");
    if (options->struct_bytes != sizeof(LsnfAdamOptions))
        return fail(LSNF_E_ARG, "lsnf_adam_step_ex: options->struct_bytes is %u, expected %u", options->struct_bytes,
                    (unsigned)sizeof(LsnfAdamOptions));
    return adam_step("lsnf_adam_step_ex", params_host, grads_host, nz, width, depth, coupling, state, *options, stream);
}

int lsnf_params_fast_path(void) { return l16_math() ? 1 : 0; }

int lsnf_forward(const float* plan, int nz, int width, int depth, int coupling, int first_block, int n_blocks, int B,
                 const float* z_in, const float* objective, float* z_out, float* logdet_out, float* ll_out,
                 float* z_saved, float* act_saved, float* params_workspace, double* stats, void* stream) {
    Check ck{"lsnf_forward"};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B)) return ck.rc;
    if (ck.empty) {
        if (stats && hipMemsetAsync(stats + 4, 0, 3 * sizeof(double), (hipStream_t)stream) != hipSuccess)
            return fail(LSNF_E_HIP, "lsnf_forward: hipMemsetAsync(stats) failed");
        return LSNF_OK;
    }
    if (ck.required(plan && z_in && z_out && logdet_out) ||
        ck.refuse(first_block < 0 || n_blocks < 1 || first_block + n_blocks > depth, "blocks [%d,%d) outside [0,%d)", first_block,
                  first_block + n_blocks, depth) ||
        ck.aligned16("plan", {plan}) || ck.aligned4("tensors", {z_in, z_out, logdet_out, objective, ll_out, z_saved}) ||
        ck.aligned16("act_saved", {act_saved}) || ck.refuse(!aligned8(stats), "stats must be 8-byte aligned"))
        return ck.rc;
    // h1 / h2 of every block into the parameter-gradient workspace (lsnf_backward_params' fast path)
    float* hdump = ck.params_workspace(params_workspace, first_block == 0 && n_blocks == depth && act_saved && (depth == 1 || z_saved),
                                       "the whole stack, act_saved and z_saved");
    if (ck.rc) return ck.rc;
    const LsnfGeo& g = ck.g;
    const int math = math_mode();
    // Calls without a stash that the software-pipelined forward covers cross over at 8 192 rows, not at the common threshold:
    // the latency kernel puts 16 / 32 rows on a workgroup up to 4 096 / 8 192 rows (one round of <= 256 workgroups that each
    // stream the weights once: 14.1 / 20.1 us), lsnf_fwd3q_kernel in its 16-rows-per-wave form takes 30.5 us up to 16 384 rows,
    // and a 64-row latency workgroup 32.6 us (tools/chk_small3_st.py, tools/shard_times.py, profiles/r03_shard_times.txt).
    // Only the AUTO threshold moves (an explicit setting is obeyed); calls that write a stash keep the common threshold, so that
    // the family that wrote it is the family that reads it.
    int small_max = small_batch_max();
    if (z_saved == nullptr && act_saved == nullptr && small_batch_setting() == LSNF_SMALL_BATCH_AUTO && small_max > 8192 &&
        math == LSNF_MATH_BF16X3 && g.HT == 2 && g.WT == 2)
        small_max = 8192;
    const int hdump_tiled = hdump && B >= LSNF_X3_MIN_ROWS && dump_may_tile(g, B, small_max) ? 1 : 0;
    if (ck.tiled_rows(hdump_tiled, "params_workspace", B, {z_in, z_out, z_saved}) ||
        ck.tag_workspace(params_workspace, B, hdump_tiled, (hipStream_t)stream))
        return ck.rc;
    LsnfForwardCall c;
    ck.head(c, plan, B, stream, {z_in, z_out, z_saved});
    c.first_block = first_block; c.n_blocks = n_blocks;
    c.z_in = z_in; c.objective = objective; c.z_out = z_out; c.logdet_out = logdet_out; c.ll_out = ll_out;
    c.z_saved = z_saved; c.act_saved = act_saved; c.stats = stats; c.hdump = hdump; c.hdump_tiled = hdump_tiled;
    const Pick p = select_forward(c, small_max);
    return report(ck.entry, p, launch_forward(p, c));
}

size_t lsnf_act_saved_floats(int nz, int width, int depth, int B) {
    LsnfGeo g;
    if (lsnf_geo_init(&g, nz, width, depth, 1) || B < 0) return 0;   // independent of the coupling type
    return (size_t)depth * lsnf_act_layout(B, g.HT, g.WT).per_block;
}

int lsnf_restash(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_out,
                 const float* z_saved, float* act_saved, void* stream) {
    Check ck{"lsnf_restash"};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B)) return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (ck.required(plan && z_out && act_saved && (depth == 1 || z_saved)) || ck.aligned16("plan / act_saved", {plan, act_saved}) ||
        ck.aligned4("tensors", {z_out, z_saved}) ||
        ck.refuse(!l16_math(), "needs a bf16x3-family math mode (lsnf_params_fast_path() == 1)"))
        return ck.rc;
    LsnfRestashCall c;
    ck.head(c, plan, B, stream, {z_out, z_saved});
    c.z_out = z_out; c.z_saved = z_saved; c.act_saved = act_saved;
    const hipError_t e = lsnf_launch_small3_restash(c);
    if (e != hipSuccess) return hip_fail(e, "lsnf_restash launch");
    return LSNF_OK;
}

int lsnf_reverse(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_in,
                 const float* objective, float* z_out, float* objective_out, void* stream) {
    return reverse_entry("lsnf_reverse", /*keep=*/false, plan, nz, width, depth, coupling, B, z_in, objective, z_out, objective_out,
                         nullptr, nullptr, nullptr, stream);
}

int lsnf_sample(const float* plan, int nz, int width, int depth, int coupling, int B, const LsnfRng* rng, float temperature,
                float* z_out, float* objective_out, float* eps_out, float* ll_out, void* stream) {
    return sample_entry("lsnf_sample", /*keep=*/false, plan, nz, width, depth, coupling, B, rng, temperature, z_out, objective_out, eps_out,
                        ll_out, nullptr, nullptr, nullptr, stream);
}

int lsnf_reverse_keep_covers(int nz, int width, int depth, int coupling, int B) {
    LsnfReverseCall c;
    if (lsnf_geo_init(&c.g, nz, width, depth, coupling) || B < 0 || B > (1 << 28)) return 0;
    c.B = B;
    return reverse_keep_covers(c) ? 1 : 0;
}

int lsnf_reverse_keep(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_in,
                      const float* objective, float* z_out, float* objective_out, float* z_saved, float* act_saved,
                      float* params_workspace, void* stream) {
    return reverse_entry("lsnf_reverse_keep", /*keep=*/true, plan, nz, width, depth, coupling, B, z_in, objective, z_out, objective_out,
                         z_saved, act_saved, params_workspace, stream);
}

int lsnf_sample_keep(const float* plan, int nz, int width, int depth, int coupling, int B, const LsnfRng* rng, float temperature,
                     float* z_out, float* objective_out, float* eps_out, float* ll_out, float* z_saved, float* act_saved,
                     float* params_workspace, void* stream) {
    return sample_entry("lsnf_sample_keep", /*keep=*/true, plan, nz, width, depth, coupling, B, rng, temperature, z_out, objective_out,
                        eps_out, ll_out, z_saved, act_saved, params_workspace, stream);
}

int lsnf_backward_z(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_out,
                    const float* z_saved, const float* act_saved, const float* g_z1, const float* g_logdet, int ll_mode,
                    float ll_scale, float* g_z_in, void* stream) {
    Check ck{"lsnf_backward_z"};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B)) return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (ck.required(plan && z_out && g_z_in && (depth == 1 || z_saved)) || ck.aligned16("plan", {plan}) ||
        ck.aligned4("tensors", {z_out, z_saved, g_z1, g_logdet, g_z_in}) || ck.aligned16("act_saved", {act_saved}))
        return ck.rc;
    LsnfBackwardCall c;
    ck.head(c, plan, B, stream, {z_out, g_z_in, z_saved, g_z1});
    c.z_out = z_out; c.z_saved = z_saved; c.act_saved = act_saved; c.g_z1 = g_z1; c.g_logdet = g_logdet;
    c.ll_mode = ll_mode; c.ll_scale = ll_scale; c.g_z_in = g_z_in;
    return backward_launch(ck.entry, c);
}

int lsnf_reverse_backward_z(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_out,
                            const float* z_saved, const float* act_saved, const float* g_x, const float* g_objective,
                            float* g_z_in, void* stream) {
    Check ck{"lsnf_reverse_backward_z"};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B)) return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (ck.required(plan && z_out && g_z_in && (depth == 1 || z_saved)) ||
        ck.refuse(!act_saved, "act_saved is required (lsnf_forward's stash, or lsnf_restash)") || ck.aligned16("plan", {plan}) ||
        ck.aligned16("act_saved", {act_saved}) || ck.aligned4("tensors", {z_out, z_saved, g_x, g_objective, g_z_in}))
        return ck.rc;
    LsnfReverseBackwardCall c;
    ck.head(c, plan, B, stream, {z_out, g_z_in, z_saved, g_x});
    c.z_out = z_out; c.z_saved = z_saved; c.act_saved = act_saved; c.g_x = g_x; c.g_objective = g_objective; c.g_z_in = g_z_in;
    const Pick p = select_reverse_backward(c);
    return report(ck.entry, p, lsnf_launch_small3_reverse_backward_z(c, p.st));
}

int lsnf_reverse_langevin_step(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_out,
                               const float* z_saved, const float* act_saved, const float* grad_g, const float* noise,
                               const LsnfRng* rng, float step_size, float* eps_new, float* g_eps_out, float* g_norm, float* eps_norm,
                               void* stream) {
    Check ck{"lsnf_reverse_langevin_step"};
    // eps_new may be z_out (every read of a workgroup's rows precedes its stores), g_eps_out may be grad_g (read first, as g_z_in / g_x
    // of lsnf_reverse_backward_z); nothing else the kernel reads may be what it writes, and no two outputs may be one tensor
    auto norm_aliases = [&](const float* nrm) {
        return nrm && (nrm == z_out || nrm == z_saved || nrm == grad_g || nrm == noise || nrm == eps_new || nrm == g_eps_out || g_norm == eps_norm);
    };
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || ck.rng(noise, rng, /*row0_first=*/false) ||
        ck.refuse(!std::isfinite(step_size), "step_size must be finite (got %g)", (double)step_size) ||
        ck.refuse(eps_new && (eps_new == grad_g || eps_new == noise || eps_new == z_saved || eps_new == g_eps_out),
                  "eps_new must not alias grad_g, noise, z_saved or g_eps_out") ||
        ck.refuse(g_eps_out && (g_eps_out == noise || g_eps_out == z_out || g_eps_out == z_saved),
                  "g_eps_out must not alias noise, z_out or z_saved") ||
        ck.refuse(norm_aliases(g_norm) || norm_aliases(eps_norm), "g_norm / eps_norm must not alias another tensor of the call"))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (ck.required(plan && z_out && eps_new && (depth == 1 || z_saved)) ||
        ck.refuse(!act_saved, "act_saved is required (the stash of lsnf_forward, lsnf_restash or lsnf_reverse_keep)") ||
        ck.aligned16("plan", {plan}) || ck.aligned16("act_saved", {act_saved}) ||
        ck.aligned4("tensors", {z_out, z_saved, grad_g, noise, eps_new, g_eps_out, g_norm, eps_norm}))
        return ck.rc;
    LsnfReverseLangevinCall c;           // (no g_x / g_objective: the upstream gradient is grad_g)
    ck.head(c, plan, B, stream, {z_out, z_saved, grad_g, noise, eps_new, g_eps_out});
    c.z_out = z_out; c.z_saved = z_saved; c.act_saved = act_saved; c.g_z_in = g_eps_out;
    c.grad_g = grad_g; c.noise = noise; c.step = step_size; c.eps_new = eps_new; c.g_norm = g_norm; c.eps_norm = eps_norm;
    c.rng = rng_args(rng);
    const Pick p = select_reverse_langevin(c);
    return report(ck.entry, p, lsnf_launch_small3_reverse_langevin(c, p.st));
}

int lsnf_langevin_step(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_cur,
                       const float* z_out, const float* z_saved, const float* act_saved, const float* grad_g,
                       const float* noise, const LsnfRng* rng, float step_size, float* z_new, float* gf_norm, float* gg_norm, void* stream) {
    Check ck{"lsnf_langevin_step"};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B)) return ck.rc;
    if (ck.empty) return LSNF_OK;        // (before the rng rules, unlike lsnf_reverse_langevin_step and lsnf_sample)
    if (ck.required(plan && z_cur && z_out && z_new && (depth == 1 || z_saved)) || ck.aligned16("plan", {plan}) ||
        ck.aligned4("tensors", {z_cur, z_out, z_saved, grad_g, noise, z_new, gf_norm, gg_norm}) || ck.aligned16("act_saved", {act_saved}) ||
        ck.rng(noise, rng, /*row0_first=*/false))
        return ck.rc;
    const LsnfLangevinArgs lv = {z_cur, grad_g, noise, z_new, gf_norm, gg_norm, step_size, rng_args(rng)};
    LsnfBackwardCall c;                  // (no g_z1 / g_logdet / g_z_in: the gradient of -log p, consumed by the update)
    ck.head(c, plan, B, stream, {z_out, z_saved, z_cur, grad_g, noise, z_new});
    c.z_out = z_out; c.z_saved = z_saved; c.act_saved = act_saved; c.ll_mode = 1; c.ll_scale = -1.0f; c.lv = &lv;
    return backward_launch(ck.entry, c);
}

int lsnf_mala_step(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_prop, const float* z_out,
                   const float* z_saved, const float* act_saved, const float* ll_prop, const float* grad_g, const float* energy_g,
                   float* z_acc, float* grad_acc, float* u_acc, const float* noise, const float* uniform, const LsnfRng* rng,
                   float step_size, unsigned flags, float* z_next, float* accept_out, float* log_alpha_out, void* stream) {
    Check ck{"lsnf_mala_step"};
    const Named reads[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"z_saved", z_saved}, {"act_saved", act_saved},
                           {"ll_prop", ll_prop}, {"grad_g", grad_g}, {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform}};
    const Named writes[] = {{"z_acc", z_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"z_next", z_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}};
    const Needed needed[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"act_saved", act_saved}, {"ll_prop", ll_prop},
                             {"z_acc", z_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed, LSNF_MALA_INIT, (flags & LSNF_MALA_INIT) != 0,
                         /*inner=*/false, "LSNF_MALA_INIT", plan, act_saved, noise, uniform, rng, step_size, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.aliases(ck)) return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck)) return ck.rc;
    const LsnfLangevinArgs lv = {z_prop, grad_g, noise, z_next, nullptr, nullptr, step_size, rng_args(rng)};
    LsnfMalaCall c;                      // (no g_z1 / g_logdet / g_z_in: the gradient of -log p at the proposal, consumed by the tail)
    ck.head(c, plan, B, stream, {z_prop, z_out, z_saved, grad_g, noise, z_next, z_acc, grad_acc});
    c.z_out = z_out; c.z_saved = z_saved; c.act_saved = act_saved; c.ll_mode = 1; c.ll_scale = -1.0f; c.lv = &lv; c.ll_prop = ll_prop;
    c.chain = {energy_g, uniform, z_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags};
    const Pick p = select_mala(c);
    return report(ck.entry, p, lsnf_launch_small3_mala(c, p.st));
}

int lsnf_reverse_mala_step(const float* plan, int nz, int width, int depth, int coupling, int B, const float* eps_prop,
                           const float* z_saved, const float* act_saved, const float* grad_g, const float* energy_g, float* eps_acc,
                           float* grad_acc, float* u_acc, const float* noise, const float* uniform, const LsnfRng* rng, float step_size,
                           unsigned flags, float* eps_next, float* accept_out, float* log_alpha_out, void* stream) {
    Check ck{"lsnf_reverse_mala_step"};
    const Named reads[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"z_saved", z_saved}, {"act_saved", act_saved}, {"grad_g", grad_g},
                           {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform}};
    const Named writes[] = {{"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"eps_next", eps_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}};
    const Needed needed[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc},
                             {"act_saved", act_saved, true, "(the stash of lsnf_forward, lsnf_restash or lsnf_reverse_keep)"},
                             {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed, LSNF_MALA_INIT, (flags & LSNF_MALA_INIT) != 0,
                         /*inner=*/false, "LSNF_MALA_INIT", plan, act_saved, noise, uniform, rng, step_size, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.aliases(ck)) return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck)) return ck.rc;
    LsnfReverseMalaCall c;               // (no g_x / g_objective / g_z_in: the gradient at the proposal is consumed by the tail)
    ck.head(c, plan, B, stream, {eps_prop, z_saved, grad_g, noise, eps_next, eps_acc, grad_acc});
    c.z_out = eps_prop; c.z_saved = z_saved; c.act_saved = act_saved;
    c.grad_g = grad_g; c.noise = noise; c.step = step_size; c.eps_new = eps_next; c.rng = rng_args(rng);
    c.chain = {energy_g, uniform, eps_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags};
    const Pick p = select_reverse_mala(c);
    return report(ck.entry, p, lsnf_launch_small3_reverse_mala(c, p.st));
}

int lsnf_hmc_step(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_prop, const float* z_out,
                  const float* z_saved, const float* act_saved, const float* ll_prop, const float* grad_g, const float* energy_g,
                  float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                  const LsnfRng* rng, float step_size, unsigned flags, float* z_next, float* accept_out, float* log_alpha_out, void* stream) {
    Check ck{"lsnf_hmc_step"};
    const Named reads[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"z_saved", z_saved}, {"act_saved", act_saved},
                           {"ll_prop", ll_prop}, {"grad_g", grad_g}, {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform}};
    // (mom is read and written by the same call: it is listed with the outputs, so it may be neither another input nor another output)
    const Named writes[] = {{"z_acc", z_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"z_next", z_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"act_saved", act_saved}, {"z_acc", z_acc},
                             {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"mom", mom}, {"kin0", kin0},
                             {"ll_prop", ll_prop, !inner, "(NULL) unless LSNF_HMC_INNER"}, {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"},
                             {"z_next", z_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed, LSNF_HMC_INIT | LSNF_HMC_INNER, init, inner,
                         "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, step_size, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck)) return ck.rc;
    const LsnfLangevinArgs lv = {z_prop, grad_g, noise, z_next, nullptr, nullptr, step_size, rng_args(rng)};
    LsnfHmcCall c;                       // (no g_z1 / g_logdet / g_z_in: the gradient of -log p at the point, consumed by the tail)
    ck.head(c, plan, B, stream, {z_prop, z_out, z_saved, grad_g, noise, z_next, z_acc, grad_acc, mom});
    c.z_out = z_out; c.z_saved = z_saved; c.act_saved = act_saved; c.ll_mode = 1; c.ll_scale = -1.0f; c.lv = &lv; c.ll_prop = ll_prop;
    c.chain = {energy_g, uniform, z_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    const Pick p = select_hmc(c);
    return report(ck.entry, p, lsnf_launch_small3_hmc(c, p.st));
}

int lsnf_reverse_hmc_step(const float* plan, int nz, int width, int depth, int coupling, int B, const float* eps_prop,
                          const float* z_saved, const float* act_saved, const float* grad_g, const float* energy_g, float* eps_acc,
                          float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                          const LsnfRng* rng, float step_size, unsigned flags, float* eps_next, float* accept_out, float* log_alpha_out,
                          void* stream) {
    Check ck{"lsnf_reverse_hmc_step"};
    const Named reads[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"z_saved", z_saved}, {"act_saved", act_saved}, {"grad_g", grad_g},
                           {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform}};
    // (mom is read and written by the same call: it is listed with the outputs, so it may be neither another input nor another output)
    const Named writes[] = {{"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"eps_next", eps_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc},
                             {"mom", mom}, {"kin0", kin0},
                             {"act_saved", act_saved, true, "(the stash of lsnf_forward, lsnf_restash or lsnf_reverse_keep)"},
                             {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"}, {"eps_next", eps_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed, LSNF_HMC_INIT | LSNF_HMC_INNER, init, inner,
                         "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, step_size, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck)) return ck.rc;
    LsnfReverseHmcCall c;                // (no g_x / g_objective / g_z_in: the gradient at the point is consumed by the tail)
    ck.head(c, plan, B, stream, {eps_prop, z_saved, grad_g, noise, eps_next, eps_acc, grad_acc, mom});
    c.z_out = eps_prop; c.z_saved = z_saved; c.act_saved = act_saved;
    c.grad_g = grad_g; c.noise = noise; c.step = step_size; c.eps_new = eps_next; c.rng = rng_args(rng);
    c.chain = {energy_g, uniform, eps_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    const Pick p = select_reverse_hmc(c);
    return report(ck.entry, p, lsnf_launch_small3_reverse_hmc(c, p.st));
}

// The two HMC entries with a step per row: the scalar entries' tables and rules, step_rows and adapt among the outputs (so that they
// alias nothing else of the call), no step_size rule (the steps are device memory), the flags and LsnfDualAvg rules of RowSteps.
int lsnf_hmc_step_rows(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_prop, const float* z_out,
                       const float* z_saved, const float* act_saved, const float* ll_prop, const float* grad_g, const float* energy_g,
                       float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                       const LsnfRng* rng, float* step_rows, float* adapt, const LsnfDualAvg* da, unsigned flags, float* z_next,
                       float* accept_out, float* log_alpha_out, void* stream) {
    Check ck{"lsnf_hmc_step_rows"};
    const Named reads[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"z_saved", z_saved}, {"act_saved", act_saved},
                           {"ll_prop", ll_prop}, {"grad_g", grad_g}, {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform}};
    const Named writes[] = {{"z_acc", z_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"z_next", z_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"adapt", adapt}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"act_saved", act_saved}, {"z_acc", z_acc},
                             {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows},
                             {"ll_prop", ll_prop, !inner, "(NULL) unless LSNF_HMC_INNER"}, {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"},
                             {"z_next", z_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed,
                         LSNF_HMC_INIT | LSNF_HMC_INNER | LSNF_HMC_ADAPT | LSNF_HMC_ADAPT_LAST, init, inner,
                         "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, /*step_size=*/1.0f, flags};
    const RowSteps rows = {step_rows, adapt, da, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || rows.scalars(ck) ||
        s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck) || rows.pointers(ck)) return ck.rc;
    const LsnfLangevinArgs lv = {z_prop, grad_g, noise, z_next, nullptr, nullptr, 0.0f, rng_args(rng)};
    LsnfHmcRowsCall c;                   // (no g_z1 / g_logdet / g_z_in: the gradient of -log p at the point, consumed by the tail)
    ck.head(c, plan, B, stream, {z_prop, z_out, z_saved, grad_g, noise, z_next, z_acc, grad_acc, mom});
    c.z_out = z_out; c.z_saved = z_saved; c.act_saved = act_saved; c.ll_mode = 1; c.ll_scale = -1.0f; c.lv = &lv; c.ll_prop = ll_prop;
    c.chain = {energy_g, uniform, z_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    c.step_rows = step_rows; c.adapt = adapt; c.da = rows.args();
    const Pick p = select_hmc_rows(c);
    return report(ck.entry, p, lsnf_launch_small3_hmc_rows(c, p.st));
}

int lsnf_reverse_hmc_step_rows(const float* plan, int nz, int width, int depth, int coupling, int B, const float* eps_prop,
                               const float* z_saved, const float* act_saved, const float* grad_g, const float* energy_g, float* eps_acc,
                               float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                               const LsnfRng* rng, float* step_rows, float* adapt, const LsnfDualAvg* da, unsigned flags, float* eps_next,
                               float* accept_out, float* log_alpha_out, void* stream) {
    Check ck{"lsnf_reverse_hmc_step_rows"};
    const Named reads[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"z_saved", z_saved}, {"act_saved", act_saved}, {"grad_g", grad_g},
                           {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform}};
    const Named writes[] = {{"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"eps_next", eps_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"adapt", adapt}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc},
                             {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows},
                             {"act_saved", act_saved, true, "(the stash of lsnf_forward, lsnf_restash or lsnf_reverse_keep)"},
                             {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"}, {"eps_next", eps_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed,
                         LSNF_HMC_INIT | LSNF_HMC_INNER | LSNF_HMC_ADAPT | LSNF_HMC_ADAPT_LAST, init, inner,
                         "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, /*step_size=*/1.0f, flags};
    const RowSteps rows = {step_rows, adapt, da, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || rows.scalars(ck) ||
        s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck) || rows.pointers(ck)) return ck.rc;
    LsnfReverseHmcRowsCall c;            // (no g_x / g_objective / g_z_in: the gradient at the point is consumed by the tail)
    ck.head(c, plan, B, stream, {eps_prop, z_saved, grad_g, noise, eps_next, eps_acc, grad_acc, mom});
    c.z_out = eps_prop; c.z_saved = z_saved; c.act_saved = act_saved;
    c.grad_g = grad_g; c.noise = noise; c.step = 0.0f; c.eps_new = eps_next; c.rng = rng_args(rng);
    c.chain = {energy_g, uniform, eps_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    c.step_rows = step_rows; c.adapt = adapt; c.da = rows.args();
    const Pick p = select_reverse_hmc_rows(c);
    return report(ck.entry, p, lsnf_launch_small3_reverse_hmc_rows(c, p.st));
}

// The two HMC entries with a metric per row: the per-row entries' tables and rules, the scales and the window's accumulators among the
// outputs (so that they alias nothing else of the call) and among the row tensors that decide the row-access width, RowMetric's rules
// after RowSteps'.
int lsnf_hmc_step_metric(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_prop, const float* z_out,
                         const float* z_saved, const float* act_saved, const float* ll_prop, const float* grad_g, const float* energy_g,
                         float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                         const LsnfRng* rng, float* step_rows, float* adapt, const LsnfDualAvg* da, float* scale_rows, float* mean_rows,
                         float* m2_rows, float* count_rows, const LsnfMetricReg* reg, unsigned flags, float* z_next, float* accept_out,
                         float* log_alpha_out, void* stream) {
    Check ck{"lsnf_hmc_step_metric"};
    const Named reads[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"z_saved", z_saved}, {"act_saved", act_saved},
                           {"ll_prop", ll_prop}, {"grad_g", grad_g}, {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform}};
    const Named writes[] = {{"z_acc", z_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"z_next", z_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"adapt", adapt},
                            {"scale_rows", scale_rows}, {"mean_rows", mean_rows}, {"m2_rows", m2_rows}, {"count_rows", count_rows}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"act_saved", act_saved}, {"z_acc", z_acc},
                             {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows},
                             {"scale_rows", scale_rows},
                             {"ll_prop", ll_prop, !inner, "(NULL) unless LSNF_HMC_INNER"}, {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"},
                             {"z_next", z_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed,
                         LSNF_HMC_INIT | LSNF_HMC_INNER | LSNF_HMC_ADAPT | LSNF_HMC_ADAPT_LAST | LSNF_HMC_METRIC_FOLD | LSNF_HMC_METRIC_CLOSE,
                         init, inner, "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, /*step_size=*/1.0f, flags};
    const RowSteps rows = {step_rows, adapt, da, flags};
    const RowMetric metric = {mean_rows, m2_rows, count_rows, reg, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || rows.scalars(ck) ||
        metric.scalars(ck) || s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck) || rows.pointers(ck) || metric.pointers(ck)) return ck.rc;
    const LsnfLangevinArgs lv = {z_prop, grad_g, noise, z_next, nullptr, nullptr, 0.0f, rng_args(rng)};
    LsnfHmcMetricCall c;                 // (no g_z1 / g_logdet / g_z_in: the gradient of -log p at the point, consumed by the tail)
    ck.head(c, plan, B, stream, {z_prop, z_out, z_saved, grad_g, noise, z_next, z_acc, grad_acc, mom, scale_rows, mean_rows, m2_rows});
    c.z_out = z_out; c.z_saved = z_saved; c.act_saved = act_saved; c.ll_mode = 1; c.ll_scale = -1.0f; c.lv = &lv; c.ll_prop = ll_prop;
    c.chain = {energy_g, uniform, z_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    c.step_rows = step_rows; c.adapt = adapt; c.da = rows.args();
    c.scale = scale_rows; c.mean = mean_rows; c.m2 = m2_rows; c.count = count_rows; c.reg = metric.args();
    const Pick p = select_hmc_metric(c);
    return report(ck.entry, p, lsnf_launch_small3_hmc_metric(c, p.st));
}

int lsnf_reverse_hmc_step_metric(const float* plan, int nz, int width, int depth, int coupling, int B, const float* eps_prop,
                                 const float* z_saved, const float* act_saved, const float* grad_g, const float* energy_g, float* eps_acc,
                                 float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                                 const LsnfRng* rng, float* step_rows, float* adapt, const LsnfDualAvg* da, float* scale_rows,
                                 float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg, unsigned flags,
                                 float* eps_next, float* accept_out, float* log_alpha_out, void* stream) {
    Check ck{"lsnf_reverse_hmc_step_metric"};
    const Named reads[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"z_saved", z_saved}, {"act_saved", act_saved}, {"grad_g", grad_g},
                           {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform}};
    const Named writes[] = {{"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"eps_next", eps_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"adapt", adapt},
                            {"scale_rows", scale_rows}, {"mean_rows", mean_rows}, {"m2_rows", m2_rows}, {"count_rows", count_rows}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc},
                             {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"scale_rows", scale_rows},
                             {"act_saved", act_saved, true, "(the stash of lsnf_forward, lsnf_restash or lsnf_reverse_keep)"},
                             {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"}, {"eps_next", eps_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed,
                         LSNF_HMC_INIT | LSNF_HMC_INNER | LSNF_HMC_ADAPT | LSNF_HMC_ADAPT_LAST | LSNF_HMC_METRIC_FOLD | LSNF_HMC_METRIC_CLOSE,
                         init, inner, "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, /*step_size=*/1.0f, flags};
    const RowSteps rows = {step_rows, adapt, da, flags};
    const RowMetric metric = {mean_rows, m2_rows, count_rows, reg, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || rows.scalars(ck) ||
        metric.scalars(ck) || s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck) || rows.pointers(ck) || metric.pointers(ck)) return ck.rc;
    LsnfReverseHmcMetricCall c;          // (no g_x / g_objective / g_z_in: the gradient at the point is consumed by the tail)
    ck.head(c, plan, B, stream, {eps_prop, z_saved, grad_g, noise, eps_next, eps_acc, grad_acc, mom, scale_rows, mean_rows, m2_rows});
    c.z_out = eps_prop; c.z_saved = z_saved; c.act_saved = act_saved;
    c.grad_g = grad_g; c.noise = noise; c.step = 0.0f; c.eps_new = eps_next; c.rng = rng_args(rng);
    c.chain = {energy_g, uniform, eps_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    c.step_rows = step_rows; c.adapt = adapt; c.da = rows.args();
    c.scale = scale_rows; c.mean = mean_rows; c.m2 = m2_rows; c.count = count_rows; c.reg = metric.args();
    const Pick p = select_reverse_hmc_metric(c);
    return report(ck.entry, p, lsnf_launch_small3_reverse_hmc_metric(c, p.st));
}

// The two HMC entries with a likelihood temperature per row: the metric entries' tables and rules, the five arrays of the temperature
// among the outputs (so that they alias nothing else of the call), like_grad_acc among the row tensors that decide the row-access
// width, RowTemper's rules after RowMetric's.
int lsnf_hmc_step_tempered(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_prop, const float* z_out,
                           const float* z_saved, const float* act_saved, const float* ll_prop, const float* grad_g, const float* energy_g,
                           float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                           const LsnfRng* rng, float* step_rows, float* adapt, const LsnfDualAvg* da, float* scale_rows, float* mean_rows,
                           float* m2_rows, float* count_rows, const LsnfMetricReg* reg, float* beta_rows, const float* beta_next,
                           float* like_grad_acc, float* like_u_acc, float* log_w, unsigned flags, float* z_next, float* accept_out,
                           float* log_alpha_out, void* stream) {
    Check ck{"lsnf_hmc_step_tempered"};
    const Named reads[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"z_saved", z_saved}, {"act_saved", act_saved},
                           {"ll_prop", ll_prop}, {"grad_g", grad_g}, {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform}};
    const Named writes[] = {{"z_acc", z_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"z_next", z_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"adapt", adapt},
                            {"scale_rows", scale_rows}, {"mean_rows", mean_rows}, {"m2_rows", m2_rows}, {"count_rows", count_rows},
                            {"beta_rows", beta_rows}, {"beta_next", beta_next}, {"like_grad_acc", like_grad_acc},
                            {"like_u_acc", like_u_acc}, {"log_w", log_w}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"act_saved", act_saved}, {"z_acc", z_acc},
                             {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows},
                             {"scale_rows", scale_rows}, {"beta_rows", beta_rows}, {"like_grad_acc", like_grad_acc},
                             {"like_u_acc", like_u_acc},
                             {"ll_prop", ll_prop, !inner, "(NULL) unless LSNF_HMC_INNER"}, {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"},
                             {"z_next", z_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed,
                         LSNF_HMC_INIT | LSNF_HMC_INNER | LSNF_HMC_ADAPT | LSNF_HMC_ADAPT_LAST | LSNF_HMC_METRIC_FOLD | LSNF_HMC_METRIC_CLOSE |
                             LSNF_HMC_ANNEAL,
                         init, inner, "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, /*step_size=*/1.0f, flags};
    const RowSteps rows = {step_rows, adapt, da, flags};
    const RowMetric metric = {mean_rows, m2_rows, count_rows, reg, flags};
    const RowTemper temper = {beta_next, log_w, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || rows.scalars(ck) ||
        metric.scalars(ck) || temper.scalars(ck) || s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck) || rows.pointers(ck) || metric.pointers(ck) || temper.pointers(ck)) return ck.rc;
    const LsnfLangevinArgs lv = {z_prop, grad_g, noise, z_next, nullptr, nullptr, 0.0f, rng_args(rng)};
    LsnfHmcTemperedCall c;               // (no g_z1 / g_logdet / g_z_in: the gradient of -log p at the point, consumed by the tail)
    ck.head(c, plan, B, stream, {z_prop, z_out, z_saved, grad_g, noise, z_next, z_acc, grad_acc, mom, scale_rows, mean_rows, m2_rows, like_grad_acc});
    c.z_out = z_out; c.z_saved = z_saved; c.act_saved = act_saved; c.ll_mode = 1; c.ll_scale = -1.0f; c.lv = &lv; c.ll_prop = ll_prop;
    c.chain = {energy_g, uniform, z_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    c.step_rows = step_rows; c.adapt = adapt; c.da = rows.args();
    c.scale = scale_rows; c.mean = mean_rows; c.m2 = m2_rows; c.count = count_rows; c.reg = metric.args();
    c.beta_rows = beta_rows; c.beta_next = beta_next; c.like_grad_acc = like_grad_acc; c.like_u_acc = like_u_acc; c.log_w = log_w;
    const Pick p = select_hmc_tempered(c);
    return report(ck.entry, p, lsnf_launch_small3_hmc_tempered(c, p.st));
}

int lsnf_reverse_hmc_step_tempered(const float* plan, int nz, int width, int depth, int coupling, int B, const float* eps_prop,
                                   const float* z_saved, const float* act_saved, const float* grad_g, const float* energy_g, float* eps_acc,
                                   float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                                   const LsnfRng* rng, float* step_rows, float* adapt, const LsnfDualAvg* da, float* scale_rows,
                                   float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg, float* beta_rows,
                                   const float* beta_next, float* like_grad_acc, float* like_u_acc, float* log_w, unsigned flags,
                                   float* eps_next, float* accept_out, float* log_alpha_out, void* stream) {
    Check ck{"lsnf_reverse_hmc_step_tempered"};
    const Named reads[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"z_saved", z_saved}, {"act_saved", act_saved}, {"grad_g", grad_g},
                           {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform}};
    const Named writes[] = {{"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"eps_next", eps_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"adapt", adapt},
                            {"scale_rows", scale_rows}, {"mean_rows", mean_rows}, {"m2_rows", m2_rows}, {"count_rows", count_rows},
                            {"beta_rows", beta_rows}, {"beta_next", beta_next}, {"like_grad_acc", like_grad_acc},
                            {"like_u_acc", like_u_acc}, {"log_w", log_w}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc},
                             {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"scale_rows", scale_rows}, {"beta_rows", beta_rows},
                             {"like_grad_acc", like_grad_acc}, {"like_u_acc", like_u_acc},
                             {"act_saved", act_saved, true, "(the stash of lsnf_forward, lsnf_restash or lsnf_reverse_keep)"},
                             {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"}, {"eps_next", eps_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed,
                         LSNF_HMC_INIT | LSNF_HMC_INNER | LSNF_HMC_ADAPT | LSNF_HMC_ADAPT_LAST | LSNF_HMC_METRIC_FOLD | LSNF_HMC_METRIC_CLOSE |
                             LSNF_HMC_ANNEAL,
                         init, inner, "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, /*step_size=*/1.0f, flags};
    const RowSteps rows = {step_rows, adapt, da, flags};
    const RowMetric metric = {mean_rows, m2_rows, count_rows, reg, flags};
    const RowTemper temper = {beta_next, log_w, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || rows.scalars(ck) ||
        metric.scalars(ck) || temper.scalars(ck) || s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck) || rows.pointers(ck) || metric.pointers(ck) || temper.pointers(ck)) return ck.rc;
    LsnfReverseHmcTemperedCall c;        // (no g_x / g_objective / g_z_in: the gradient at the point is consumed by the tail)
    ck.head(c, plan, B, stream, {eps_prop, z_saved, grad_g, noise, eps_next, eps_acc, grad_acc, mom, scale_rows, mean_rows, m2_rows, like_grad_acc});
    c.z_out = eps_prop; c.z_saved = z_saved; c.act_saved = act_saved;
    c.grad_g = grad_g; c.noise = noise; c.step = 0.0f; c.eps_new = eps_next; c.rng = rng_args(rng);
    c.chain = {energy_g, uniform, eps_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    c.step_rows = step_rows; c.adapt = adapt; c.da = rows.args();
    c.scale = scale_rows; c.mean = mean_rows; c.m2 = m2_rows; c.count = count_rows; c.reg = metric.args();
    c.beta_rows = beta_rows; c.beta_next = beta_next; c.like_grad_acc = like_grad_acc; c.like_u_acc = like_u_acc; c.log_w = log_w;
    const Pick p = select_reverse_hmc_tempered(c);
    return report(ck.entry, p, lsnf_launch_small3_reverse_hmc_tempered(c, p.st));
}

// The two HMC entries with a replica-exchange move: the tempered entries' tables and rules, swap_uniform among the reads, swap_out and
// log_swap_out among the outputs, RowExchange's rules after RowTemper's.
int lsnf_hmc_step_exchange(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_prop, const float* z_out,
                           const float* z_saved, const float* act_saved, const float* ll_prop, const float* grad_g, const float* energy_g,
                           float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                           const LsnfRng* rng, float* step_rows, float* adapt, const LsnfDualAvg* da, float* scale_rows, float* mean_rows,
                           float* m2_rows, float* count_rows, const LsnfMetricReg* reg, float* beta_rows, const float* beta_next,
                           float* like_grad_acc, float* like_u_acc, float* log_w, unsigned flags, float* z_next, float* accept_out,
                           float* log_alpha_out, int ladder, const float* swap_uniform, float* swap_out, float* log_swap_out, void* stream) {
    Check ck{"lsnf_hmc_step_exchange"};
    const Named reads[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"z_saved", z_saved}, {"act_saved", act_saved},
                           {"ll_prop", ll_prop}, {"grad_g", grad_g}, {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform},
                           {"swap_uniform", swap_uniform}};
    const Named writes[] = {{"z_acc", z_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"z_next", z_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"adapt", adapt},
                            {"scale_rows", scale_rows}, {"mean_rows", mean_rows}, {"m2_rows", m2_rows}, {"count_rows", count_rows},
                            {"beta_rows", beta_rows}, {"beta_next", beta_next}, {"like_grad_acc", like_grad_acc},
                            {"like_u_acc", like_u_acc}, {"log_w", log_w}, {"swap_out", swap_out}, {"log_swap_out", log_swap_out}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"act_saved", act_saved}, {"z_acc", z_acc},
                             {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows},
                             {"scale_rows", scale_rows}, {"beta_rows", beta_rows}, {"like_grad_acc", like_grad_acc},
                             {"like_u_acc", like_u_acc},
                             {"ll_prop", ll_prop, !inner, "(NULL) unless LSNF_HMC_INNER"}, {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"},
                             {"z_next", z_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed,
                         LSNF_HMC_INIT | LSNF_HMC_INNER | LSNF_HMC_ADAPT | LSNF_HMC_ADAPT_LAST | LSNF_HMC_METRIC_FOLD | LSNF_HMC_METRIC_CLOSE |
                             LSNF_HMC_ANNEAL | LSNF_HMC_SWAP | LSNF_HMC_SWAP_ODD,
                         init, inner, "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, /*step_size=*/1.0f, flags};
    const RowSteps rows = {step_rows, adapt, da, flags};
    const RowMetric metric = {mean_rows, m2_rows, count_rows, reg, flags};
    const RowTemper temper = {beta_next, log_w, flags};
    const RowExchange exchange = {ladder, B, swap_uniform, swap_out, log_swap_out, rng, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || rows.scalars(ck) ||
        metric.scalars(ck) || temper.scalars(ck) || exchange.scalars(ck) || s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck) || rows.pointers(ck) || metric.pointers(ck) || temper.pointers(ck) || exchange.pointers(ck))
        return ck.rc;
    const LsnfLangevinArgs lv = {z_prop, grad_g, noise, z_next, nullptr, nullptr, 0.0f, rng_args(rng)};
    LsnfHmcExchangeCall c;               // (no g_z1 / g_logdet / g_z_in: the gradient of -log p at the point, consumed by the tail)
    ck.head(c, plan, B, stream, {z_prop, z_out, z_saved, grad_g, noise, z_next, z_acc, grad_acc, mom, scale_rows, mean_rows, m2_rows, like_grad_acc});
    c.z_out = z_out; c.z_saved = z_saved; c.act_saved = act_saved; c.ll_mode = 1; c.ll_scale = -1.0f; c.lv = &lv; c.ll_prop = ll_prop;
    c.chain = {energy_g, uniform, z_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    c.step_rows = step_rows; c.adapt = adapt; c.da = rows.args();
    c.scale = scale_rows; c.mean = mean_rows; c.m2 = m2_rows; c.count = count_rows; c.reg = metric.args();
    c.beta_rows = beta_rows; c.beta_next = beta_next; c.like_grad_acc = like_grad_acc; c.like_u_acc = like_u_acc; c.log_w = log_w;
    c.ladder = ladder; c.swap_uniform = swap_uniform; c.swap_out = swap_out; c.log_swap_out = log_swap_out;
    const Pick p = select_hmc_exchange(c);
    return report(ck.entry, p, lsnf_launch_small3_hmc_exchange(c, p.st));
}

int lsnf_reverse_hmc_step_exchange(const float* plan, int nz, int width, int depth, int coupling, int B, const float* eps_prop,
                                   const float* z_saved, const float* act_saved, const float* grad_g, const float* energy_g, float* eps_acc,
                                   float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                                   const LsnfRng* rng, float* step_rows, float* adapt, const LsnfDualAvg* da, float* scale_rows,
                                   float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg, float* beta_rows,
                                   const float* beta_next, float* like_grad_acc, float* like_u_acc, float* log_w, unsigned flags,
                                   float* eps_next, float* accept_out, float* log_alpha_out, int ladder, const float* swap_uniform,
                                   float* swap_out, float* log_swap_out, void* stream) {
    Check ck{"lsnf_reverse_hmc_step_exchange"};
    const Named reads[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"z_saved", z_saved}, {"act_saved", act_saved}, {"grad_g", grad_g},
                           {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform},
                           {"swap_uniform", swap_uniform}};
    const Named writes[] = {{"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"eps_next", eps_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"adapt", adapt},
                            {"scale_rows", scale_rows}, {"mean_rows", mean_rows}, {"m2_rows", m2_rows}, {"count_rows", count_rows},
                            {"beta_rows", beta_rows}, {"beta_next", beta_next}, {"like_grad_acc", like_grad_acc},
                            {"like_u_acc", like_u_acc}, {"log_w", log_w}, {"swap_out", swap_out}, {"log_swap_out", log_swap_out}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc},
                             {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"scale_rows", scale_rows}, {"beta_rows", beta_rows},
                             {"like_grad_acc", like_grad_acc}, {"like_u_acc", like_u_acc},
                             {"act_saved", act_saved, true, "(the stash of lsnf_forward, lsnf_restash or lsnf_reverse_keep)"},
                             {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"}, {"eps_next", eps_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed,
                         LSNF_HMC_INIT | LSNF_HMC_INNER | LSNF_HMC_ADAPT | LSNF_HMC_ADAPT_LAST | LSNF_HMC_METRIC_FOLD | LSNF_HMC_METRIC_CLOSE |
                             LSNF_HMC_ANNEAL | LSNF_HMC_SWAP | LSNF_HMC_SWAP_ODD,
                         init, inner, "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, /*step_size=*/1.0f, flags};
    const RowSteps rows = {step_rows, adapt, da, flags};
    const RowMetric metric = {mean_rows, m2_rows, count_rows, reg, flags};
    const RowTemper temper = {beta_next, log_w, flags};
    const RowExchange exchange = {ladder, B, swap_uniform, swap_out, log_swap_out, rng, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || rows.scalars(ck) ||
        metric.scalars(ck) || temper.scalars(ck) || exchange.scalars(ck) || s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck) || rows.pointers(ck) || metric.pointers(ck) || temper.pointers(ck) || exchange.pointers(ck))
        return ck.rc;
    LsnfReverseHmcExchangeCall c;        // (no g_x / g_objective / g_z_in: the gradient at the point is consumed by the tail)
    ck.head(c, plan, B, stream, {eps_prop, z_saved, grad_g, noise, eps_next, eps_acc, grad_acc, mom, scale_rows, mean_rows, m2_rows, like_grad_acc});
    c.z_out = eps_prop; c.z_saved = z_saved; c.act_saved = act_saved;
    c.grad_g = grad_g; c.noise = noise; c.step = 0.0f; c.eps_new = eps_next; c.rng = rng_args(rng);
    c.chain = {energy_g, uniform, eps_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    c.step_rows = step_rows; c.adapt = adapt; c.da = rows.args();
    c.scale = scale_rows; c.mean = mean_rows; c.m2 = m2_rows; c.count = count_rows; c.reg = metric.args();
    c.beta_rows = beta_rows; c.beta_next = beta_next; c.like_grad_acc = like_grad_acc; c.like_u_acc = like_u_acc; c.log_w = log_w;
    c.ladder = ladder; c.swap_uniform = swap_uniform; c.swap_out = swap_out; c.log_swap_out = log_swap_out;
    const Pick p = select_reverse_hmc_exchange(c);
    return report(ck.entry, p, lsnf_launch_small3_reverse_hmc_exchange(c, p.st));
}

// The two HMC entries with a resampling move: the tempered entries' tables and rules, resample_uniform among the reads, ancestor_out
// and ess_out among the outputs, RowResample's rules after RowTemper's.
int lsnf_hmc_step_resample(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_prop, const float* z_out,
                           const float* z_saved, const float* act_saved, const float* ll_prop, const float* grad_g, const float* energy_g,
                           float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                           const LsnfRng* rng, float* step_rows, float* adapt, const LsnfDualAvg* da, float* scale_rows, float* mean_rows,
                           float* m2_rows, float* count_rows, const LsnfMetricReg* reg, float* beta_rows, const float* beta_next,
                           float* like_grad_acc, float* like_u_acc, float* log_w, unsigned flags, float* z_next, float* accept_out,
                           float* log_alpha_out, int group, float ess_frac, const float* resample_uniform, float* ancestor_out,
                           float* ess_out, void* stream) {
    Check ck{"lsnf_hmc_step_resample"};
    const Named reads[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"z_saved", z_saved}, {"act_saved", act_saved},
                           {"ll_prop", ll_prop}, {"grad_g", grad_g}, {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform},
                           {"resample_uniform", resample_uniform}};
    const Named writes[] = {{"z_acc", z_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"z_next", z_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"adapt", adapt},
                            {"scale_rows", scale_rows}, {"mean_rows", mean_rows}, {"m2_rows", m2_rows}, {"count_rows", count_rows},
                            {"beta_rows", beta_rows}, {"beta_next", beta_next}, {"like_grad_acc", like_grad_acc},
                            {"like_u_acc", like_u_acc}, {"log_w", log_w}, {"ancestor_out", ancestor_out}, {"ess_out", ess_out}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"act_saved", act_saved}, {"z_acc", z_acc},
                             {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows},
                             {"scale_rows", scale_rows}, {"beta_rows", beta_rows}, {"like_grad_acc", like_grad_acc},
                             {"like_u_acc", like_u_acc},
                             {"ll_prop", ll_prop, !inner, "(NULL) unless LSNF_HMC_INNER"}, {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"},
                             {"z_next", z_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed,
                         LSNF_HMC_INIT | LSNF_HMC_INNER | LSNF_HMC_ADAPT | LSNF_HMC_ADAPT_LAST | LSNF_HMC_METRIC_FOLD | LSNF_HMC_METRIC_CLOSE |
                             LSNF_HMC_ANNEAL | LSNF_HMC_RESAMPLE,
                         init, inner, "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, /*step_size=*/1.0f, flags};
    const RowSteps rows = {step_rows, adapt, da, flags};
    const RowMetric metric = {mean_rows, m2_rows, count_rows, reg, flags};
    const RowTemper temper = {beta_next, log_w, flags};
    const RowResample resample = {group, B, resample_uniform, ancestor_out, ess_out, rng, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || rows.scalars(ck) ||
        metric.scalars(ck) || temper.scalars(ck) || resample.scalars(ck) || s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck) || rows.pointers(ck) || metric.pointers(ck) || temper.pointers(ck) || resample.pointers(ck))
        return ck.rc;
    const LsnfLangevinArgs lv = {z_prop, grad_g, noise, z_next, nullptr, nullptr, 0.0f, rng_args(rng)};
    LsnfHmcResampleCall c;               // (no g_z1 / g_logdet / g_z_in: the gradient of -log p at the point, consumed by the tail)
    ck.head(c, plan, B, stream, {z_prop, z_out, z_saved, grad_g, noise, z_next, z_acc, grad_acc, mom, scale_rows, mean_rows, m2_rows, like_grad_acc});
    c.z_out = z_out; c.z_saved = z_saved; c.act_saved = act_saved; c.ll_mode = 1; c.ll_scale = -1.0f; c.lv = &lv; c.ll_prop = ll_prop;
    c.chain = {energy_g, uniform, z_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    c.step_rows = step_rows; c.adapt = adapt; c.da = rows.args();
    c.scale = scale_rows; c.mean = mean_rows; c.m2 = m2_rows; c.count = count_rows; c.reg = metric.args();
    c.beta_rows = beta_rows; c.beta_next = beta_next; c.like_grad_acc = like_grad_acc; c.like_u_acc = like_u_acc; c.log_w = log_w;
    c.group = group; c.ess_frac = ess_frac; c.resample_uniform = resample_uniform; c.ancestor_out = ancestor_out; c.ess_out = ess_out;
    const Pick p = select_hmc_resample(c);
    return report(ck.entry, p, lsnf_launch_small3_hmc_resample(c, p.st));
}

int lsnf_reverse_hmc_step_resample(const float* plan, int nz, int width, int depth, int coupling, int B, const float* eps_prop,
                                   const float* z_saved, const float* act_saved, const float* grad_g, const float* energy_g, float* eps_acc,
                                   float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                                   const LsnfRng* rng, float* step_rows, float* adapt, const LsnfDualAvg* da, float* scale_rows,
                                   float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg, float* beta_rows,
                                   const float* beta_next, float* like_grad_acc, float* like_u_acc, float* log_w, unsigned flags,
                                   float* eps_next, float* accept_out, float* log_alpha_out, int group, float ess_frac,
                                   const float* resample_uniform, float* ancestor_out, float* ess_out, void* stream) {
    Check ck{"lsnf_reverse_hmc_step_resample"};
    const Named reads[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"z_saved", z_saved}, {"act_saved", act_saved}, {"grad_g", grad_g},
                           {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform},
                           {"resample_uniform", resample_uniform}};
    const Named writes[] = {{"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"eps_next", eps_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"adapt", adapt},
                            {"scale_rows", scale_rows}, {"mean_rows", mean_rows}, {"m2_rows", m2_rows}, {"count_rows", count_rows},
                            {"beta_rows", beta_rows}, {"beta_next", beta_next}, {"like_grad_acc", like_grad_acc},
                            {"like_u_acc", like_u_acc}, {"log_w", log_w}, {"ancestor_out", ancestor_out}, {"ess_out", ess_out}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc},
                             {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"scale_rows", scale_rows}, {"beta_rows", beta_rows},
                             {"like_grad_acc", like_grad_acc}, {"like_u_acc", like_u_acc},
                             {"act_saved", act_saved, true, "(the stash of lsnf_forward, lsnf_restash or lsnf_reverse_keep)"},
                             {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"}, {"eps_next", eps_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed,
                         LSNF_HMC_INIT | LSNF_HMC_INNER | LSNF_HMC_ADAPT | LSNF_HMC_ADAPT_LAST | LSNF_HMC_METRIC_FOLD | LSNF_HMC_METRIC_CLOSE |
                             LSNF_HMC_ANNEAL | LSNF_HMC_RESAMPLE,
                         init, inner, "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, /*step_size=*/1.0f, flags};
    const RowSteps rows = {step_rows, adapt, da, flags};
    const RowMetric metric = {mean_rows, m2_rows, count_rows, reg, flags};
    const RowTemper temper = {beta_next, log_w, flags};
    const RowResample resample = {group, B, resample_uniform, ancestor_out, ess_out, rng, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || rows.scalars(ck) ||
        metric.scalars(ck) || temper.scalars(ck) || resample.scalars(ck) || s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck) || rows.pointers(ck) || metric.pointers(ck) || temper.pointers(ck) || resample.pointers(ck))
        return ck.rc;
    LsnfReverseHmcResampleCall c;        // (no g_x / g_objective / g_z_in: the gradient at the point is consumed by the tail)
    ck.head(c, plan, B, stream, {eps_prop, z_saved, grad_g, noise, eps_next, eps_acc, grad_acc, mom, scale_rows, mean_rows, m2_rows, like_grad_acc});
    c.z_out = eps_prop; c.z_saved = z_saved; c.act_saved = act_saved;
    c.grad_g = grad_g; c.noise = noise; c.step = 0.0f; c.eps_new = eps_next; c.rng = rng_args(rng);
    c.chain = {energy_g, uniform, eps_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    c.step_rows = step_rows; c.adapt = adapt; c.da = rows.args();
    c.scale = scale_rows; c.mean = mean_rows; c.m2 = m2_rows; c.count = count_rows; c.reg = metric.args();
    c.beta_rows = beta_rows; c.beta_next = beta_next; c.like_grad_acc = like_grad_acc; c.like_u_acc = like_u_acc; c.log_w = log_w;
    c.group = group; c.ess_frac = ess_frac; c.resample_uniform = resample_uniform; c.ancestor_out = ancestor_out; c.ess_out = ess_out;
    const Pick p = select_reverse_hmc_resample(c);
    return report(ck.entry, p, lsnf_launch_small3_reverse_hmc_resample(c, p.st));
}

// The two HMC entries with a schedule search: the resampling entries' tables and rules, cess_frac and min_step behind ess_out,
// RowSchedule's rules after RowResample's.
int lsnf_hmc_step_schedule(const float* plan, int nz, int width, int depth, int coupling, int B, const float* z_prop, const float* z_out,
                           const float* z_saved, const float* act_saved, const float* ll_prop, const float* grad_g, const float* energy_g,
                           float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                           const LsnfRng* rng, float* step_rows, float* adapt, const LsnfDualAvg* da, float* scale_rows, float* mean_rows,
                           float* m2_rows, float* count_rows, const LsnfMetricReg* reg, float* beta_rows, const float* beta_next,
                           float* like_grad_acc, float* like_u_acc, float* log_w, unsigned flags, float* z_next, float* accept_out,
                           float* log_alpha_out, int group, float ess_frac, const float* resample_uniform, float* ancestor_out,
                           float* ess_out, float cess_frac, float min_step, void* stream) {
    Check ck{"lsnf_hmc_step_schedule"};
    const Named reads[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"z_saved", z_saved}, {"act_saved", act_saved},
                           {"ll_prop", ll_prop}, {"grad_g", grad_g}, {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform},
                           {"resample_uniform", resample_uniform}};
    const Named writes[] = {{"z_acc", z_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"z_next", z_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"adapt", adapt},
                            {"scale_rows", scale_rows}, {"mean_rows", mean_rows}, {"m2_rows", m2_rows}, {"count_rows", count_rows},
                            {"beta_rows", beta_rows}, {"beta_next", beta_next}, {"like_grad_acc", like_grad_acc},
                            {"like_u_acc", like_u_acc}, {"log_w", log_w}, {"ancestor_out", ancestor_out}, {"ess_out", ess_out}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"z_prop", z_prop}, {"z_out", z_out}, {"act_saved", act_saved}, {"z_acc", z_acc},
                             {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows},
                             {"scale_rows", scale_rows}, {"beta_rows", beta_rows}, {"like_grad_acc", like_grad_acc},
                             {"like_u_acc", like_u_acc},
                             {"ll_prop", ll_prop, !inner, "(NULL) unless LSNF_HMC_INNER"}, {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"},
                             {"z_next", z_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed,
                         LSNF_HMC_INIT | LSNF_HMC_INNER | LSNF_HMC_ADAPT | LSNF_HMC_ADAPT_LAST | LSNF_HMC_METRIC_FOLD | LSNF_HMC_METRIC_CLOSE |
                             LSNF_HMC_ANNEAL | LSNF_HMC_RESAMPLE | LSNF_HMC_SCHEDULE,
                         init, inner, "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, /*step_size=*/1.0f, flags};
    const RowSteps rows = {step_rows, adapt, da, flags};
    const RowMetric metric = {mean_rows, m2_rows, count_rows, reg, flags};
    const RowTemper temper = {beta_next, log_w, flags};
    const RowResample resample = {group, B, resample_uniform, ancestor_out, ess_out, rng, flags};
    const RowSchedule schedule = {group, B, cess_frac, min_step, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || rows.scalars(ck) ||
        metric.scalars(ck) || temper.scalars(ck) || resample.scalars(ck) || schedule.scalars(ck) || s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck) || rows.pointers(ck) || metric.pointers(ck) || temper.pointers(ck) || resample.pointers(ck))
        return ck.rc;
    const LsnfLangevinArgs lv = {z_prop, grad_g, noise, z_next, nullptr, nullptr, 0.0f, rng_args(rng)};
    LsnfHmcScheduleCall c;               // (no g_z1 / g_logdet / g_z_in: the gradient of -log p at the point, consumed by the tail)
    ck.head(c, plan, B, stream, {z_prop, z_out, z_saved, grad_g, noise, z_next, z_acc, grad_acc, mom, scale_rows, mean_rows, m2_rows, like_grad_acc});
    c.z_out = z_out; c.z_saved = z_saved; c.act_saved = act_saved; c.ll_mode = 1; c.ll_scale = -1.0f; c.lv = &lv; c.ll_prop = ll_prop;
    c.chain = {energy_g, uniform, z_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    c.step_rows = step_rows; c.adapt = adapt; c.da = rows.args();
    c.scale = scale_rows; c.mean = mean_rows; c.m2 = m2_rows; c.count = count_rows; c.reg = metric.args();
    c.beta_rows = beta_rows; c.beta_next = beta_next; c.like_grad_acc = like_grad_acc; c.like_u_acc = like_u_acc; c.log_w = log_w;
    c.group = group; c.ess_frac = ess_frac; c.resample_uniform = resample_uniform; c.ancestor_out = ancestor_out; c.ess_out = ess_out;
    c.cess_frac = cess_frac; c.min_step = min_step;
    const Pick p = select_hmc_schedule(c);
    return report(ck.entry, p, lsnf_launch_small3_hmc_schedule(c, p.st));
}

int lsnf_reverse_hmc_step_schedule(const float* plan, int nz, int width, int depth, int coupling, int B, const float* eps_prop,
                                   const float* z_saved, const float* act_saved, const float* grad_g, const float* energy_g, float* eps_acc,
                                   float* grad_acc, float* u_acc, float* mom, float* kin0, const float* noise, const float* uniform,
                                   const LsnfRng* rng, float* step_rows, float* adapt, const LsnfDualAvg* da, float* scale_rows,
                                   float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg, float* beta_rows,
                                   const float* beta_next, float* like_grad_acc, float* like_u_acc, float* log_w, unsigned flags,
                                   float* eps_next, float* accept_out, float* log_alpha_out, int group, float ess_frac,
                                   const float* resample_uniform, float* ancestor_out, float* ess_out, float cess_frac,
                                   float min_step, void* stream) {
    Check ck{"lsnf_reverse_hmc_step_schedule"};
    const Named reads[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"z_saved", z_saved}, {"act_saved", act_saved}, {"grad_g", grad_g},
                           {"energy_g", energy_g}, {"noise", noise}, {"uniform", uniform},
                           {"resample_uniform", resample_uniform}};
    const Named writes[] = {{"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc}, {"eps_next", eps_next}, {"accept_out", accept_out},
                            {"log_alpha_out", log_alpha_out}, {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"adapt", adapt},
                            {"scale_rows", scale_rows}, {"mean_rows", mean_rows}, {"m2_rows", m2_rows}, {"count_rows", count_rows},
                            {"beta_rows", beta_rows}, {"beta_next", beta_next}, {"like_grad_acc", like_grad_acc},
                            {"like_u_acc", like_u_acc}, {"log_w", log_w}, {"ancestor_out", ancestor_out}, {"ess_out", ess_out}};
    const bool init = (flags & LSNF_HMC_INIT) != 0, inner = (flags & LSNF_HMC_INNER) != 0;
    const Needed needed[] = {{"plan", plan}, {"eps_prop", eps_prop}, {"eps_acc", eps_acc}, {"grad_acc", grad_acc}, {"u_acc", u_acc},
                             {"mom", mom}, {"kin0", kin0}, {"step_rows", step_rows}, {"scale_rows", scale_rows}, {"beta_rows", beta_rows},
                             {"like_grad_acc", like_grad_acc}, {"like_u_acc", like_u_acc},
                             {"act_saved", act_saved, true, "(the stash of lsnf_forward, lsnf_restash or lsnf_reverse_keep)"},
                             {"z_saved", z_saved, depth > 1, "(NULL) for depth > 1"}, {"eps_next", eps_next, inner, "(NULL) with LSNF_HMC_INNER"}};
    const ChainStep s = {reads, writes, /*next=*/&writes[3], /*point=*/&reads[1], needed,
                         LSNF_HMC_INIT | LSNF_HMC_INNER | LSNF_HMC_ADAPT | LSNF_HMC_ADAPT_LAST | LSNF_HMC_METRIC_FOLD | LSNF_HMC_METRIC_CLOSE |
                             LSNF_HMC_ANNEAL | LSNF_HMC_RESAMPLE | LSNF_HMC_SCHEDULE,
                         init, inner, "LSNF_HMC_INIT or LSNF_HMC_INNER", plan, act_saved, noise, uniform, rng, /*step_size=*/1.0f, flags};
    const RowSteps rows = {step_rows, adapt, da, flags};
    const RowMetric metric = {mean_rows, m2_rows, count_rows, reg, flags};
    const RowTemper temper = {beta_next, log_w, flags};
    const RowResample resample = {group, B, resample_uniform, ancestor_out, ess_out, rng, flags};
    const RowSchedule schedule = {group, B, cess_frac, min_step, flags};
    if (ck.geometry(nz, width, depth, coupling) || ck.batch(B) || s.scalars(ck) || s.phases(ck, accept_out, log_alpha_out) || rows.scalars(ck) ||
        metric.scalars(ck) || temper.scalars(ck) || resample.scalars(ck) || schedule.scalars(ck) || s.aliases(ck))
        return ck.rc;
    if (ck.empty) return LSNF_OK;
    if (s.pointers(ck) || rows.pointers(ck) || metric.pointers(ck) || temper.pointers(ck) || resample.pointers(ck))
        return ck.rc;
    LsnfReverseHmcScheduleCall c;        // (no g_x / g_objective / g_z_in: the gradient at the point is consumed by the tail)
    ck.head(c, plan, B, stream, {eps_prop, z_saved, grad_g, noise, eps_next, eps_acc, grad_acc, mom, scale_rows, mean_rows, m2_rows, like_grad_acc});
    c.z_out = eps_prop; c.z_saved = z_saved; c.act_saved = act_saved;
    c.grad_g = grad_g; c.noise = noise; c.step = 0.0f; c.eps_new = eps_next; c.rng = rng_args(rng);
    c.chain = {energy_g, uniform, eps_acc, grad_acc, u_acc, accept_out, log_alpha_out, flags}; c.mom = mom; c.kin0 = kin0;
    c.step_rows = step_rows; c.adapt = adapt; c.da = rows.args();
    c.scale = scale_rows; c.mean = mean_rows; c.m2 = m2_rows; c.count = count_rows; c.reg = metric.args();
    c.beta_rows = beta_rows; c.beta_next = beta_next; c.like_grad_acc = like_grad_acc; c.like_u_acc = like_u_acc; c.log_w = log_w;
    c.group = group; c.ess_frac = ess_frac; c.resample_uniform = resample_uniform; c.ancestor_out = ancestor_out; c.ess_out = ess_out;
    c.cess_frac = cess_frac; c.min_step = min_step;
    const Pick p = select_reverse_hmc_schedule(c);
    return report(ck.entry, p, lsnf_launch_small3_reverse_hmc_schedule(c, p.st));
}

size_t lsnf_backward_params_workspace_floats(int nz, int width, int depth, int B) {
    LsnfGeo g;
    if (lsnf_geo_init(&g, nz, width, depth, 1) || B < 0) return 0;   // independent of the coupling type
    return lsnf_params_workspace_floats(nz, width, depth, B);
}

int lsnf_backward_params(const float* plan, const float* const* params_host, float* const* grads_host, int nz, int width,
                         int depth, int coupling, int B, const float* z_in, const float* z_out, const float* z_saved,
                         const float* act_saved, const float* g_z1, const float* g_logdet, int ll_mode, float ll_scale,
                         float* g_z_in, float* workspace, void* stream) {
    return backward_params_entry("lsnf_backward_params", 0, plan, params_host, grads_host, nz, width, depth, coupling, B, z_in, z_out, z_saved,
                                 act_saved, g_z1, g_logdet, ll_mode, ll_scale, g_z_in, workspace, stream);
}

size_t lsnf_backward_params_det_workspace_floats(int nz, int width, int depth, int B) {
    LsnfGeo g;
    if (lsnf_geo_init(&g, nz, width, depth, 1) || B < 0) return 0;   // independent of the coupling type
    return lsnf_params_det_workspace_floats(nz, width, depth, B);
}

int lsnf_backward_params_det(const float* plan, const float* const* params_host, float* const* grads_host, int nz, int width,
                             int depth, int coupling, int B, const float* z_in, const float* z_out, const float* z_saved,
                             const float* act_saved, const float* g_z1, const float* g_logdet, int ll_mode, float ll_scale,
                             float* g_z_in, float* workspace, void* stream) {
    return backward_params_entry("lsnf_backward_params_det", 1, plan, params_host, grads_host, nz, width, depth, coupling, B, z_in, z_out,
                                 z_saved, act_saved, g_z1, g_logdet, ll_mode, ll_scale, g_z_in, workspace, stream);
}

}  // extern "C"

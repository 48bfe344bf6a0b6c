// lsnf_launch.h -- host only: the whole interface between the C ABI (lsnf_api.hip) and the kernel files.
//
// One call descriptor per operation: the entry point validates, fills the descriptor ONCE, selects by the predicates below and
// hands the same descriptor to the launcher(s) of its pick -- a predicate and the launcher's opening guard therefore see the very
// call the selection saw.  Every launcher / predicate takes the descriptor plus at most the one thing the selection decided (st,
// fixup, the contraction kind).  A new operand of an operation is one new member here (NULL / 0 where a caller does not set it)
// and the kernels that use it.  Below the declarations: the host helpers every launcher shares.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <type_traits>
#include "lsnf_layout.h"

// ---- call descriptors -------------------------------------------------------------------------------------------------
struct LsnfCall {                        // what every call on a prepared plan has
    LsnfGeo g;
    const float* plan = nullptr;
    int B = 0;
    int vec4 = 1;                        // vector width (floats) that every (B, nz) tensor of the call allows: 4, 2 or 1
    hipStream_t stream = nullptr;
};
struct LsnfForwardCall : LsnfCall {      // lsnf_forward
    int first_block = 0, n_blocks = 0;
    const float* z_in = nullptr; const float* objective = nullptr;
    float* z_out = nullptr; float* logdet_out = nullptr; float* ll_out = nullptr;
    float* z_saved = nullptr; float* act_saved = nullptr;     // of the whole stack: the launchers move to first_block
    double* stats = nullptr;
    float* hdump = nullptr; int hdump_tiled = 0;              // parameter-gradient dump (LsnfDumpLayout) of block 0; h1 / h2 tiled
};
struct LsnfRestashCall : LsnfCall {      // lsnf_restash
    const float* z_out = nullptr; const float* z_saved = nullptr; float* act_saved = nullptr;
};
struct LsnfReverseCall : LsnfCall {      // lsnf_reverse; lsnf_sample: smp != NULL runs the kernels' sampling form, which draws its
    const float* z_in = nullptr; const float* objective = nullptr;      // rows -- z_in / objective are then NULL
    float* z_out = nullptr; float* objective_out = nullptr;
    const LsnfSampleArgs* smp = nullptr;
    // lsnf_reverse_keep / lsnf_sample_keep (NULL elsewhere; only the latency bf16x3 kernel writes them): the block outputs, the stash
    // and the parameter-gradient dump (LsnfDumpLayout of block 0, h1 / h2 row-major) of the FORWARD at z_out
    float* z_saved = nullptr; float* act_saved = nullptr; float* hdump = nullptr;
};
struct LsnfBackwardCall : LsnfCall {     // lsnf_backward_z, lsnf_langevin_step (lv != NULL), step (1) of lsnf_backward_params (dump)
    const float* z_out = nullptr; const float* z_saved = nullptr; const float* act_saved = nullptr;
    const float* g_z1 = nullptr; const float* g_logdet = nullptr;
    int ll_mode = 0; float ll_scale = 0.f;
    float* g_z_in = nullptr;
    const LsnfLangevinArgs* lv = nullptr;
    float* dump = nullptr; double* gl_total = nullptr; int dump_tiled = 0;
};
struct LsnfChainArgs {                   // what every Metropolis-adjusted step has: the caller's energy, the uniform, the kept state
    const float* energy_g = nullptr; const float* uniform = nullptr;      // (acc = the accepted points), the decision, the flags
    float* acc = nullptr; float* grad_acc = nullptr; float* u_acc = nullptr;
    float* accept_out = nullptr; float* log_alpha_out = nullptr;
    unsigned flags = 0;                  // LSNF_MALA_* / LSNF_HMC_*
};
struct LsnfMalaCall : LsnfBackwardCall {  // lsnf_mala_step: ll_mode 1 / ll_scale -1 at the proposal; lv holds z_prop (z_cur), grad_g,
    const float* ll_prop = nullptr;      // noise, z_next (z_new), step, rng
    LsnfChainArgs chain;                 // (acc: z_acc)
};
struct LsnfHmcCall : LsnfMalaCall {      // lsnf_hmc_step: the MALA call's tensors at a point of a trajectory; flags: LSNF_HMC_*
    float* mom = nullptr; float* kin0 = nullptr;      // the momentum (B, nz; read and written), the kinetic energy the trajectory began with (B)
};
struct LsnfHmcRowsCall : LsnfHmcCall {   // lsnf_hmc_step_rows: lv->step is not read; flags: LSNF_HMC_* with ADAPT / ADAPT_LAST
    float* step_rows = nullptr; float* adapt = nullptr;      // each row's step (B), the rows' dual-averaging state (B, 4; ADAPT only)
    LsnfDualAvgArgs da = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
};
struct LsnfHmcMetricCall : LsnfHmcRowsCall {      // lsnf_hmc_step_metric; flags: LsnfHmcRowsCall's with METRIC_FOLD / METRIC_CLOSE
    float* scale = nullptr;              // each row's scale per column (B, nz): read by every phase, written by a closing call
    float* mean = nullptr; float* m2 = nullptr; float* count = nullptr;      // the window's Welford state (B, nz; B, nz; B): FOLD only
    LsnfMetricArgs reg = {0.f, 0.f, 0.f, 0.f};
};
struct LsnfHmcTemperedCall : LsnfHmcMetricCall {      // lsnf_hmc_step_tempered; flags: LsnfHmcMetricCall's with ANNEAL
    float* beta_rows = nullptr;          // each row's likelihood temperature (B): read by every phase, written by an annealing call
    const float* beta_next = nullptr;    // the next one (B): ANNEAL only
    float* like_grad_acc = nullptr; float* like_u_acc = nullptr;      // the likelihood's part of the kept state (B, nz; B)
    float* log_w = nullptr;              // the Kahan pair of the rows' importance weights (B, 2; 8-byte aligned): ANNEAL only
};
struct LsnfHmcExchangeCall : LsnfHmcTemperedCall {      // lsnf_hmc_step_exchange; flags: LsnfHmcTemperedCall's with SWAP / SWAP_ODD
    int ladder = 0;                      // R consecutive rows aligned to R are the rungs of one ladder (2, 4, 8 or 16): SWAP only
    const float* swap_uniform = nullptr; // the pairs' uniforms (B), read at the lower row; NULL: drawn in-kernel
    float* swap_out = nullptr; float* log_swap_out = nullptr;      // optional (B each)
};
struct LsnfHmcResampleCall : LsnfHmcTemperedCall {      // lsnf_hmc_step_resample; flags: LsnfHmcTemperedCall's with RESAMPLE
    int group = 0;                       // P consecutive rows aligned to P are the particles of one group (2, 4, 8 or 16): RESAMPLE only
    float ess_frac = 0.0f;               // a group resamples iff its effective sample size is below ess_frac * P
    const float* resample_uniform = nullptr;   // the groups' uniforms (B), read at the group's first row; NULL: drawn in-kernel
    float* ancestor_out = nullptr; float* ess_out = nullptr;       // optional (B each)
};
struct LsnfHmcScheduleCall : LsnfHmcResampleCall {      // lsnf_hmc_step_schedule; flags: LsnfHmcResampleCall's with SCHEDULE
    float cess_frac = 0.0f;              // a searching group steps to where its conditional effective sample size is cess_frac * P
    float min_step = 0.0f;               // and by no less than this (`group` is the length for SCHEDULE and RESAMPLE alike)
};
struct LsnfReverseBackwardCall : LsnfCall {      // lsnf_reverse_backward_z
    const float* z_out = nullptr; const float* z_saved = nullptr; const float* act_saved = nullptr;
    const float* g_x = nullptr; const float* g_objective = nullptr;
    float* g_z_in = nullptr;
};
struct LsnfReverseLangevinCall : LsnfReverseBackwardCall {      // lsnf_reverse_langevin_step: g_x / g_objective stay NULL (the
    const float* grad_g = nullptr; const float* noise = nullptr;   // upstream gradient is grad_g), g_z_in is the optional g_eps_out
    LsnfRngArgs rng = {0ull, 0ull, nullptr, 0ll, 0};
    float step = 0.f;
    float* eps_new = nullptr; float* g_norm = nullptr; float* eps_norm = nullptr;
};
struct LsnfReverseMalaCall : LsnfReverseLangevinCall {      // lsnf_reverse_mala_step: z_out is the proposal eps_prop, eps_new the next
    LsnfChainArgs chain;                 // proposal eps_next (may be NULL); g_z_in and the norms stay NULL.  (acc: eps_acc)
};
struct LsnfReverseHmcCall : LsnfReverseMalaCall {      // lsnf_reverse_hmc_step: the base-space MALA call's tensors at a point of a
    float* mom = nullptr; float* kin0 = nullptr;      // trajectory; flags: LSNF_HMC_*.  mom (B, nz; read and written), kin0 (B)
};
struct LsnfReverseHmcRowsCall : LsnfReverseHmcCall {      // lsnf_reverse_hmc_step_rows: `step` is not read; flags as LsnfHmcRowsCall's
    float* step_rows = nullptr; float* adapt = nullptr;
    LsnfDualAvgArgs da = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
};
struct LsnfReverseHmcMetricCall : LsnfReverseHmcRowsCall {      // lsnf_reverse_hmc_step_metric: as LsnfHmcMetricCall
    float* scale = nullptr; float* mean = nullptr; float* m2 = nullptr; float* count = nullptr;
    LsnfMetricArgs reg = {0.f, 0.f, 0.f, 0.f};
};
struct LsnfReverseHmcTemperedCall : LsnfReverseHmcMetricCall {      // lsnf_reverse_hmc_step_tempered: as LsnfHmcTemperedCall
    float* beta_rows = nullptr; const float* beta_next = nullptr; float* like_grad_acc = nullptr; float* like_u_acc = nullptr;
    float* log_w = nullptr;
};
struct LsnfReverseHmcExchangeCall : LsnfReverseHmcTemperedCall {      // lsnf_reverse_hmc_step_exchange: as LsnfHmcExchangeCall
    int ladder = 0; const float* swap_uniform = nullptr; float* swap_out = nullptr; float* log_swap_out = nullptr;
};
struct LsnfReverseHmcResampleCall : LsnfReverseHmcTemperedCall {      // lsnf_reverse_hmc_step_resample: as LsnfHmcResampleCall
    int group = 0; float ess_frac = 0.0f; const float* resample_uniform = nullptr; float* ancestor_out = nullptr; float* ess_out = nullptr;
};
struct LsnfReverseHmcScheduleCall : LsnfReverseHmcResampleCall {      // lsnf_reverse_hmc_step_schedule: as LsnfHmcScheduleCall
    float cess_frac = 0.0f; float min_step = 0.0f;
};
struct LsnfContractCall : LsnfCall {     // steps (2), (3) of lsnf_backward_params: batch contraction of the dump, chain rule
    const float* const* params_host = nullptr; float* const* grads_host = nullptr;
    const float* z_in = nullptr; const float* z_out = nullptr; const float* z_saved = nullptr;
    float* workspace = nullptr;          // [G | folded gradients | dump | tag] (lsnf_layout.h)
    int g_tiled = 0;                     // the backward wrote its g arrays tiled
    // lsnf_backward_params_det: the contraction writes per-chunk partials behind the tag word (lsnf_layout.h), chunked by (B,
    // depth, kind) alone, and lsnf_fold_reduce_kernel sums them -- and dL/dlogdet over the batch -- in a fixed order
    int det = 0;
    const float* g_logdet = nullptr; int ll_mode = 0; float ll_scale = 0.f;      // (det only: the upstream dL/dlogdet_b)
};
struct LsnfPrepareCall {                 // lsnf_prepare
    LsnfGeo g;
    const float* const* params_host = nullptr; float* plan = nullptr; void* scratch = nullptr;
    hipStream_t stream = nullptr;
};
struct LsnfInitCall {                    // lsnf_actnorm_init
    LsnfGeo g;
    float* const* params_host = nullptr; int B = 0; const float* z_in = nullptr; void* workspace = nullptr;
    hipStream_t stream = nullptr;
};
struct LsnfAdamCall {                    // lsnf_adam_step, lsnf_adam_step_ex
    LsnfGeo g;
    float* const* params_host = nullptr; const float* const* grads_host = nullptr; void* state = nullptr;
    double lr = 0.0, beta1 = 0.0, beta2 = 0.0, eps = 0.0, weight_decay = 0.0, max_norm = 0.0, ema_decay = 0.0;
    unsigned flags = 0;                  // LSNF_ADAM_*
    const float* lr_dev = nullptr; float* grad_norm_out = nullptr;
    hipStream_t stream = nullptr;
};

// ---- launchers and the predicates of what each takes (pure host functions, no HIP calls) ---------------------------------
// *_covers: does the kernel take this call?  *_st: rows per workgroup / 16 of a latency kernel for this call (forward, reverse:
// 0 if it does not take it).  fixup: 1 = run as the fix-up pass behind an fp16x2 launch.
size_t lsnf_prep_scratch_bytes(int nz, int depth);
hipError_t lsnf_launch_prepare(const LsnfPrepareCall& c);
size_t lsnf_init_workspace_bytes(const LsnfGeo& g, int B);
hipError_t lsnf_launch_actnorm_init(const LsnfInitCall& c);
size_t lsnf_adam_bytes(const LsnfGeo& g, unsigned flags);       // (only LSNF_ADAM_AMSGRAD and LSNF_ADAM_EMA count)
hipError_t lsnf_launch_adam(const LsnfAdamCall& c);

hipError_t lsnf_launch_forward(const LsnfForwardCall& c);
bool lsnf_forward3_covers(const LsnfForwardCall& c, int fixup);
hipError_t lsnf_launch_forward3(const LsnfForwardCall& c, int fixup);
bool lsnf_forward3q_covers(const LsnfForwardCall& c);
hipError_t lsnf_launch_forward3q(const LsnfForwardCall& c);
bool lsnf_forward2h_covers(const LsnfForwardCall& c, int fixup);
hipError_t lsnf_launch_forward2h(const LsnfForwardCall& c, int fixup);
int lsnf_small3_forward_st(const LsnfForwardCall& c);
hipError_t lsnf_launch_small3_forward(const LsnfForwardCall& c, int st);
bool lsnf_small_forward_covers(const LsnfForwardCall& c);
hipError_t lsnf_launch_small_forward(const LsnfForwardCall& c);
hipError_t lsnf_launch_small3_restash(const LsnfRestashCall& c);

hipError_t lsnf_launch_reverse(const LsnfReverseCall& c);
bool lsnf_reverse3_covers(const LsnfReverseCall& c);
hipError_t lsnf_launch_reverse3(const LsnfReverseCall& c, int fixup);
bool lsnf_reverse2h_covers(const LsnfReverseCall& c);
hipError_t lsnf_launch_reverse2h(const LsnfReverseCall& c, int fixup);
int lsnf_small3_reverse_st(const LsnfReverseCall& c);
hipError_t lsnf_launch_small3_reverse(const LsnfReverseCall& c, int st);
bool lsnf_small_reverse_covers(const LsnfReverseCall& c);
hipError_t lsnf_launch_small_reverse(const LsnfReverseCall& c);

hipError_t lsnf_launch_backward_z(const LsnfBackwardCall& c);
hipError_t lsnf_launch_backward3_z(const LsnfBackwardCall& c);
hipError_t lsnf_launch_backward3_z_wide(const LsnfBackwardCall& c);       // (lsnf_bwd3w.hip: the f_width-128 instantiation)
bool lsnf_small_backward_covers(const LsnfBackwardCall& c);
hipError_t lsnf_launch_small_backward_z(const LsnfBackwardCall& c);
int lsnf_small3_backward_st(const LsnfBackwardCall& c);
hipError_t lsnf_launch_small3_backward_z(const LsnfBackwardCall& c, int st);
hipError_t lsnf_launch_small3_mala(const LsnfMalaCall& c, int st);          // st: lsnf_small3_backward_st of the call
hipError_t lsnf_launch_small3_hmc(const LsnfHmcCall& c, int st);            // st: lsnf_small3_backward_st of the call
hipError_t lsnf_launch_small3_hmc_rows(const LsnfHmcRowsCall& c, int st);   // st: lsnf_small3_backward_st of the call
hipError_t lsnf_launch_small3_hmc_metric(const LsnfHmcMetricCall& c, int st);       // st: lsnf_small3_backward_st of the call
hipError_t lsnf_launch_small3_hmc_tempered(const LsnfHmcTemperedCall& c, int st);   // st: lsnf_small3_backward_st of the call
hipError_t lsnf_launch_small3_hmc_exchange(const LsnfHmcExchangeCall& c, int st);   // st: lsnf_small3_backward_st of the call
hipError_t lsnf_launch_small3_hmc_resample(const LsnfHmcResampleCall& c, int st);   // st: lsnf_small3_backward_st of the call
hipError_t lsnf_launch_small3_hmc_schedule(const LsnfHmcScheduleCall& c, int st);   // st: lsnf_small3_backward_st of the call
int lsnf_small3_reverse_backward_st(const LsnfReverseBackwardCall& c);
hipError_t lsnf_launch_small3_reverse_backward_z(const LsnfReverseBackwardCall& c, int st);
hipError_t lsnf_launch_small3_reverse_langevin(const LsnfReverseLangevinCall& c, int st);      // st: of the same predicate
hipError_t lsnf_launch_small3_reverse_mala(const LsnfReverseMalaCall& c, int st);              // st: of the same predicate
hipError_t lsnf_launch_small3_reverse_hmc(const LsnfReverseHmcCall& c, int st);                // st: of the same predicate
hipError_t lsnf_launch_small3_reverse_hmc_rows(const LsnfReverseHmcRowsCall& c, int st);       // st: of the same predicate
hipError_t lsnf_launch_small3_reverse_hmc_metric(const LsnfReverseHmcMetricCall& c, int st);   // st: of the same predicate
hipError_t lsnf_launch_small3_reverse_hmc_tempered(const LsnfReverseHmcTemperedCall& c, int st);   // st: of the same predicate
hipError_t lsnf_launch_small3_reverse_hmc_exchange(const LsnfReverseHmcExchangeCall& c, int st);   // st: of the same predicate
hipError_t lsnf_launch_small3_reverse_hmc_resample(const LsnfReverseHmcResampleCall& c, int st);   // st: of the same predicate
hipError_t lsnf_launch_small3_reverse_hmc_schedule(const LsnfReverseHmcScheduleCall& c, int st);   // st: of the same predicate

bool lsnf_contract_x3_covers(const LsnfContractCall& c);                   // (also asked with NULL tensors: lsnf_api.hip dump_may_tile)
hipError_t lsnf_launch_contract_x3(const LsnfContractCall& c, int chunk_override);
hipError_t lsnf_launch_params_contract(const LsnfContractCall& c, int contraction);       // contraction: LsnfContraction

// ---- shared host helpers ---------------------------------------------------------------------------------------------
// Kernels that use more than 64 KiB of dynamic LDS need the attribute set once PER DEVICE of the process.
inline hipError_t lsnf_allow_big_lds(const void* kernel, unsigned long long* done_mask) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && ((*done_mask >> dev) & 1ull)) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) *done_mask |= 1ull << dev;      // benign race: the call is idempotent
    return hipSuccess;
}
// THE launch: the LDS attribute at most once per kernel instantiation (the template argument) and device, the launch, its error.
template <auto Kern, class Args>
hipError_t lsnf_launch_kernel(dim3 grid, unsigned threads, size_t lds, hipStream_t stream, const Args& a) {
    static unsigned long long lds_ok = 0;
    if (hipError_t e = lsnf_allow_big_lds((const void*)Kern, &lds_ok); e != hipSuccess) return e;
    hipLaunchKernelGGL(Kern, grid, dim3(threads), lds, stream, a);
    return hipGetLastError();
}
inline unsigned lsnf_grid(int B, int rows_per_workgroup) { return (unsigned)((B + rows_per_workgroup - 1) / rows_per_workgroup); }

// f(Cfg<HT, WT>{}) for the kernel instantiation of the geometry (lsnf_pick_tiles: (1,1), (2,2) or (2,4)).
template <template <int, int> class Cfg, class F>
inline auto lsnf_with_cfg(const LsnfGeo& g, F&& f) {
    if (g.HT == 1) return f(Cfg<1, 1>{});
    if (g.WT == 2) return f(Cfg<2, 2>{});
    return f(Cfg<2, 4>{});
}
// f(integral_constant<int, ST>{}) for the rows per workgroup / 16 of a latency kernel
template <class F>
inline auto lsnf_with_st(int st, F&& f) {
    return st == 4 ? f(std::integral_constant<int, 4>{}) : st == 2 ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 1>{});
}
// Rows per workgroup / 16 the latency kernels WANT, by batch size: 16 rows while one round of workgroups covers the batch (<= 256
// CUs x 16 rows), then 32, then 64 -- the weight stream per workgroup is the same, so a second round costs a whole stream while a
// second sample tile costs its MFMAs only.  LSNF_SMALL3_ST (1 / 2 / 4) forces a shape (experiments, tests).  Each kernel then gives
// way to the next smaller shape it has.
inline int lsnf_small3_st_wanted(int B) {
    static const char* env = getenv("LSNF_SMALL3_ST");
    return env ? atoi(env) : (B <= 256 * 16 ? 1 : (B <= 256 * 32 ? 2 : 4));
}
// 8 waves (256-row workgroups) or 4 for the bf16 throughput kernels: 256-row workgroups need B > 32 768 to put one on (almost)
// every CU; below that 128-row workgroups use twice the CUs.  LSNF_FORCE_WAVES (4 / 8): experiment knob of tools/.
inline bool lsnf_eight_waves(int B) {
    static const char* fw = getenv("LSNF_FORCE_WAVES");
    return fw ? atoi(fw) == 8 : B > 128 * 256;
}

// Plan regions and caller tensors at first_block of a forward call (NULL stays NULL).
inline const float* lsnf_fwd_consts_at(const LsnfForwardCall& c) { return c.plan + c.g.off_fwd_const + (size_t)c.first_block * c.g.fwd_const_floats; }
inline const float* lsnf_fwd_panels_at(const LsnfForwardCall& c) { return c.plan + c.g.off_fwd_panels + (size_t)c.first_block * c.g.fwd_block_floats; }
inline const float* lsnf_f3b_panels_at(const LsnfForwardCall& c) { return c.plan + c.g.off_f3b_panels + (size_t)c.first_block * c.g.f3_block_floats; }
inline const float* lsnf_f2h_panels_at(const LsnfForwardCall& c) { return c.plan + c.g.off_f2h_panels + (size_t)c.first_block * c.g.f2h_block_floats; }
inline float* lsnf_act_saved_at(const LsnfForwardCall& c) {
    return c.act_saved ? c.act_saved + (size_t)c.first_block * lsnf_act_layout(c.B, c.g.HT, c.g.WT).per_block : nullptr;
}
inline float* lsnf_hdump_at(const LsnfForwardCall& c) {
    return c.hdump ? c.hdump + (size_t)c.first_block * lsnf_dump_layout(c.B, c.g.nz, c.g.width).per_block : nullptr;
}
inline const unsigned* lsnf_guard_words(const LsnfCall& c) { return reinterpret_cast<const unsigned*>(c.plan + c.g.off_guard); }

// What the kernel-argument structs of an operation have in common, from its descriptor; the caller adds its panels and extras.
template <class A>
inline void lsnf_fill_forward(A& a, const LsnfForwardCall& c) {
    a.consts = lsnf_fwd_consts_at(c);
    a.z_in = c.z_in; a.objective = c.objective; a.z_out = c.z_out; a.logdet_out = c.logdet_out; a.ll_out = c.ll_out;
    a.z_saved = c.z_saved; a.act_saved = lsnf_act_saved_at(c); a.stats = c.stats;
    a.B = c.B; a.nz = c.g.nz; a.half = c.g.half; a.n_blocks = c.n_blocks; a.vec4 = c.vec4;
}
template <class A>
inline void lsnf_fill_reverse(A& a, const LsnfReverseCall& c) {
    a.fwd_consts = c.plan + c.g.off_fwd_const; a.inv_consts = c.plan + c.g.off_inv_const;
    a.z_in = c.z_in; a.objective = c.objective; a.z_out = c.z_out; a.objective_out = c.objective_out;
    a.B = c.B; a.nz = c.g.nz; a.half = c.g.half; a.depth = c.g.depth; a.vec4 = c.vec4;
}
// f(true_type, a) for the sampling form (a.s set), f(false_type, a's plain base) otherwise: the kernels' argument types
template <class Plain, class Sample, class F>
inline hipError_t lsnf_with_sample(Sample& a, const LsnfSampleArgs* smp, F&& f) {
    if (smp) { a.s = *smp; return f(std::true_type{}, a); }
    return f(std::false_type{}, static_cast<const Plain&>(a));
}
// the Langevin tail of a backward (lv == NULL: no update, all of it NULL / 0)
template <class A>
inline void lsnf_fill_langevin(A& a, const LsnfLangevinArgs* lv) {
    static const LsnfLangevinArgs none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, LsnfRngArgs{0ull, 0ull, nullptr, 0ll, 0}};
    const LsnfLangevinArgs& l = lv ? *lv : none;
    a.z_cur = l.z_cur; a.grad_g = l.grad_g; a.noise = l.noise; a.z_new = l.z_new; a.gf_norm = l.gf_norm; a.gg_norm = l.gg_norm;
    a.step = l.step; a.rng = l.rng;
}
template <class A>
inline void lsnf_fill_backward(A& a, const LsnfBackwardCall& c) {
    a.z_out = c.z_out; a.z_saved = c.z_saved; a.act_saved = c.act_saved; a.g_z1 = c.g_z1; a.g_logdet = c.g_logdet; a.g_z_in = c.g_z_in;
    a.dump = c.dump; a.gl_total = c.gl_total; a.width = c.g.width;
    lsnf_fill_langevin(a, c.lv);
    a.ll_scale = c.ll_scale; a.ll_mode = c.ll_mode; a.B = c.B; a.nz = c.g.nz; a.half = c.g.half; a.depth = c.g.depth; a.vec4 = c.vec4;
}
// the chain state of a Metropolis-adjusted form, but for the accepted points: the caller stores ch.acc under its kernel's name for them
template <class A>
inline void lsnf_fill_chain(A& a, const LsnfChainArgs& ch) {
    a.energy_g = ch.energy_g; a.uniform = ch.uniform; a.grad_acc = ch.grad_acc; a.u_acc = ch.u_acc;
    a.accept_out = ch.accept_out; a.log_alpha_out = ch.log_alpha_out; a.flags = ch.flags;
}
// the MALA form of the latency bf16x3 backward (Small3MalaArgs and what derives from it)
template <class A>
inline void lsnf_fill_mala(A& a, const LsnfMalaCall& c) {
    lsnf_fill_backward(a, c);
    a.panels = c.plan + c.g.off_b3b_panels;
    a.ll_prop = c.ll_prop; a.z_acc = c.chain.acc;
    lsnf_fill_chain(a, c.chain);
}

/*
 * lsnf_flow.h -- C ABI of the MI355X (gfx950) latent-flow-prior library `liblsnf_flow.so`.
 *
 * The reference (jianwen-xie/Latent-Space-Normalizing-Flow) has no native/FFI layer: its
 * replaceable unit is the Python class `_netF` (reference model.py:460-498).  This header is
 * the boundary a maintainer binds from Python (ctypes) to make `_netF`
 * run on hand-written HIP kernels.  Every entry point names the reference code it replaces.
 *
 * Conventions
 *   - plain C: pointers + sizes only, no torch / STL types.
 *   - every `const float*` / `float*` below is a DEVICE pointer (HBM) unless the name ends
 *     in `_host`; tensors are dense row-major fp32: z is (B, nz), per-sample vectors are (B,).
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the null stream).  Calls are
 *     asynchronous, do not synchronise the device and write only the buffers named as outputs
 *     (the plan is read-only after lsnf_prepare), so they are re-entrant per stream and
 *     hipGraph-capturable (no allocation inside).  The only process-wide state are the two
 *     tuning knobs below (lsnf_set_small_batch_max, lsnf_set_math_mode): atomics, read once per call.
 *   - return value: 0 on success, a negative LSNF_E_* code on failure; `lsnf_last_error()`
 *     returns a thread-local message.  Nothing falls back to a CPU path.
 *
 * Geometry: nz even, 2 <= nz <= 128; 1 <= width <= 128; 1 <= depth <= 16;
 * coupling 1 (affine, reference default train.py:63) or 0 (additive, model.py:407-408; runs on the
 * affine kernels with a neutral scale path, i.e. ~12 % more MFMA work than strictly needed).
 */
#ifndef LSNF_FLOW_H
#define LSNF_FLOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSNF_ABI_VERSION 5

#define LSNF_OK 0
#define LSNF_E_ARG (-1)       /* bad argument (NULL pointer, size out of range, misaligned) */
#define LSNF_E_GEOMETRY (-2)  /* nz / width / depth outside what the kernels are built for */
#define LSNF_E_HIP (-3)       /* a HIP runtime call or kernel launch failed */
#define LSNF_E_NODEVICE (-4)  /* no gfx950 device visible */

/* Number of live parameter tensors per coupling block, in this order (names as in the
 * reference's state_dict, prefix `revnet2d_s.0.revnet2d_step_s.{i}.`; shapes row-major):
 *   0 actnorm.b            (nz)         model.py:230
 *   1 actnorm.logs         (nz)         model.py:233
 *   2 invertible_1x1_conv.w(nz, nz)     model.py:177
 *   3 f.fc_1.w             (nz/2, w)    model.py:318
 *   4 f.fc_1.actnorm.b     (w)
 *   5 f.fc_1.actnorm.logs  (w)
 *   6 f.fc_2.w             (w, w)
 *   7 f.fc_2.actnorm.b     (w)
 *   8 f.fc_2.actnorm.logs  (w)
 *   9 f.fc_zeros.w         (w, n_out)   model.py:340   n_out = nz (affine) | nz/2 (additive)
 *  10 f.fc_zeros.b         (n_out)      model.py:341
 *  11 f.fc_zeros.logs      (n_out)      model.py:342
 * (`f.fc_1.b`, `f.fc_2.b` are dead parameters in the reference, model.py:319,327-330, and the
 * `.bias` keys alias `.b`, model.py:231: none of them cross this boundary.) */
#define LSNF_PARAMS_PER_BLOCK 12

int lsnf_abi_version(void);
const char* lsnf_last_error(void);

/* Tuning knob: batches of at most `rows` rows run on the small-batch (latency) kernels, larger ones on the
 * throughput kernels; both compute the same function (results agree to fp32 rounding, not bit for bit).  ONE threshold
 * for every entry point, so the kernel family that writes an activation stash is the one that reads it.
 *   rows >= 0                 : set the threshold (0 disables the latency kernels); returns the previous SETTING
 *   LSNF_SMALL_BATCH_AUTO (-2): back to the built-in crossover of the arithmetic mode in force (16384 rows; 12288 in
 *                               LSNF_MATH_FP16X2) -- the initial state unless the LSNF_SMALL_MAX environment variable is set;
 *                               returns the previous setting
 *   -1                        : query only: returns the threshold in force (a row count)
 * "previous setting" is a row count or LSNF_SMALL_BATCH_AUTO, so `prev = set(x); ...; set(prev)` restores exactly.
 * Under LSNF_SMALL_BATCH_AUTO one kind of call has its own crossover: lsnf_forward WITHOUT z_saved / act_saved in
 * LSNF_MATH_BF16X3 at nz in 66..128, f_width <= 64 switches to the (software-pipelined) throughput kernel above 8192 rows. */
#define LSNF_SMALL_BATCH_AUTO (-2)
int lsnf_set_small_batch_max(int rows);

/* Arithmetic of the GEMMs.  Affects the forward, the backward and the reverse (both kernel families); the parameter-
 * gradient contraction over the batch is fp32 MFMA in every mode:
 *   LSNF_MATH_BF16X3 : (default) both operands split error-free into three bf16 terms (3 x 8 = 24 significand bits,
 *                      fp32's exponent range), six bf16 MFMAs per product with fp32 accumulation, on
 *                      v_mfma_f32_16x16x32_bf16.  Same accuracy class as fp32 MFMA (dropped terms <= 2^-26 |w||x|);
 *                      results agree with LSNF_MATH_FP32 to fp32 rounding, not bit for bit.  Throughput forward calls
 *                      without stash / parameter-gradient dump at nz in 66..128, f_width <= 64 run lsnf_fwd3q_kernel
 *                      (csrc/lsnf_fwd3p.hip: operand split and coupling epilogue software-pipelined between the MFMAs),
 *                      everything else csrc/lsnf_fwd3.hip (separate split / MFMA / epilogue phases).
 *   LSNF_MATH_BF16X3_PHASED : as LSNF_MATH_BF16X3 with every throughput forward on csrc/lsnf_fwd3.hip (comparison, tests).
 *   LSNF_MATH_FP32   : fp32 MFMA (v_mfma_f32_32x32x2_f32) everywhere.
 *   LSNF_MATH_FP16X2 : (opt-in; NARROWER than the reference's fp32: 11 + 11 operand bits) throughput forward and reverse
 *                      with both operands split into two fp16 terms, three fp16 MFMAs per product (csrc/lsnf_fwd2h.hip;
 *                      dropped terms <= 2^-22 |w||x|; operands below 2^-3 in magnitude additionally carry an ABSOLUTE
 *                      error of up to 2^-25, because their second term falls into fp16's subnormals -- relative accuracy
 *                      of small-magnitude latents and their gradients is not fp32's); half the matrix work of
 *                      LSNF_MATH_BF16X3.  fp16's range is
 *                      guarded: a wave that meets an operand (or folded weight) at or beyond 65504 flags its first output
 *                      element, and the LSNF_MATH_BF16X3 kernel queued behind the launch recomputes the flagged
 *                      workgroups (an early-exit launch otherwise), so results are finite wherever the fp32
 *                      computation's are.  In-place calls (an output aliases an input: z_out == z_in, or logdet_out /
 *                      objective_out == objective -- the fix-up pass re-reads both inputs) and calls with in-kernel batch
 *                      sums (`stats`) run LSNF_MATH_BF16X3 directly (the phase-separated lsnf_fwd3b_kernel / lsnf_rev3_kernel).
 *                      Every other kernel (latency kernels, backward) as LSNF_MATH_BF16X3.
 * mode < 0 only queries.  Returns the previous mode (default LSNF_MATH_DEFAULT, or the LSNF_MATH environment
 * variable "fp32" / "bf16x3" / "bf16x3_phased" / "fp16x2").  Other values are refused. */
#define LSNF_MATH_FP32 0
#define LSNF_MATH_BF16X3 1
#define LSNF_MATH_FP16X2 3
#define LSNF_MATH_BF16X3_PHASED 5
#define LSNF_MATH_DEFAULT LSNF_MATH_BF16X3
int lsnf_set_math_mode(int mode);

/* Device query: writes the gfx arch name (e.g. "gfx950") of device `device`; LSNF_E_NODEVICE
 * if there is none.  Only call that touches the device without doing work. */
int lsnf_device_arch(int device, char* buf, size_t buflen);

/* ---- prepared weights ("plan") ---------------------------------------------------------
 * Batch-independent work of one `_netF` evaluation, hoisted out of the per-call path:
 * exp(3*logs) folding of the three actnorms (model.py:264-268), de-interleave of fc_zeros'
 * shift / scale columns (model.py:411-413), log|det W| in float64 (model.py:182), W^-1
 * (model.py:193), all re-laid-out in MFMA-fragment order.  Valid until a parameter changes.
 * Written by lsnf_prepare only: every other entry point reads it (`const float* plan` means const), so one plan may be
 * shared by any number of streams and captured graphs.  Do not share one plan buffer between devices. */

/* Size in floats of the prepared-weight buffer for this geometry (0 on bad geometry). */
size_t lsnf_plan_floats(int nz, int width, int depth, int coupling);

/* Size in bytes of the scratch `lsnf_prepare` needs (float64 LU workspace). */
size_t lsnf_prepare_scratch_bytes(int nz, int width, int depth);

/* params_host: HOST array of depth*LSNF_PARAMS_PER_BLOCK DEVICE pointers (order above).
 * plan: device buffer of lsnf_plan_floats() floats, 16-byte aligned.  scratch: device. */
int lsnf_prepare(const float* const* params_host, int nz, int width, int depth, int coupling,
                 float* plan, void* scratch, void* stream);

/* ---- data-dependent actnorm init: replaces `_netF.forward(z, objective, init=True)`'s parameter writes ---------
 * (actnorm_center / actnorm_scale with init=True, model.py:238-241,253-262, threaded through revnet2d_step.forward
 * model.py:389-422 and fc.forward model.py:324-331; Glow's initialisation).  For block k in order, on that block's input
 * (z_in for k = 0, else block k-1's output under its NEW parameters): block actnorm b := -mean x, logs := log(1 / (sqrt(
 * mean (x+b)^2) + 1e-6)) / 3; then the same for fc_1.actnorm on y[:, :nz/2] @ fc_1.w and for fc_2.actnorm on
 * relu(fc_1 actnorm) @ fc_2.w.  Writes tensors 0, 1, 4, 5, 7, 8 of every block IN PLACE (params_host: same order as
 * lsnf_prepare's array); reads the other six.  fp32 products (FMA), fp64 batch statistics from per-workgroup partial sums
 * reduced in a fixed order (no atomics): bit-for-bit reproducible, and independent of the two tuning knobs and of the
 * actnorm values the call starts from.  B >= 1 (B = 1 gives b = -z, logs = log(1e6)/3).
 * workspace: device, 16-byte aligned, lsnf_actnorm_init_workspace_bytes() bytes (0 on bad geometry or B < 1).
 * Plans prepared before the call are stale afterwards: run lsnf_prepare again. */
size_t lsnf_actnorm_init_workspace_bytes(int nz, int width, int depth, int coupling, int B);
int lsnf_actnorm_init(float* const* params_host, int nz, int width, int depth, int coupling, int B,
                      const float* z_in, void* workspace, void* stream);

/* ---- forward: replaces `_netF.forward(z, objective)` (model.py:473-483) -----------------
 * Runs blocks [first_block, first_block+n_blocks) of the stack (model.py:357-360; one block =
 * revnet2d_step.forward model.py:391-422) on B rows in ONE launch.
 *   z_in      (B, nz)   input latents
 *   objective (B) or NULL (= zeros)      running log-det in
 *   z_out     (B, nz)   output of the last block run; may be z_in itself (in-place call)
 *   logdet_out(B)       objective + sum of the blocks' log|det J|; may be objective itself
 *   ll_out    (B) or NULL: -0.5*sum_j z_out^2 + log(2*pi) + logdet_out  (train.py:317-319)
 *   z_saved   NULL, or ((n_blocks-1), B, nz): outputs of all but the last block, kept for
 *             lsnf_backward_z / lsnf_backward_params.
 *   act_saved NULL, or lsnf_act_saved_floats(nz,width,depth,B) floats (16-byte aligned): opaque stash of
 *             what autograd would keep besides the block outputs (the coupling's sigmoid and the two
 *             relu masks, model.py:307-308,415), indexed by absolute block.  Handing it to
 *             lsnf_backward_z / lsnf_langevin_step removes their recomputation of the coupling MLP.
 *   params_workspace NULL, or the workspace of the lsnf_backward_params call that will follow for this evaluation
 *             (lsnf_backward_params_workspace_floats(), 16-byte aligned): the forward then also writes the hidden
 *             activations h1, h2 of every block into it, which lets lsnf_backward_params run FROM THE STASH instead of
 *             recomputing the coupling MLP.  Whole stack only, with act_saved and z_saved; needs a bf16x3-family math
 *             mode (lsnf_params_fast_path() == 1, LSNF_E_ARG otherwise).  Where the large-batch kernels may write the
 *             dump tiled (math mode LSNF_MATH_BF16X3 or LSNF_MATH_BF16X3_PHASED, B > the small-batch threshold,
 *             B >= 12 288, nz a multiple of 64, width of 16, both <= 128) z_in, z_out and z_saved must be 16-byte
 *             aligned (LSNF_E_ARG otherwise; lsnf_backward_params applies the same rule).
 *   stats     NULL, or LSNF_STATS_DOUBLES doubles (device, 8-byte aligned) that the caller zero-initialises ONCE:
 *             after the launch stats[4] = sum_b ll_b (train.py:320), stats[5] = sum_b logdet_b,
 *             stats[6] = B.  Summed inside the kernel (fp64 atomics, one pair per workgroup, into 64
 *             sub-accumulators stats[8..]; tickets find the last workgroup, which reads them all, publishes and
 *             re-arms them; everything but stats[4..6] is internal and back at zero after the launch).
 *             One stats buffer must not be shared by launches on different streams.            */
#define LSNF_STATS_DOUBLES 264
int lsnf_forward(const float* plan, int nz, int width, int depth, int coupling,
                 int first_block, int n_blocks, int B,
                 const float* z_in, const float* objective,
                 float* z_out, float* logdet_out, float* ll_out, float* z_saved,
                 float* act_saved, float* params_workspace, double* stats, void* stream);

/* floats of lsnf_forward's optional activation stash for a batch of B rows (0 on bad geometry) */
size_t lsnf_act_saved_floats(int nz, int width, int depth, int B);

/* ---- reverse: replaces `_netF.forward(z, objective, reverse=True)` (model.py:484-498,
 * block inverse model.py:424-456).  Functional: inputs are not modified (the reference
 * mutates them in place, model.py:436-438) unless the caller aliases them: z_out may be z_in and
 * objective_out may be objective (in-place call).  objective (B) or NULL (= zeros);
 * objective_out = objective - sum log|det J|
 * (the reference returns its negation when return_obj=True, model.py:498). */
int lsnf_reverse(const float* plan, int nz, int width, int depth, int coupling, int B,
                 const float* z_in, const float* objective,
                 float* z_out, float* objective_out, void* stream);

/* ---- backward w.r.t. z: replaces autograd of train.py:316-323 ---------------------------
 * Given upstream gradients g_z1 = dL/dz_out (B,nz) (NULL = 0), g_logdet = dL/dlogdet_out
 * (B) (NULL = 0) computes g_z_in = dL/dz_in (B,nz).  z_out / z_saved are what lsnf_forward
 * wrote for the same inputs (full stack: first_block = 0, n_blocks = depth); act_saved is
 * NULL (the coupling MLP is recomputed from z_saved) or the stash that forward filled.
 * If ll_mode != 0 the upstream gradient is that of L = ll_scale * sum_b ll_b, i.e.
 * g_z1 = -ll_scale*z_out, g_logdet = ll_scale, and the two pointers are ignored
 * (train.py:320 uses L = -sum ll -> ll_scale = -1). */
int lsnf_backward_z(const float* plan, int nz, int width, int depth, int coupling, int B,
                    const float* z_out, const float* z_saved, const float* act_saved,
                    const float* g_z1, const float* g_logdet, int ll_mode, float ll_scale,
                    float* g_z_in, void* stream);

/* ---- backward of lsnf_reverse w.r.t. its inputs (autograd through the sampling direction, model.py:484-498) ----
 * With f the forward stack, x = f^-1(y) = the z_out of lsnf_reverse and objective_out = objective - logdet_f(x):
 *     g_z_in = J_f(x)^-T (g_x - g_objective * grad_x logdet_f(x)),      dL/d objective = g_objective itself.
 * z_out / z_saved / act_saved: what lsnf_forward (whole stack, with the stash) wrote when run on x; act_saved is required
 * (lsnf_restash can rebuild it) and may come from any kernel family / math mode.
 * g_x = dL/dx (B,nz) or NULL (= 0); g_objective = dL/d objective_out (B) or NULL (= 0); g_z_in (B,nz) may be g_x itself.
 * The parameter gradients of the reverse need no entry point of their own: they are lsnf_backward_params of the FORWARD
 * evaluated at x with upstream gradients g_z1 = -g_z_in, g_logdet = -g_objective (implicit-function theorem).
 * One kernel and one arithmetic (bf16x3, not narrower than fp32) under every lsnf_set_math_mode and for every B;
 * lsnf_set_small_batch_max does not affect it. */
int lsnf_reverse_backward_z(const float* plan, int nz, int width, int depth, int coupling, int B,
                            const float* z_out, const float* z_saved, const float* act_saved,
                            const float* g_x, const float* g_objective, float* g_z_in, void* stream);

/* The activation stash of a forward that was run WITHOUT one (act_saved = NULL), rebuilt from its block outputs: the
 * coupling MLP's input is the first half of the block's output (model.py:422), so sigmoid(p) and the two ReLU masks follow
 * from z_out / z_saved alone (S2, S3 and the pre-sigmoid half of S4 per block; blocks in parallel).  lsnf_restash + the
 * from-the-stash lsnf_backward_z replace the recomputing backward on the bf16 matrix pipe; the ABI allocates nothing, so
 * the caller owns the stash (lsnf_act_saved_floats).  Needs a bf16x3-family math mode (LSNF_E_ARG otherwise). */
int lsnf_restash(const float* plan, int nz, int width, int depth, int coupling, int B,
                 const float* z_out, const float* z_saved, float* act_saved, void* stream);

/* ---- fused Langevin update: replaces train.py:317-329 after the forward ---------------------
 * One launch computes g_f = d(-sum ll)/dz (as lsnf_backward_z with ll_mode=1, ll_scale=-1) and applies
 *     z_new = z_cur - 0.5*s^2 * (grad_g + g_f) + s * noise          (train.py:324,326)
 * plus the per-sample gradient norms of train.py:328-329 (the caller takes their mean).
 *   z_cur  (B,nz) current latents (the z that lsnf_forward was run on); z_out / z_saved / act_saved
 *          (act_saved may be NULL) from that forward
 *   grad_g (B,nz) or NULL (= 0): the generator's gradient z_grad_g (train.py:314)
 *   noise  (B,nz) or NULL: N(0,1) draws supplied by the caller (train.py:326 `randn_like`)
 *   rng    NULL, or (only when noise is NULL) the in-kernel generator below; both NULL = no noise, as the
 *          test-time sampler (train.py:624-625)
 *   z_new  (B,nz), may alias z_cur (in-place update);  gf_norm, gg_norm: (B) or NULL. */
typedef struct LsnfRng {
    /* Counter-based N(0,1) noise made inside the update kernel: Philox4x32-10 + Box-Muller, a pure function of
     * (seed, offset, global row, column) -- the same draw whatever the batch size, kernel family or sharding of
     * the rows over GPUs (exact definition: csrc/lsnf_device.h lsnf_noise_tile, restated in
     * oracle/philox_oracle.py).  Use a new `offset` for every Langevin step. */
    unsigned long long seed;
    unsigned long long offset;
    const unsigned long long* offset_dev;   /* NULL, or device counter added to offset (captured graphs) */
    long long row0;                         /* global index of this call's row 0 (sharded chains); usually 0 */
} LsnfRng;

int lsnf_langevin_step(const float* plan, int nz, int width, int depth, int coupling, int B,
                       const float* z_cur, const float* z_out, const float* z_saved, const float* act_saved,
                       const float* grad_g, const float* noise, const LsnfRng* rng, float step_size,
                       float* z_new, float* gf_norm, float* gg_norm, void* stream);

/* ---- fused prior sampling: replaces `sample_x`'s `torch.randn` + `_netF.forward(z, zeros, reverse=True)` ----
 * (train.py:428-434, 472-478, 567-574).  ONE launch of the lsnf_reverse kernel the batch size selects, in a form that DRAWS its
 * input rows where lsnf_reverse loads them:
 *     eps[b][c] = temperature * xi(seed, offset (+ *offset_dev), row0 + b, c)
 * with xi exactly the N(0,1) draw of lsnf_langevin_step (LsnfRng above; oracle/philox_oracle.py) and the product one fp32
 * multiply.  A pure function of (seed, offset, global row, column): the same rows whatever B, the kernel family, the math mode
 * or the sharding -- a rank that samples rows [r0, r1) of a global batch passes row0 = r0, B = r1 - r0 and gets the bits the
 * one-GPU call has there (in z_out / objective_out / ll_out too, when both calls select the same kernel).
 *   rng          required; row0 >= 0; offset_dev NULL or an 8-byte aligned device counter (captured graphs).  Not modified:
 *                use a new offset for every call.
 *   temperature  finite and >= 0 (the `temp` of train.py:429); 0 gives the flow's image of the origin in every row
 *   z_out        (B, nz)  x = f^-1(eps): what lsnf_reverse(z_in = eps, objective = NULL) writes, bit for bit
 *   objective_out(B) or NULL: -logdet_f(x), lsnf_reverse's bits
 *   eps_out      (B, nz) or NULL: the drawn rows; must not be z_out
 *   ll_out       (B) or NULL: -0.5*sum_c eps^2 + log(2*pi) - objective_out = log p(x) under the flow prior: lsnf_forward's ll_out
 *                at x with z1 = eps and logdet = logdet_f(x), without the second pass
 * Selection, math modes and the fp16x2 fix-up pass as lsnf_reverse (the fix-up pass redraws the rows of the workgroups it
 * recomputes).  B = 0 succeeds without a launch.  Anything else outside these rules: LSNF_E_ARG.
 * Added without an ABI bump (a new symbol; nothing existing changed). */
int lsnf_sample(const float* plan, int nz, int width, int depth, int coupling, int B,
                const LsnfRng* rng, float temperature,
                float* z_out, float* objective_out, float* eps_out, float* ll_out, void* stream);

/* ---- stash-keeping reverse / sampling: the sampling direction leaves what its own backward needs ----
 * lsnf_reverse_keep / lsnf_sample_keep are lsnf_reverse / lsnf_sample -- same kernel, same bits in z_out, objective_out (eps_out,
 * ll_out) -- that ALSO write, each only if its pointer is not NULL, what lsnf_forward(z_in = x, whole stack) would keep for a
 * backward pass at x = z_out: the coupling MLP's input is the first half of a block's OUTPUT (model.py:422), so the reverse holds the
 * forward's block outputs, sigmoid and ReLU masks in registers when it produces x.
 *   z_saved          ((depth-1), B, nz): outputs of forward blocks 0 .. depth-2 at x (the last block's output is the call's own
 *                    input, z_in / eps_out, and is not written again); must not alias another tensor of the call
 *   act_saved        lsnf_act_saved_floats() floats, 16-byte aligned: the stash, in lsnf_forward's layout
 *   params_workspace the workspace of the lsnf_backward_params call that will follow (16-byte aligned): h1 / h2 of every block, as
 *                    lsnf_forward(params_workspace) leaves them; needs act_saved, z_saved (depth > 1) and
 *                    lsnf_params_fast_path() == 1
 * lsnf_reverse_backward_z(z_out = z_in / eps_out, z_saved, act_saved, ...), lsnf_backward_z and lsnf_backward_params(z_in = x,
 * z_out = z_in / eps_out, z_saved, act_saved, workspace) take them as they take lsnf_forward's: the second pass over x is not needed.
 * lsnf_sample_keep with act_saved or z_saved requires eps_out.  lsnf_reverse_keep with act_saved or z_saved refuses the in-place call
 * z_out == z_in: it would overwrite the last block's output, which every backward must be given.  Other rules (NULL, alignment,
 * aliasing) as lsnf_reverse / lsnf_sample.
 * Covered: the latency bf16x3 reverse only -- a bf16x3-family math mode (lsnf_params_fast_path() == 1), B <= the small-batch
 * threshold in force (lsnf_set_small_batch_max(-1)) and a geometry / depth that kernel takes; lsnf_reverse_keep_covers() answers
 * 1 / 0 for a call (0 on a bad geometry), and outside it both entry points return LSNF_E_ARG (not covered: the throughput reverse
 * kernels, LSNF_MATH_FP32).  B = 0 succeeds without a launch.  Added without an ABI bump (new symbols; nothing existing changed). */
int lsnf_reverse_keep_covers(int nz, int width, int depth, int coupling, int B);
int lsnf_reverse_keep(const float* plan, int nz, int width, int depth, int coupling, int B,
                      const float* z_in, const float* objective, float* z_out, float* objective_out,
                      float* z_saved, float* act_saved, float* params_workspace, void* stream);
int lsnf_sample_keep(const float* plan, int nz, int width, int depth, int coupling, int B,
                     const LsnfRng* rng, float temperature,
                     float* z_out, float* objective_out, float* eps_out, float* ll_out,
                     float* z_saved, float* act_saved, float* params_workspace, void* stream);

/* ---- fused Langevin update in the base space: eps-space Langevin with x = f^-1(eps) ----
 * lsnf_reverse_backward_z with the update as its output section, one launch.  With g = J_{f^-1}(eps)^T grad_g (the bits of
 * lsnf_reverse_backward_z(g_x = grad_g, g_objective = NULL)) it computes per element, in this order, every step one fp32 rounding:
 *     coef = 0.5f * step_size * step_size
 *     t    = eps + g                        (g = 0 where grad_g is NULL: the same bits as explicit zeros)
 *     u    = fma(-coef, t, eps)             = eps - coef * t
 *     new  = fma(step_size, xi, u)          = u + step_size * xi      (only when noise or rng is given; new = u otherwise)
 * xi is the row of `noise`, or the N(0,1) draw of LsnfRng above -- lsnf_langevin_step's and lsnf_sample's draw (at temperature 1
 * lsnf_sample's eps_out IS xi), through the same instructions as a loaded xi: the two agree bit for bit.
 *   z_out        (B, nz) eps, the reverse's input = the last forward block's output; z_saved / act_saved as for
 *                lsnf_reverse_backward_z: from lsnf_forward at x, lsnf_restash, or lsnf_reverse_keep / lsnf_sample_keep
 *   grad_g       (B, nz) dL/dx, or NULL
 *   noise / rng  both NULL: no noise; rng only when noise is NULL; rng->row0 >= 0, offset_dev NULL or 8-byte aligned
 *   step_size    finite
 *   eps_new      (B, nz), required; may be z_out itself (the in-place step: every read of a workgroup's rows precedes its stores,
 *                rows are workgroup-private); must not be grad_g, noise, z_saved or g_eps_out
 *   g_eps_out    (B, nz) or NULL: g; may be grad_g; must not be noise, z_out or z_saved
 *   g_norm       (B) or NULL: ||g||_2 per row;   eps_norm (B) or NULL: ||eps||_2 per row (of the input); neither may be
 *                another tensor of the call (nor each other).  Every forbidden alias is LSNF_E_ARG.
 * Alignment as lsnf_reverse_backward_z (plan and act_saved 16 bytes, tensors 4; the vector width follows the pointers).  A row's
 * result does not depend on B, on the workgroup shape or on row0 sharding.  One kernel under every lsnf_set_math_mode and for every
 * B.  B = 0 succeeds without a launch.  Added without an ABI bump (a new symbol; nothing existing changed). */
int lsnf_reverse_langevin_step(const float* plan, int nz, int width, int depth, int coupling, int B,
                               const float* z_out, const float* z_saved, const float* act_saved,
                               const float* grad_g, const float* noise, const LsnfRng* rng, float step_size,
                               float* eps_new, float* g_eps_out, float* g_norm, float* eps_norm, void* stream);

/* ---- backward w.r.t. the parameters: replaces `loss_f.backward()` (train.py:406-411) --------
 * Gradients of L w.r.t. the 12 live tensors of every block (same order as lsnf_prepare), for the
 * upstream gradients described under lsnf_backward_z (train.py:410: L = -mean ll -> ll_mode=1,
 * ll_scale = -1/B).  Includes d log|det W|/dW = W^-T (model.py:182) and the actnorm log-det terms.
 *   params_host : HOST array of depth*12 DEVICE pointers to the raw parameters (read only)
 *   grads_host  : HOST array of depth*12 DEVICE pointers that receive the gradients (a NULL entry
 *                 skips that tensor); shapes as the parameters
 *   z_in        : (B, nz) input of the stack; z_out / z_saved as written by lsnf_forward
 *   act_saved   : NULL -- the backward recomputes the coupling MLP (fp32 MFMA) -- or the stash of the lsnf_forward call of
 *                 this evaluation, which must then ALSO have been given `params_workspace` = this call's `workspace`
 *                 (fast path: backward from the stash on the bf16 matrix pipe, nothing recomputed; same math mode and
 *                 small-batch threshold in force for both calls; ignored when lsnf_params_fast_path() == 0)
 *   g_z_in      : NULL, or (B, nz) to also receive dL/dz_in (same values as lsnf_backward_z)
 *   workspace   : lsnf_backward_params_workspace_floats() floats, 16-byte aligned.  Opaque between the two calls of the fast path
 *                 (the forward records there in which form it left h1 / h2: from 12 288 rows the batch contraction runs on the bf16
 *                 matrix pipe and the large-batch kernels write their arrays tiled); pass the forward's own z_in / z_out / z_saved.
 *                 Where the dump may be tiled (see params_workspace under lsnf_forward) the fast path refuses z tensors that are
 *                 not 16-byte aligned with LSNF_E_ARG, as that forward does: the two calls then always agree on the dump's form.
 * Sums over the batch use fp32 atomics above 128 rows, and G = sum_b dL/dlogdet_b float64 atomics above one workgroup of rows
 * (order, hence last bits, may vary run to run: tests/test_gpu_module.py bounds the spread at B = 65 536 to 2e-6 of each
 * tensor's norm).  lsnf_backward_params_det below is the same call with every sum over the batch in a fixed order. */
size_t lsnf_backward_params_workspace_floats(int nz, int width, int depth, int B);
/* 1 if the math mode in force offers the from-the-stash fast path of lsnf_backward_params (every bf16x3-family mode) */
int lsnf_params_fast_path(void);
int lsnf_backward_params(const float* plan, const float* const* params_host, float* const* grads_host,
                         int nz, int width, int depth, int coupling, int B,
                         const float* z_in, const float* z_out, const float* z_saved, const float* act_saved,
                         const float* g_z1, const float* g_logdet, int ll_mode, float ll_scale,
                         float* g_z_in, float* workspace, void* stream);

/* ---- bit-reproducible parameter gradients: lsnf_backward_params with a fixed-order batch contraction ----
 * Same arguments, same selection of the backward and contraction kernels, same fast path / recomputing path and the same
 * alignment rules as lsnf_backward_params, no atomics in any result: every workgroup of the batch contraction stores its
 * partial matrices and column sums into its own slot of a partials area, one further launch (lsnf_fold_reduce_kernel) adds
 * the slots in chunk order in float64 and rounds once, and G is summed over the batch in float64 in a fixed tree.  The
 * chunking follows from (B, depth, contraction kind) alone -- not from the device's CU count, the stream or the environment
 * (LSNF_TN_CHUNK is ignored): at most 128 chunks for the fp32-MFMA contractions (128 rows per chunk below 16 384 rows, 512
 * from there, more once that would exceed 128 chunks), 256 / depth chunks for the bf16 contraction (from 12 288 rows).
 * Guarantee: the same build, inputs, math mode and small-batch threshold give the same bits in every gradient tensor and in
 * g_z_in -- on any stream, inside or outside a captured graph, on any gfx950 device.  "Inputs" includes what selects the
 * contraction kind, since the kind sets the chunking and the arithmetic: whether act_saved is given, the alignment of z_in /
 * z_out / z_saved / g_z1 / g_z_in (16-byte aligned tensors take the bf16 contraction from 12 288 rows and the widest row loads
 * below; others the narrower fp32 forms), and the process-wide experiment knobs LSNF_TN_X3 / LSNF_TN_PLAIN, which this entry
 * point honours as lsnf_backward_params does (read once per process: leave them unset, or set them alike in every run).  The bits are NOT claimed equal to
 * lsnf_backward_params' (another summation order; both are within the same distance of the float64 gradients), nor equal
 * across batch shardings or math modes.
 *   workspace : lsnf_backward_params_det_workspace_floats() floats, 16-byte aligned: lsnf_backward_params_workspace_floats()
 *               rounded up to 16 bytes, plus the partials area behind it -- chunks(B, depth) * depth * F floats, F = the
 *               folded gradients of one block (nz*nz + nz + (nz/2 + width + nz) * width + 2*width + nz, rounded up to 4).
 *               nz 128 / width 64 / depth 5: 663 040 bytes per chunk -- 1 chunk at B = 100, 64 at 8 192, 128 (84.9 MB, on
 *               top of the 671 MB of the dump) at 65 536.  The part before the partials is lsnf_backward_params' own layout:
 *               lsnf_forward / lsnf_reverse_keep take the same pointer as `params_workspace`, and the buffer is also
 *               valid for lsnf_backward_params.
 * Stream-ordered (memset of the 16-byte header, backward, contraction, reduce, unfold: a straight line of launches),
 * allocates nothing, capturable.  Errors as lsnf_backward_params.  Added without an ABI bump (new symbols; nothing existing
 * changed). */
size_t lsnf_backward_params_det_workspace_floats(int nz, int width, int depth, int B);
int lsnf_backward_params_det(const float* plan, const float* const* params_host, float* const* grads_host,
                             int nz, int width, int depth, int coupling, int B,
                             const float* z_in, const float* z_out, const float* z_saved, const float* act_saved,
                             const float* g_z1, const float* g_logdet, int ll_mode, float ll_scale,
                             float* g_z_in, float* workspace, void* stream);

/* ---- optimizer step of the flow: replaces `clip_grad_norm_` + `optF.step()` (train.py:413-415, optimizer train.py:295) ----
 * Global-norm clip and torch.optim.Adam (non-amsgrad, maximize=False, L2 weight decay; definition: PyTorch's
 * _single_tensor_adam) over the depth*12 live tensors, in at most two stream-ordered launches (csrc/lsnf_optim.hip):
 *     norm = sqrt(sum g^2)  (float64, fixed order)        coef = min(1, max_norm / (norm + 1e-6))   (clip_grad_norm_'s formula)
 *     g   = coef * grad                       (only when max_norm > 0; a coef of exactly 1 leaves the unclipped call's bits)
 *     g   = g + weight_decay * p              (only when weight_decay != 0)
 *     m   = m + (1 - beta1) * (g - m)
 *     v   = beta2 * v + (1 - beta2) * g * g
 *     bc1 = 1 - beta1^step;  bc2 = 1 - beta2^step          (float64, step = the device counter AFTER its increment)
 *     p   = p - (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
 * Scalars that depend on `step` or on the norm are derived in float64 once per workgroup.  The element math runs in float64
 * on the stored fp32 values (p is updated from the unrounded m and v) and every stored p, m and v is rounded ONCE: the
 * correctly rounded value of the formulas above, at most half an ulp per step from the float64 definition.  (In fp32
 * arithmetic the two to four roundings per value and the fp32 images of 1 - beta put v up to 1.4 ulp off after one step.)
 *  No atomics and no cross-workgroup barrier: the
 * result is bit-for-bit reproducible and does not depend on the vector width the pointers allow.
 *   params_host  HOST array of depth*12 DEVICE pointers (order above), updated in place; none may be NULL
 *   grads_host   HOST array of depth*12 DEVICE pointers, read only; a NULL entry skips that tensor entirely (its parameter,
 *                m and v keep their bits and it contributes 0 to the norm: torch's `grad is None`)
 *   state        device, 16-byte aligned, lsnf_adam_state_bytes() bytes, owned by the caller; all-zero bytes are a fresh
 *                optimizer.  Layout:
 *                  [LSNF_ADAM_STEP_OFFSET, +8 * LSNF_ADAM_MAX_GROUPS)      int64 step counters, one per workgroup of the update
 *                                                                           launch (a single launch cannot read AND advance a
 *                                                                           shared counter without a grid-wide barrier, so each
 *                                                                           workgroup advances its own; the grid follows from
 *                                                                           the geometry alone, so they always agree; slots
 *                                                                           beyond the grid are not touched).  The one at
 *                                                                           byte 0 is THE step count.  To set the step, write
 *                                                                           all LSNF_ADAM_MAX_GROUPS of them.
 *                  [LSNF_ADAM_PARTIALS_OFFSET, +8 * LSNF_ADAM_MAX_GROUPS)  float64 partial sums of g^2 (internal)
 *                  LSNF_ADAM_NORM_OFFSET                                   float: the last pre-clip norm that was computed
 *                  LSNF_ADAM_HEADER_BYTES ...                              m, flat, in ABI tensor order (block by block, no
 *                                                                           padding between tensors): N = depth * sum of the 12
 *                                                                           sizes floats, rounded up to a multiple of 4; then v
 *   lr, beta1, beta2, eps, weight_decay, max_norm
 *                doubles, as torch.optim.Adam holds them (0.999 is not a float: 1 - beta2 would be off by 1.3e-5 of itself)
 *   lr_dev       NULL, or one device float that replaces `lr` (learning-rate schedules under a captured graph; the idea of
 *                LsnfRng.offset_dev)
 *   max_norm     <= 0: no clipping
 *   grad_norm_out NULL, or one device float that receives the pre-clip global norm (may be the state's own norm slot)
 * With neither clipping nor a norm output the norm launch is skipped: one launch.  Asynchronous, allocates nothing, capturable.
 * LSNF_E_ARG: NULL tables / state / parameter pointer, a pointer that is not 4-byte aligned, misaligned state, lr / eps /
 * weight_decay negative or not finite, a beta outside [0, 1), max_norm NaN.  Non-finite gradients are NOT special-cased: as in
 * torch a NaN norm makes coef NaN and poisons the step -- check grad_norm_out, or use lsnf_adam_step_ex's SKIP_NONFINITE.  Plans prepared before the call are stale
 * afterwards, as after lsnf_actnorm_init.  Added without an ABI bump (new symbols; nothing existing changed). */
#define LSNF_ADAM_MAX_GROUPS 256
#define LSNF_ADAM_STEP_OFFSET 0
#define LSNF_ADAM_PARTIALS_OFFSET 2048
#define LSNF_ADAM_NORM_OFFSET 4096
#define LSNF_ADAM_HEADER_BYTES 4160
size_t lsnf_adam_state_bytes(int nz, int width, int depth, int coupling);      /* 0 on bad geometry */
int lsnf_adam_step(float* const* params_host, const float* const* grads_host,
                   int nz, int width, int depth, int coupling, void* state,
                   double lr, const float* lr_dev, double beta1, double beta2, double eps, double weight_decay,
                   double max_norm, float* grad_norm_out, void* stream);

/* ---- variants of the optimizer step: amsgrad, maximize, AdamW's decoupled decay, non-finite skip, weight EMA ---------------
 * lsnf_adam_step_ex is lsnf_adam_step with an options struct; with flags 0 it IS lsnf_adam_step (same kernel, same bits, same
 * state bytes).  Per element, in this order (torch.optim.Adam / AdamW's _single_tensor_adam for the first four flags):
 *     g   = grad;                 MAXIMIZE: g = -g
 *     g   = coef * g                                        (clip, as above; the norm does not see the sign)
 *     pk  = p
 *     weight_decay != 0:          DECOUPLED: pk = p * (1 - lr * weight_decay)      (the scalar in float64, once per workgroup;
 *                                                                                   lr = *lr_dev when given)
 *                                 else:      g  = g + weight_decay * p             (as above)
 *     m, v                                                  (as above)
 *     AMSGRAD: vmax = max(vmax, v)  (the unrounded v);  den = sqrt(vmax) / sqrt(bc2) + eps        else den from v as above
 *     p   = pk - (lr / bc1) * m / den
 *     EMA:     e_prev = (step == 1) ? p before this update : e;      e = e_prev + (1 - ema_decay) * ((float)p - e_prev)
 * `step` is the counter after its increment: an all-zero state stays "a fresh optimizer", and the average starts from the
 * parameters as the first step finds them.  The average takes the STORED (rounded) new parameter, so a float64 average of the
 * stored parameters reproduces it to half an ulp per step.  Float64 math on the stored fp32 values and one rounding per stored
 * value, as above, for vmax and e too.  With EMA a tensor whose gradient is NULL still has its average updated (its p is
 * loaded; its p / m / v / vmax keep their bits): a tensor that gets its first gradient later does not start from a zero
 * average.
 * SKIP_NONFINITE forces the norm launch.  Every workgroup folds the same partials in the same fixed order and so reaches the
 * same verdict; if the norm is not finite, no p, m, v, vmax or e is written, no step counter advances, the int64 at
 * LSNF_ADAM_SKIPPED_OFFSET grows by 1 (thread 0 of workgroup 0, a plain store) and the norm slot and grad_norm_out still
 * receive the non-finite norm.  No atomics, no grid barrier; bit-for-bit reproducible and capturable like lsnf_adam_step.
 *   state     lsnf_adam_state_bytes_ex(..., flags) bytes: header, m, v, then vmax (only with AMSGRAD), then e (only with EMA),
 *             each the N floats m has.  With neither flag: lsnf_adam_state_bytes().  AMSGRAD and EMA fix the state's size, so
 *             the caller passes them at EVERY call on that state; MAXIMIZE, DECOUPLED and SKIP_NONFINITE may change from call
 *             to call.  The skipped count lives in the spare header bytes, present in every state.
 *   options   struct_bytes = sizeof(LsnfAdamOptions); the fields are lsnf_adam_step's arguments plus flags and ema_decay
 *             (read only with EMA).
 * LSNF_E_ARG, before any HIP call: NULL options, a struct_bytes other than sizeof(LsnfAdamOptions), an unknown flag bit,
 * ema_decay outside [0, 1) or NaN with EMA, and everything lsnf_adam_step refuses.  Added without an ABI bump (new symbols;
 * nothing existing changed). */
#define LSNF_ADAM_AMSGRAD 1u
#define LSNF_ADAM_DECOUPLED 2u
#define LSNF_ADAM_MAXIMIZE 4u
#define LSNF_ADAM_EMA 8u
#define LSNF_ADAM_SKIP_NONFINITE 16u
#define LSNF_ADAM_SKIPPED_OFFSET 4104
typedef struct LsnfAdamOptions {
    unsigned struct_bytes, flags;
    double lr;
    const float* lr_dev;
    double beta1, beta2, eps, weight_decay, max_norm, ema_decay;
    float* grad_norm_out;
} LsnfAdamOptions;
size_t lsnf_adam_state_bytes_ex(int nz, int width, int depth, int coupling, unsigned flags);   /* 0 on bad geometry or flags */
int lsnf_adam_step_ex(float* const* params_host, const float* const* grads_host,
                      int nz, int width, int depth, int coupling, void* state,
                      const LsnfAdamOptions* options, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LSNF_FLOW_H */

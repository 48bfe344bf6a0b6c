/* lsnf_flow_mcmc.h -- Markov-chain extensions of the C ABI of liblsnf_flow.so (include/lsnf_flow.h: conventions, error codes,
 * LsnfRng).  The symbols here are exported by the same library; lsnf_abi_version() does not count them (the core ABI is unchanged).
 *
 * ---- Metropolis-adjusted Langevin step (MALA): accept / reject fused into the step kernel ----------------------------------
 * Target: p(z) ~ exp(-U(z)), U(z) = energy_g(z) - ll(z), ll = the flow prior's log-density (lsnf_forward's ll_out) and energy_g the
 * caller's per-row energy (the generator's |x - G(z)|^2 / (2 sigma^2); NULL = 0: the prior alone).  Proposal from a state z with
 * gradient g = grad U(z):  z' = z - 0.5 s^2 g + s xi, accepted with probability min(1, exp(log_alpha)),
 *     log_alpha = U(z) - U(z') - (|z - z' + 0.5 s^2 g'|^2 - |z' - z + 0.5 s^2 g|^2) / (2 s^2).
 * grad U(z') is only known after a forward and a backward AT z', so one call DECIDES the proposal it is given and PROPOSES the next:
 *   lsnf_forward at z_prop (ll_out, z_saved, act_saved), the caller's grad_g / energy_g at z_prop, then ONE launch here:
 *     g_prop = grad_g + d(-ll)/dz(z_prop)            (lsnf_langevin_step's gradient, from the stash)
 *     U_prop = energy_g - ll_prop,  d = z_prop - z_acc,  A = sum_c (0.5 s^2 g_prop - d)^2,  Bq = sum_c (d + 0.5 s^2 grad_acc)^2
 *     log_alpha = u_acc - U_prop - (A - Bq) / (2 s^2)                          (all fp32)
 *     accept iff ln(u) < log_alpha        (a NaN log_alpha rejects, +inf accepts)
 *     accepted rows: z_acc <- z_prop, grad_acc <- g_prop, u_acc <- U_prop;  rejected rows keep their state bits
 *     z_next = z_state - 0.5 s^2 g_state + s xi   (only if z_next is given; the arithmetic of lsnf_langevin_step's update)
 * K proposals are K + 1 calls: call 0 with LSNF_MALA_INIT at the chain's start (every row accepted, the state arrays are written
 * without being read, log_alpha_out = +0), calls 1 .. K-1 decide and propose, call K decides only (z_next NULL).
 *
 *   z_prop (B,nz)  the proposal; z_out / z_saved / act_saved / ll_prop: lsnf_forward's outputs AT z_prop (act_saved is required:
 *                  the stash of any math mode / kernel family; z_saved for depth > 1)
 *   grad_g (B,nz), energy_g (B): the caller's gradient and energy at z_prop, either may be NULL (= 0)
 *   z_acc (B,nz), grad_acc (B,nz), u_acc (B): the chain state, read and updated in place
 *   u:  `uniform` (B) draws in (0,1), or -- with rng -- ((x0 >> 8) + 0.5) * 2^-24 in fp32 (lsnf_box_muller's arithmetic), x0 = the
 *       first word of Philox4x32-10 at counter (2 << 16, row_lo, offset_lo, offset_hi ^ row_hi), key (seed_lo, seed_hi),
 *       row = rng->row0 + sample: the noise draws use 0 and 1 in that field, so this is a stream of its own, a pure function of
 *       (seed, offset, global row)
 *   xi: a row of `noise` (B,nz), or lsnf_langevin_step's LsnfRng draw at the same (seed, offset, row, column)
 *   rng and a tensor (noise or uniform) exclude each other; without rng, `uniform` is required unless LSNF_MALA_INIT and `noise`
 *   is required iff z_next is given
 *   step_size: finite and non-zero (it divides);  flags: LSNF_MALA_INIT or 0
 *   z_next (B,nz) or NULL; may be z_prop (a workgroup reads its rows before it stores them).  No other output (z_acc, grad_acc,
 *   u_acc, z_next, accept_out, log_alpha_out) may alias anything the call reads, or another output
 *   accept_out (B) or NULL: 1.0 / 0.0;  log_alpha_out (B) or NULL
 * One kernel (lsnf_small3_mala_kernel) under every lsnf_set_math_mode and for every B (more rounds of workgroups above 16 384 rows),
 * independent of lsnf_set_small_batch_max.  B = 0 succeeds without a launch.  Every refusal is LSNF_E_ARG / LSNF_E_GEOMETRY, made
 * before any HIP call.
 *
 * ---- The same step in the flow's base space: lsnf_reverse_mala_step ------------------------------------------------------------
 * The chain runs on eps with x = f^-1(eps) (lsnf_reverse); the flow's log-determinant cancels in the target:
 *     pi(eps) ~ exp(-U(eps)),  U(eps) = |eps|^2 / 2 + energy_g,  grad U(eps) = eps + g,  g = J_{f^-1}(eps)^T grad_g
 * energy_g / grad_g: the caller's per-row energy and its gradient AT x = f^-1(eps) (the generator's |x_obs - G(x)|^2 / (2 sigma^2);
 * NULL = 0: the chain samples N(0, I)); g has the bits of lsnf_reverse_backward_z(g_x = grad_g, g_objective = NULL).  The proposal
 * from a state (e, t = grad U(e)) is lsnf_reverse_langevin_step's arithmetic, operation for operation:
 *     coef = 0.5f * s * s (two roundings);  u = fma(-coef, t, e);  next = fma(s, xi, u)
 * One call DECIDES the proposal it is given and PROPOSES the next; the caller's generator runs between the reverse at eps_prop and
 * this ONE launch.  With d = eps_prop - eps_acc:
 *     t_prop = eps_prop + g_prop                                  (one fp32 add: lsnf_reverse_langevin_step's t)
 *     U_prop = energy_g + 0.5 * sum_c eps_prop^2
 *     A = sum_c (coef t_prop - d)^2,  Bq = sum_c (d + coef grad_acc)^2
 *     log_alpha = (u_acc - U_prop) - (A - Bq) / (2 s^2)           (all fp32, no fp contraction)
 *     accept iff ln(u) < log_alpha        (a NaN log_alpha rejects, +inf accepts)
 *     accepted rows: eps_acc <- eps_prop, grad_acc <- t_prop, u_acc <- U_prop;  rejected rows keep their state bits
 *     eps_next = fma(s, xi, fma(-coef, grad_state, eps_state))    (only if eps_next is given)
 * K proposals are K + 1 calls: call 0 with LSNF_MALA_INIT at the chain's start (every row accepted, the state arrays are written
 * without being read, log_alpha_out = +0, eps_next = lsnf_reverse_langevin_step's eps_new bit for bit), calls 1 .. K-1 decide and
 * propose, call K decides only (eps_next NULL).
 *
 *   eps_prop (B,nz) the proposal = the reverse's input (the z_out of lsnf_reverse_langevin_step); z_saved / act_saved: the block
 *                  outputs and the stash AT x = f^-1(eps_prop), from lsnf_reverse_keep, lsnf_forward at x or lsnf_restash
 *                  (act_saved is required; z_saved for depth > 1)
 *   grad_g (B,nz), energy_g (B): either may be NULL (= 0)
 *   eps_acc (B,nz), grad_acc (B,nz), u_acc (B): the chain state (eps, eps + g, U), read and updated in place
 *   u:  `uniform` (B) draws in (0,1), or -- with rng -- lsnf_mala_step's draw (Philox word 0 at field value 2 of the noise's counter)
 *   xi: a row of `noise` (B,nz), or lsnf_reverse_langevin_step's LsnfRng draw at the same (seed, offset, row, column): the same bits
 *   rng and a tensor (noise or uniform) exclude each other; rng->offset_dev 8-byte aligned, rng->row0 >= 0; without rng, `uniform`
 *   is required unless LSNF_MALA_INIT and `noise` is required iff eps_next is given
 *   step_size: finite and non-zero (it divides);  flags: LSNF_MALA_INIT or 0
 *   eps_next (B,nz) or NULL; may be eps_prop (a workgroup reads its rows before it stores them).  No other output (eps_acc, grad_acc,
 *   u_acc, eps_next, accept_out, log_alpha_out) may alias anything the call reads, or another output
 *   accept_out (B) or NULL: 1.0 / 0.0;  log_alpha_out (B) or NULL
 *   alignment as lsnf_reverse_backward_z: plan and act_saved 16 bytes, every other tensor 4
 * One kernel (lsnf_small3_rmala_kernel) under every lsnf_set_math_mode and for every B (more rounds of workgroups above 16 384 rows),
 * independent of lsnf_set_small_batch_max; a row's decision and bits do not depend on B, the workgroup shape or rng->row0 sharding.
 * B = 0 succeeds without a launch.  Every refusal is LSNF_E_ARG / LSNF_E_GEOMETRY, made before any HIP call. */
#ifndef LSNF_FLOW_MCMC_H
#define LSNF_FLOW_MCMC_H

#include "lsnf_flow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSNF_MALA_INIT 1u
int lsnf_mala_step(const float* plan, int nz, int width, int depth, int coupling, int B,
                   const float* z_prop, const float* z_out, const float* z_saved, const float* act_saved,
                   const float* ll_prop, const float* grad_g, const float* energy_g,
                   float* z_acc, float* grad_acc, float* u_acc,
                   const float* noise, const float* uniform, const LsnfRng* rng, float step_size, unsigned flags,
                   float* z_next, float* accept_out, float* log_alpha_out, void* stream);
int lsnf_reverse_mala_step(const float* plan, int nz, int width, int depth, int coupling, int B,
                           const float* eps_prop, const float* z_saved, const float* act_saved,
                           const float* grad_g, const float* energy_g,
                           float* eps_acc, float* grad_acc, float* u_acc,
                           const float* noise, const float* uniform, const LsnfRng* rng, float step_size, unsigned flags,
                           float* eps_next, float* accept_out, float* log_alpha_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LSNF_FLOW_MCMC_H */

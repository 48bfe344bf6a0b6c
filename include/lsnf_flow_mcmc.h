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
 * B = 0 succeeds without a launch.  Every refusal is LSNF_E_ARG / LSNF_E_GEOMETRY, made before any HIP call.
 *
 * ---- Hamiltonian Monte Carlo in z: L leapfrog steps per accept / reject (lsnf_hmc_step) ------------------------------------------
 * The target of lsnf_mala_step, p(z) ~ exp(-U(z)), U = energy_g - ll, with a momentum p ~ N(0, I), step s and L >= 1 leapfrog steps
 * per trajectory.  As there, grad U at a point is known only after a forward and a backward AT that point, so one call finishes the
 * work at the point z_prop it is given (lsnf_forward's outputs at z_prop, the caller's grad_g / energy_g at z_prop) and produces the
 * next point.  From a state (z_s, g_s = grad U(z_s), u_s = U(z_s)), every line in fp32 with the operations and the order written,
 * no fused multiply-add (hs = 0.5f * s: exact):
 *   begin  (inside the call that owns the state: LSNF_HMC_INIT, or an end call with z_next)
 *           kin0 = 0.5f * sum_c xi^2;   ph = xi - hs * g_s;   z_next = z_s + s * ph;   mom <- ph
 *   inner  (LSNF_HMC_INNER, the calls at z_1 .. z_{L-1})
 *           g = grad_g + d(-ll)/dz(z_prop);   ph = mom - s * g;   z_next = z_prop + s * ph;   mom <- ph
 *   end    (flags 0, the call at z_L)
 *           g_prop = grad_g + d(-ll)/dz(z_prop);   U_prop = energy_g - ll_prop;   pL = mom - hs * g_prop;   kinL = 0.5f * sum_c pL^2
 *           log_alpha = (u_acc - U_prop) + (kin0 - kinL)
 *           accept iff ln(u) < log_alpha        (a NaN log_alpha rejects, +inf accepts)
 *           accepted rows: z_acc <- z_prop, grad_acc <- g_prop, u_acc <- U_prop;  rejected rows keep their state bits
 *           z_next given: begin the next trajectory from the (updated) state;  z_next NULL: mom <- pL (the full-step momentum at
 *           the proposal is left readable), nothing else is proposed and kin0 is left as it is
 * The sums over a row's columns: a lane adds the squares of its 8 columns in column order, lsnf_mala_step's reduction adds the
 * lanes of a wave and the four waves' partials are added in wave order.
 * K trajectories of L steps are K L + 1 calls: one LSNF_HMC_INIT call at the chain's start (every row accepted, the state written
 * without being read, log_alpha_out = +0, the first trajectory begun; without z_next it writes the state alone and leaves mom and
 * kin0 as they are), L - 1 LSNF_HMC_INNER calls per trajectory, K end calls, the last one with z_next NULL.  With L = 1 there are no
 * inner calls and the chain is lsnf_mala_step's in exact arithmetic (kinL = A / (2 s^2), kin0 = Bq / (2 s^2) in its notation).
 *
 *   the arguments shared with lsnf_mala_step follow its rules (z_prop .. energy_g, z_acc / grad_acc / u_acc, step_size, accept_out,
 *   log_alpha_out, the 16-byte alignment of plan and act_saved and the 4-byte alignment of every tensor), except as stated below
 *   mom (B,nz): the momentum, read AND written by the same call (written only by INIT when z_next is NULL);  kin0 (B): the kinetic
 *       energy the running trajectory began with, written by a call that begins one, read by an end call.  Both are required
 *   xi: a row of `noise` (B,nz), or lsnf_langevin_step's LsnfRng draw at the call's (seed, offset, row, column)
 *   u:  lsnf_mala_step's: `uniform` (B), or with rng word 0 of Philox at field value 2 of the noise's counter
 *   flags: 0, LSNF_HMC_INIT or LSNF_HMC_INNER; both together and unknown bits are refused
 *   an LSNF_HMC_INNER call draws and decides nothing: it requires z_next, refuses noise, uniform and rng, wants accept_out and
 *       log_alpha_out NULL, neither reads nor writes z_acc, grad_acc, u_acc or kin0 (they are still required), and the library never
 *       reads ll_prop or energy_g (ll_prop may be NULL there)
 *   INIT and end calls: rng and a tensor (noise or uniform) exclude each other; without rng, `noise` is required iff z_next is
 *       given and `uniform` is required unless LSNF_HMC_INIT
 *   z_next (B,nz) or NULL; may be z_prop (a lane stores the columns it loaded, after the barrier).  No other output (z_acc,
 *   grad_acc, u_acc, mom, kin0, z_next, accept_out, log_alpha_out) may alias anything the call reads, or another output
 * One kernel (lsnf_small3_hmc_kernel) under every lsnf_set_math_mode, for every B and every phase, independent of
 * lsnf_set_small_batch_max; a row's bits do not depend on B, the workgroup shape or rng->row0 sharding.  B = 0 succeeds without a
 * launch.  Every refusal is LSNF_E_ARG / LSNF_E_GEOMETRY, made before any HIP call.
 *
 * ---- Hamiltonian Monte Carlo in the flow's base space (lsnf_reverse_hmc_step) ------------------------------------------------------
 * The target and the gradient of lsnf_reverse_mala_step -- pi(eps) ~ exp(-U(eps)), U(eps) = |eps|^2 / 2 + energy_g, grad U = eps + g,
 * g = J_{f^-1}(eps)^T grad_g with the bits of lsnf_reverse_backward_z(g_x = grad_g, g_objective = NULL) -- with a momentum p ~ N(0, I):
 * the flow has whitened the prior, so the identity mass matrix is the right one for the prior alone (an informative likelihood makes
 * the posterior in eps anisotropic again: lsnf_reverse_hmc_step_metric below).  eps_prop / z_saved / act_saved are the reverse's
 * input, the block outputs and the stash AT x = f^-1(eps_prop) (lsnf_reverse_keep, lsnf_forward at x or lsnf_restash); the caller's
 * generator runs between the reverse and this ONE launch, which finishes the work at the point eps_prop of a trajectory and produces
 * the next point.  From a state (e_s, t_s = grad U(e_s), u_s = U(e_s)), every line in fp32 with the operations and the order written,
 * no fused multiply-add (hs = 0.5f * s: exact); in every phase that forms a gradient t_prop = eps_prop + g is ONE fp32 add
 * (lsnf_reverse_mala_step's t_prop: grad_acc has that function's bits):
 *   begin  (inside the call that owns the state: LSNF_HMC_INIT, or an end call with eps_next)
 *           kin0 = 0.5f * sum_c xi^2;   ph = xi - hs * t_s;   eps_next = e_s + s * ph;   mom <- ph
 *   inner  (LSNF_HMC_INNER, the calls at eps_1 .. eps_{L-1})
 *           ph = mom - s * t_prop;   eps_next = eps_prop + s * ph;   mom <- ph
 *   end    (flags 0, the call at eps_L)
 *           U_prop = energy_g + 0.5f * sum_c eps_prop^2;   pL = mom - hs * t_prop;   kinL = 0.5f * sum_c pL^2
 *           log_alpha = (u_acc - U_prop) + (kin0 - kinL)
 *           accept iff ln(u) < log_alpha        (a NaN log_alpha rejects, +inf accepts)
 *           accepted rows: eps_acc <- eps_prop, grad_acc <- t_prop, u_acc <- U_prop;  rejected rows keep their state bits
 *           eps_next given: begin the next trajectory from the (updated) state;  eps_next NULL: mom <- pL (the full-step momentum at
 *           the proposal is left readable), nothing else is proposed and kin0 is left as it is
 * The sums over a row's columns: sum eps_prop^2 in lsnf_reverse_mala_step's order (an LSNF_HMC_INIT call writes that function's
 * LSNF_MALA_INIT state -- eps_acc, grad_acc, u_acc -- bit for bit); sum pL^2 and sum xi^2 in lsnf_hmc_step's: a lane adds the squares
 * of its 8 columns in column order, the wave reduction adds the lanes of a wave and the four waves' partials are added in wave order.
 * A draw for a padding column is not counted.
 * K trajectories of L steps are K L + 1 calls: one LSNF_HMC_INIT call at the chain's start (every row accepted, the state written
 * without being read, log_alpha_out = +0, the first trajectory begun; without eps_next it writes the state alone and leaves mom and
 * kin0 as they are), L - 1 LSNF_HMC_INNER calls per trajectory, K end calls, the last one with eps_next NULL.  With L = 1 there are no
 * inner calls and the chain is lsnf_reverse_mala_step's in exact arithmetic (kinL = A / (2 s^2), kin0 = Bq / (2 s^2) in its notation).
 *
 *   the arguments shared with lsnf_reverse_mala_step follow its rules (eps_prop .. energy_g, eps_acc / grad_acc / u_acc, step_size,
 *   accept_out, log_alpha_out, the 16-byte alignment of plan and act_saved and the 4-byte alignment of every tensor; act_saved is
 *   required, z_saved for depth > 1), except as stated below -- the rules of lsnf_hmc_step, word for word where they apply
 *   mom (B,nz): the momentum, read AND written by the same call (written only by INIT when eps_next is NULL);  kin0 (B): the kinetic
 *       energy the running trajectory began with, written by a call that begins one, read by an end call.  Both are required
 *   xi: a row of `noise` (B,nz), or lsnf_reverse_mala_step's LsnfRng draw (lsnf_sample's eps at temperature 1) at the call's (seed,
 *       offset, global row, column)
 *   u:  lsnf_mala_step's: `uniform` (B), or with rng word 0 of Philox at field value 2 of the noise's counter
 *   flags: 0, LSNF_HMC_INIT or LSNF_HMC_INNER; both together and unknown bits are refused
 *   an LSNF_HMC_INNER call draws and decides nothing: it requires eps_next, refuses noise, uniform and rng, wants accept_out and
 *       log_alpha_out NULL, neither reads nor writes eps_acc, grad_acc, u_acc or kin0 (they are still required), and the library never
 *       reads energy_g
 *   INIT and end calls: rng and a tensor (noise or uniform) exclude each other; without rng, `noise` is required iff eps_next is
 *       given and `uniform` is required unless LSNF_HMC_INIT
 *   step_size: finite and non-zero
 *   eps_next (B,nz) or NULL; may be eps_prop (a lane stores the columns it loaded, after the barrier).  No other output (eps_acc,
 *   grad_acc, u_acc, mom, kin0, eps_next, accept_out, log_alpha_out) may alias anything the call reads, or another output
 * One kernel (lsnf_small3_rhmc_kernel) under every lsnf_set_math_mode, for every B (more rounds of workgroups above 16 384 rows) and
 * every phase, independent of lsnf_set_small_batch_max; a row's bits do not depend on B, the workgroup shape or rng->row0 sharding.
 * B = 0 succeeds without a launch.  Every refusal is LSNF_E_ARG / LSNF_E_GEOMETRY, made before any HIP call.
 *
 * ---- A step per row, adapted on the device (lsnf_hmc_step_rows, lsnf_reverse_hmc_step_rows) ------------------------------------------
 * Every row of a batch targets a posterior of its own, so every row may run at a step of its own.  The two entry points are
 * lsnf_hmc_step and lsnf_reverse_hmc_step with `float step_size` replaced by `float* step_rows, float* adapt, const LsnfDualAvg* da`;
 * every other argument, rule, draw and refusal is the scalar call's, word for word (there is no step_size rule: the steps are
 * device memory and are not looked at on the host; a row whose step is zero or not finite gets what the arithmetic gives it).
 *   step_rows (B): row b's step for the RUNNING trajectory.  Every phase reads it; only an LSNF_HMC_ADAPT end call writes it.
 *   adapt (B,4), 16-byte aligned: {log_step_bar, hbar, count, mu} per row, the state of the dual averaging (Hoffman & Gelman 2014,
 *       algorithm 5).  mu is the caller's, log(10 * the first step); a fresh row has log_step_bar = hbar = count = 0.  With
 *       LSNF_HMC_ADAPT adapt and da are required; without it both must be NULL.
 *   da: the update's constants (host memory, read during the call only): all finite, target_accept in (0,1), gamma > 0, t0 + 1 > 0,
 *       step_min > 0, step_max >= step_min.  Stan's: 0.8, 0.05, 10, 0.75.
 *   flags: 0, LSNF_HMC_INIT or LSNF_HMC_INNER as in the scalar call; LSNF_HMC_ADAPT with an end call only (refused with INIT or
 *       INNER), LSNF_HMC_ADAPT_LAST with LSNF_HMC_ADAPT only; unknown bits are refused
 *   step_rows and adapt are outputs in the sense of the aliasing rule: they may alias nothing else the call touches
 * (1) Without LSNF_HMC_ADAPT row b's outputs are the scalar call's at step_size = step_rows[b], bit for bit, in every phase: the
 *     operations and the order written above with s read per row.
 * (2) An end call with LSNF_HMC_ADAPT finishes and decides the trajectory with the old step_rows[b], then, per row, in fp32 with the
 *     operations and the order written and no fused multiply-add (la: the row's log_alpha; LAST: LSNF_HMC_ADAPT_LAST):
 *         a    = (la == la) ? fminf(1, expf(la)) : 0          (a NaN log_alpha counts as a rejection)
 *         t    = count + 1;  eta = 1 / (t + t0)
 *         hbar = (1 - eta) * hbar + eta * (target_accept - a)
 *         ls   = clamp(mu - (sqrtf(t) / gamma) * hbar, logf(step_min), logf(step_max))      (the two logs taken on the host)
 *         w    = powf(t, -kappa);  lsb = w * ls + (1 - w) * lsb
 *         s'   = expf(LAST ? lsb : ls)
 *     stores adapt = {lsb, hbar, t, mu} and step_rows[b] = s', and, if z_next / eps_next is given, begins the next trajectory with
 *     s' (hs = 0.5f * s').  mom, with z_next / eps_next NULL, is the full-step momentum at the OLD step.  This keeps the chain valid:
 *     a row's step is fixed before its momentum is drawn and is constant within a trajectory.  While steps adapt the chain is not
 *     exactly invariant; it is from the call with LSNF_HMC_ADAPT_LAST on, which leaves the averaged step for the calls that follow.
 * Kernels: lsnf_small3_hmcr_kernel / lsnf_small3_rhmcr_kernel, the scalar kernels' stages with the per-row tail, the same
 * instantiations and workgroup shapes; a row's bits -- its new step and adapt included -- do not depend on B, the workgroup shape
 * or rng->row0 sharding.  With L = 1 the calls are the adaptive MALA step in exact arithmetic, as the scalar calls are MALA's.
 *
 * ---- A diagonal metric per row, estimated in warm-up windows on the device (lsnf_hmc_step_metric, lsnf_reverse_hmc_step_metric) ------
 * Without a metric the stiffest coordinate of a row's posterior sets its step, in z and -- once the likelihood is informative -- in
 * the base space as well (the flow whitens the prior, not the posterior).  Row b has a positive scale per column, sd[b, c]: the
 * square root of the diagonal inverse mass (Stan's inv_e_metric, as a standard deviation).  The chain is HMC with identity mass in
 * the coordinate y = z / sd: the momentum q ~ N(0, I) lives in that coordinate, so kin0, kinL, the reductions and the decision are the
 * per-row call's, untouched, and the only change is one more multiply in two products.  The two entry points are the per-row calls
 * with `float* scale_rows, float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg` inserted between da and
 * flags.  Everything fp32, no fused multiply-add; s is the row's step, hs = 0.5f * s; the parentheses are the rule -- sd * g and
 * sd * qh are each ONE rounded product, formed first:
 *   begin   kin0 = 0.5f * sum_c xi^2;   qh = xi  - hs * (sd * g_s);     z_next = z_s    + s * (sd * qh);   mom <- qh
 *   inner   g = grad_g + d(-ll)/dz;     qh = mom - s  * (sd * g);       z_next = z_prop + s * (sd * qh);   mom <- qh
 *   end     qL = mom - hs * (sd * g_prop);   kinL = 0.5f * sum_c qL^2;   log_alpha, accept, state update: lsnf_hmc_step_rows' lines
 * (lsnf_reverse_hmc_step_metric: the same with t = eps + g in place of g, from lsnf_reverse_hmc_step_rows' lines.)  Hence, exactly:
 * (1) with sd == 1.0f everywhere a row's outputs in every phase are the per-row call's, bit for bit;
 * (2) with sd == 2^k on every column of a row, a row's outputs at step s are the per-row call's at step s * 2^k, bit for bit (every
 *     product is then an exact scaling), wherever no intermediate overflows or becomes subnormal.
 *   scale_rows (B,nz): sd.  Every phase reads it; only a call with LSNF_HMC_METRIC_CLOSE writes it.  Always required.
 *   mean_rows (B,nz), m2_rows (B,nz), count_rows (B): the Welford accumulators of the row's running window (a fresh window: zeros)
 *   reg: the close's constants (host memory, read during the call only): all finite, n0 >= 0, var0 >= 0, scale_min > 0,
 *       scale_max >= scale_min.  Stan's: n0 = 5, var0 = 1e-3.
 *   mean_rows, m2_rows, count_rows and reg are required with LSNF_HMC_METRIC_FOLD and must be NULL without it
 *   flags: the per-row call's; LSNF_HMC_METRIC_FOLD with an end call only (refused with INIT or INNER), LSNF_HMC_METRIC_CLOSE with
 *       LSNF_HMC_METRIC_FOLD only; unknown bits are refused
 *   the four arrays are outputs in the sense of the aliasing rule: they may alias nothing else the call touches
 *   every other argument, rule, draw and refusal is the per-row call's, word for word
 * FOLD: the end call folds the state AFTER its decision, x = z_prop on accepted rows and z_acc on rejected ones (eps_prop / eps_acc),
 * into the row's accumulators, before the next trajectory begins (per column; count per row):
 *         n = count + 1;   d = x - mean;   mean' = mean + d / n;   m2' = m2 + d * (x - mean');   count' = n
 * CLOSE: the same call, after the fold:
 *         n >= 2:  v = (n / (n + n0)) * (m2' / (n - 1)) + var0 * (n0 / (n + n0));   sd' = fminf(fmaxf(sqrtf(v), scale_min), scale_max)
 *         n <  2:  sd' = sd (the bits are kept)
 *     stores sd', stores zeros for mean, m2 and count, begins the next trajectory with sd' if a next point is asked for (mom, with no
 *     next point, is the full-step momentum at the OLD step and the OLD scale) and, with LSNF_HMC_ADAPT and without
 *     LSNF_HMC_ADAPT_LAST, stores the dual-averaging quad as {0, 0, 0, logf(10.0f * s')}, s' the step this call's update wrote:
 *     Stan's restart of the step adaptation at a window's end.  (A variance that is NaN closes at scale_min.)
 * A row's scale is fixed before its momentum is drawn and constant within a trajectory, exactly as its step is.  While scales change
 * the chain is not exactly invariant; from the last close on it is.
 * Kernels: lsnf_small3_hmcm_kernel / lsnf_small3_rhmcm_kernel, the per-row kernels' stages, instantiations and workgroup shapes; sd,
 * mean and m2 are read and written by the lane that owns their columns, so a row's bits -- scale and accumulators included -- do not
 * depend on B, the workgroup shape or rng->row0 sharding.  B = 0 succeeds without a launch.
 *
 * ---- A likelihood temperature per row: tempered steps with fused importance weights (lsnf_hmc_step_tempered, ------------------------
 * ---- lsnf_reverse_hmc_step_tempered) -----------------------------------------------------------------------------------------------------
 * The target at inverse temperature beta is p_flow(z) * p(x | G(z))^beta: the likelihood's part of the potential and of its gradient
 * carries the weight beta, the prior's part the weight 1.  Row b has a temperature of its own in device memory.  With a common schedule
 * 0 = beta_0 <= .. <= beta_T = 1 the calls are annealed importance sampling (Neal 2001) with HMC transitions; rows at distinct fixed
 * temperatures are the replicas of a parallel-tempering sampler.  The two entry points are the metric calls with
 * `float* beta_rows, const float* beta_next, float* like_grad_acc, float* like_u_acc, float* log_w` inserted between reg and flags.
 * Everything fp32 with the operations and the order written, no fused multiply-add; each product in parentheses is ONE rounded
 * product, formed first.  The likelihood's parts of a point are gl and el:
 *   z space:     gl = grad_g,  el = energy_g  (NULL = 0)
 *   base space:  gl = J_{f^-1}(eps)^T grad_g, the kernel's own back-propagated gradient, unscaled, with lsnf_reverse_backward_z's bits;
 *                el = energy_g  (NULL = 0)
 * In every phase that forms a gradient or a potential (beta = beta_rows[b]):
 *   z:    g = (beta * gl) + d(-ll)/dz(z_prop);     U_prop = (beta * el) - ll_prop
 *   eps:  t_prop = eps_prop + (beta * gl);         U_prop = (beta * el) + 0.5f * sum_c eps_prop^2
 * Everything else of begin / inner / end is the metric call's lines: the decision, the state update, the dual averaging, the fold and
 * the close.
 *   beta_rows (B): row b's beta for the RUNNING trajectory.  Every phase reads it; only a call with LSNF_HMC_ANNEAL writes it.  It is
 *       device memory and is not looked at on the host, as step_rows is.  Always required.
 *   like_grad_acc (B,nz), like_u_acc (B): gl and el of the kept state.  They are written wherever z_acc / eps_acc is written: every
 *       row on LSNF_HMC_INIT, accepted rows on an end call; rejected rows keep their bits.  Always required; LSNF_HMC_INNER calls
 *       neither read nor write them.
 *   flags: the metric call's; LSNF_HMC_ANNEAL with LSNF_HMC_INIT or an end call (refused with LSNF_HMC_INNER); unknown bits are refused
 *   beta_next (B), log_w (B,2; 8-byte aligned): required with LSNF_HMC_ANNEAL, must be NULL without it
 *   all five arrays are outputs in the sense of the aliasing rule: they may alias nothing else the call touches
 *   every other argument, rule, draw and refusal is the metric call's, word for word
 * ANNEAL runs after the decision and after the metric call's adapt / fold / close, and before the next trajectory begins.  With
 * (g_s, u_s, gl_s, el_s) the state after the decision (the proposal's on accepted rows, the kept one on rejected rows):
 *         d = beta_next[b] - beta
 *         inc = -(d * el_s);   y = inc - c;   t = w + y;   c' = (t - w) - y;   w' = t      (log_w[b] = {w, c}: Kahan's sum)
 *         u_acc <- u_s + (d * el_s);     grad_acc <- g_s + (d * gl_s)   per column          (every row, accepted or not)
 *         beta_rows[b] <- beta_next[b]
 *     The trajectory this call begins (if a next point is asked for) starts from the re-tempered grad_acc.  log_w[b][0] - log_w[b][1]
 *     is the row's log importance weight, sum_t -(beta_{t+1} - beta_t) * E(state_t).  LSNF_HMC_INIT does not clear log_w: zeroing it
 *     is the caller's job.  The kept state can be re-tempered exactly because the likelihood's part of it is kept apart.
 * Hence, exactly:
 * (1) with beta_rows == 1.0f everywhere and without LSNF_HMC_ANNEAL, every output a call shares with the metric call has that call's
 *     bits, in every phase (1.0f * x is x);
 * (2) with beta_rows[b] == 2^k, row b's outputs are the metric call's at (2^k grad_g, 2^k energy_g), bit for bit (the products are
 *     exact scalings), wherever nothing overflows or becomes subnormal.
 * Kernels: lsnf_small3_hmct_kernel / lsnf_small3_rhmct_kernel, the metric kernels' stages, instantiations and workgroup shapes; beta,
 * like_u_acc and the log_w pair are row scalars read by every wave in front of the barrier and stored by one lane after it,
 * like_grad_acc is read and written by the lane that owns its columns, so a row's bits do not depend on B, the workgroup shape or
 * rng->row0 sharding.  B = 0 succeeds without a launch.
 *
 * ---- Replica exchange between rows at distinct temperatures: parallel tempering (lsnf_hmc_step_exchange, -----------------------------
 * ---- lsnf_reverse_hmc_step_exchange) -----------------------------------------------------------------------------------------------------
 * The two entry points are the tempered calls with `int ladder, const float* swap_uniform, float* swap_out, float* log_swap_out`
 * inserted between log_alpha_out and stream, and two more flags.  Without LSNF_HMC_SWAP every output has the tempered call's bits in
 * every phase and the four new arguments must be 0 / NULL (ladder is not looked at).
 *   ladder: R in {2, 4, 8, 16}, B % R == 0.  Rows [k R, (k + 1) R) are the rungs of ladder k, rung r = row % R; beta per rung is
 *       whatever beta_rows holds (it need not be ordered).
 *   flags: the tempered call's; LSNF_HMC_SWAP only on an end call (neither LSNF_HMC_INIT nor LSNF_HMC_INNER) and without
 *       LSNF_HMC_ADAPT, LSNF_HMC_METRIC_FOLD, LSNF_HMC_METRIC_CLOSE and LSNF_HMC_ANNEAL; LSNF_HMC_SWAP_ODD only with LSNF_HMC_SWAP.
 *       Even parity pairs rungs (0,1), (2,3), ..; odd parity pairs (1,2), (3,4), .. and leaves rungs 0 and R - 1 idle (R = 2: nothing
 *       swaps).  A pair never crosses a ladder's border.
 *   swap_uniform (B): the uniform of the pair (a, b), a the lower row, is swap_uniform[a].  It goes with the tensor form of the noise
 *       and is then required; with an rng it must be NULL and the number is word 0 of Philox at the call's (seed, offset), at the
 *       global row of a, at counter field value 3 (the noise draws use 0 and 1, the trajectory's uniform 2), formed as that uniform
 *       is: a pure function of (seed, offset, global row of a), so a ladder swaps alike however the batch is sharded along whole ladders.
 *   swap_out, log_swap_out (B): optional outputs; they may alias nothing else the call touches.
 * The move comes after the trajectory's decision and the state update and before the next trajectory begins.  With
 * (z_s, g_s, u_s, gl_s, el_s) a row's state after the decision, for the pair (a, b):
 *         d = beta_a - beta_b;   e = el_s_a - el_s_b;   log_r = d * e              (one rounded product; both rows form it in this order)
 *         the pair swaps iff logf(u) < log_r                                       (a NaN log_r rejects)
 *     The states are exchanged, not the temperatures.  A row that swaps (p its partner, d_own = beta_own - beta_p):
 *         z_acc <- z_s_p;   like_grad_acc <- gl_s_p;   like_u_acc <- el_s_p
 *         grad_acc <- g_s_p + (d_own * gl_s_p)   per column;     u_acc <- u_s_p + (d_own * el_s_p)
 *     and the trajectory this call begins (if a next point is asked for) starts from that state with the row's own step, scale and xi.
 *     beta_rows, step_rows, scale_rows and everything of the adaptation stay with the row.
 *         swap_out[b] = 1.0f on both rows of an exchanged pair, else 0.0f;   log_swap_out[b] = log_r on both rows of a pair, 0.0f on
 *     an idle rung.  accept_out and log_alpha_out stay the trajectory's own.
 * Kernels: lsnf_small3_hmcx_kernel / lsnf_small3_rhmcx_kernel, the tempered kernels' stages, instantiations and workgroup shapes.  A
 * ladder lies inside one wave's 16-row tile, the partner's state comes over lane to lane, and every lane writes its own row only: no
 * row reads what another row writes in the same launch.  B = 0 succeeds without a launch.
 *
 * ---- Resampling between the rows of a group on an annealing end call: a sequential Monte Carlo sampler (lsnf_hmc_step_resample, ------
 * ---- lsnf_reverse_hmc_step_resample) -----------------------------------------------------------------------------------------------------
 * The two entry points are the tempered calls with `int group, float ess_frac, const float* resample_uniform, float* ancestor_out,
 * float* ess_out` inserted between log_alpha_out and stream, and one more flag (LSNF_HMC_SWAP is not among theirs).  Without
 * LSNF_HMC_RESAMPLE every output has the tempered call's bits in every phase and the three pointers must be NULL (group and ess_frac
 * are not looked at).
 *   group: P in {2, 4, 8, 16}, B % P == 0.  Rows [k P, (k + 1) P) are the particles of group k, rung r = row % P.
 *   ess_frac: the group resamples iff its effective sample size is below ess_frac * P.  <= 0: never; > 1: always.
 *   flags: the tempered call's; LSNF_HMC_RESAMPLE only on an end call (neither LSNF_HMC_INIT nor LSNF_HMC_INNER) WITH LSNF_HMC_ANNEAL
 *       and without LSNF_HMC_ADAPT, LSNF_HMC_METRIC_FOLD and LSNF_HMC_METRIC_CLOSE: the chain is frozen.
 *   resample_uniform (B): the group's ONE uniform u, in [0, 1), is resample_uniform[first row of the group].  It goes with the tensor
 *       form of the noise and is then required; with an rng it must be NULL and the number is word 0 of Philox at the call's (seed,
 *       offset), at the global row of the group's first row, at counter field value 4 (the noise draws use 0 and 1, the trajectory's
 *       uniform 2, the swap's 3), formed as those uniforms are: a pure function of (seed, offset, that global row), so a group
 *       resamples alike however the batch is sharded along whole groups.
 *   ancestor_out, ess_out (B): optional outputs; they may alias nothing else the call touches.
 * The move comes after the trajectory's decision, the state update and the ANNEAL lines above, and before the next trajectory begins.
 * With {w_i, c_i} row i's Kahan pair after the increment, beta'_i = beta_next[i], and (z_s, g_s', u_s', gl_s, el_s) row i's state after
 * the decision with g_s' and u_s' re-tempered to beta'_i by the ANNEAL lines; i, j run over the group's rungs 0 .. P - 1.  Every line
 * is one fp32 operation, rounded once:
 *         l_i = w_i - c_i
 *         m = max_i l_i                                          (fmaxf, in rung order: a NaN is passed over)
 *         e_i = expf(l_i - m)
 *         S1 = ((e_0 + e_1) + ..) + e_{P-1};   q_i = e_i * e_i;   S2 = ((q_0 + q_1) + ..) + q_{P-1}       (from 0.0f, in rung order)
 *         ess = (S1 * S1) / S2
 *         the group resamples iff ess < ess_frac * P             (a NaN anywhere makes this false: the group is left alone)
 *     Systematic resampling of a group that resamples, for rung k (P as a float is a power of two, so / P is exact):
 *         tau_k = (((float)k + u) / P) * S1
 *         cum_j = ((e_0 + e_1) + ..) + e_j                       (S1's partial sums)
 *         a_k = min(#{ j : cum_j <= tau_k }, P - 1)              (the clamp matters only where tau_k reaches S1: u = 1.0f, which the
 *                                                                 in-kernel number's last rounding can give, or a rounding of tau_k)
 *         log_w[k] <- { m + logf(S1 / P), 0.0f }                 (every row of the group; S1 / P first)
 *     A row with a_k != k takes its ancestor's state (a = a_k, d_own = beta'_k - beta'_a) over what the update stored:
 *         z_acc <- z_s_a;   like_grad_acc <- gl_s_a;   like_u_acc <- el_s_a
 *         grad_acc <- g_s'_a + (d_own * gl_s_a)   per column;     u_acc <- u_s'_a + (d_own * el_s_a)
 *     and the trajectory this call begins (if a next point is asked for) starts from that state with the row's own step, scale and xi.
 *     beta_rows, step_rows, scale_rows and everything of the adaptation stay with the row.  Rows with a_k == k keep the tempered
 *     call's bits but for log_w; a group that does not resample keeps them everywhere.
 *         ancestor_out[b] = (float)a_k in a group that resamples, else (float)k;   ess_out[b] = ess on every row of the group.
 *     accept_out and log_alpha_out stay the trajectory's own.  The mean of exp(log_w) over a group is unchanged by the move up to
 *     rounding, so logsumexp over the rows minus log(rows) remains the unbiased estimate of the normalising constant.
 * Kernels: lsnf_small3_hmcs_kernel / lsnf_small3_rhmcs_kernel, the tempered kernels' stages, instantiations and workgroup shapes.  A
 * group lies inside one wave's 16-row tile, every lane of every wave forms the sums from the same values in the same order, the
 * ancestor's state comes over lane to lane, and every lane writes its own row only: no row reads what another row writes in the same
 * launch.  B = 0 succeeds without a launch.
 *
 * ---- The next temperature chosen in the annealing call: adaptive tempering (lsnf_hmc_step_schedule, -----------------------------------
 * ---- lsnf_reverse_hmc_step_schedule) -----------------------------------------------------------------------------------------------------
 * The two entry points are the resampling calls with `float cess_frac, float min_step` inserted between ess_out and stream, and one
 * more flag.  Without LSNF_HMC_SCHEDULE every output has the resampling call's bits in every phase (cess_frac and min_step are not
 * looked at).  With it beta_next is not the groups' next temperature but its CEILING: the call steps each group of P rows to the
 * temperature at which the conditional effective sample size of the incremental weights (Zhou, Johansen & Aston 2016) is cess_frac * P,
 * found by twelve halvings, and no further than the ceiling.
 *   group: P in {2, 4, 8, 16}, B % P == 0, whenever LSNF_HMC_SCHEDULE or LSNF_HMC_RESAMPLE is set: one argument serves both.
 *   cess_frac: 0 < cess_frac < 1.   min_step: finite and >= 0; with min_step > 0 a group needs at most 1 / min_step calls to arrive.
 *   flags: the resampling call's; LSNF_HMC_SCHEDULE goes WITH LSNF_HMC_ANNEAL, on an LSNF_HMC_INIT call or an end call (never with
 *       LSNF_HMC_INNER) and without LSNF_HMC_ADAPT, LSNF_HMC_METRIC_FOLD and LSNF_HMC_METRIC_CLOSE; with or without LSNF_HMC_RESAMPLE,
 *       which stays refused on an INIT call.
 *   beta_rows, beta_next: the search reads them at the group's rung 0; the caller keeps both equal on the rows of a group.
 * The search runs after the trajectory's decision and before the ANNEAL lines.  With {w_i, c_i} row i's Kahan pair BEFORE the increment
 * and el_s_i the likelihood energy of its state after the decision (an INIT call: the point's), i over the group's rungs.  Every line
 * is one fp32 operation, rounded once, no contraction.  `tree` is the xor-butterfly over the rungs, t1_i = x_i o x_{i^1}, t2_i = t1_i o
 * t1_{i^2}, .. (log2 P levels): +, fmaxf and fminf commute, so every row of the group holds the same bits.
 *         b = beta_rows[rung 0];  cap = beta_next[rung 0];  D = cap - b
 *         l_i = w_i - c_i;  m = tree fmaxf l_i;  W_i = expf(l_i - m);  S0 = tree + W_i
 *         emin = tree fminf el_s_i;  r_i = el_s_i - emin
 *         cess(x):  a_i = x * r_i;  v_i = expf(-a_i);  t_i = W_i * v_i;  q_i = t_i * v_i
 *                   N1 = tree + t_i;  N2 = tree + q_i;  cess = (N1 * N1) / (N2 * S0)
 *         if !(D > 0):                  beta' = b            (at or past its ceiling, or NaN: nothing moves)
 *         else if cess(D) >= cess_frac: beta' = cap          (exactly: the ceiling is reached)
 *         else lo = 0, hi = D;  12 times: mid = 0.5f * (lo + hi);  cess(mid) >= cess_frac ? lo = mid : hi = mid
 *              delta = fmaxf(lo, min_step);  beta' = fminf(b + delta, cap)
 *     (cess here is the conditional effective sample size over P, in (0, 1].)  Every row b of the group then runs the ANNEAL lines
 *     above with beta' in the place of beta_next[b] -- d = beta' - beta_rows[b], the weight increment, the re-tempering, beta_rows[b] <-
 *     beta' -- and the resampling move follows, unchanged, if its flag is set.  beta_next is not written.  A NaN in a row's el_s or
 *     weight makes every comparison false: the group advances by min_step and the resampling rule leaves it alone.  Twelve halvings
 *     resolve 1 / 4096 of the remaining span D.
 * Kernels: lsnf_small3_hmca_kernel / lsnf_small3_rhmca_kernel, the resampling kernels' stages, instantiations and workgroup shapes.  The
 * search is thirteen evaluations of cess, each two butterflies of log2 P lane exchanges, in the wave that holds the group's tile: no row
 * reads what another row writes in the same launch.  B = 0 succeeds without a launch. */
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
#define LSNF_HMC_INIT  1u
#define LSNF_HMC_INNER 2u
int lsnf_hmc_step(const float* plan, int nz, int width, int depth, int coupling, int B,
                  const float* z_prop, const float* z_out, const float* z_saved, const float* act_saved,
                  const float* ll_prop, const float* grad_g, const float* energy_g,
                  float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                  const float* noise, const float* uniform, const LsnfRng* rng, float step_size, unsigned flags,
                  float* z_next, float* accept_out, float* log_alpha_out, void* stream);
int lsnf_reverse_hmc_step(const float* plan, int nz, int width, int depth, int coupling, int B,
                          const float* eps_prop, const float* z_saved, const float* act_saved,
                          const float* grad_g, const float* energy_g,
                          float* eps_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                          const float* noise, const float* uniform, const LsnfRng* rng, float step_size, unsigned flags,
                          float* eps_next, float* accept_out, float* log_alpha_out, void* stream);

/* dual averaging of the rows' steps (Hoffman & Gelman 2014, algorithm 5); Stan's constants: 0.8, 0.05, 10, 0.75 */
typedef struct LsnfDualAvg { float target_accept, gamma, t0, kappa, step_min, step_max; } LsnfDualAvg;
#define LSNF_HMC_ADAPT      4u   /* end calls only: update the rows' adaptation state from this decision */
#define LSNF_HMC_ADAPT_LAST 8u   /* with ADAPT: the step written is exp(log_step_bar), the averaged one */
int lsnf_hmc_step_rows(const float* plan, int nz, int width, int depth, int coupling, int B,
                       const float* z_prop, const float* z_out, const float* z_saved, const float* act_saved,
                       const float* ll_prop, const float* grad_g, const float* energy_g,
                       float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                       const float* noise, const float* uniform, const LsnfRng* rng,
                       float* step_rows, float* adapt, const LsnfDualAvg* da, unsigned flags,
                       float* z_next, float* accept_out, float* log_alpha_out, void* stream);
int lsnf_reverse_hmc_step_rows(const float* plan, int nz, int width, int depth, int coupling, int B,
                               const float* eps_prop, const float* z_saved, const float* act_saved,
                               const float* grad_g, const float* energy_g,
                               float* eps_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                               const float* noise, const float* uniform, const LsnfRng* rng,
                               float* step_rows, float* adapt, const LsnfDualAvg* da, unsigned flags,
                               float* eps_next, float* accept_out, float* log_alpha_out, void* stream);

/* a diagonal metric per row: the regularisation of a window's variance and the clamp of the scale; Stan's n0 = 5, var0 = 1e-3 */
typedef struct LsnfMetricReg { float n0, var0, scale_min, scale_max; } LsnfMetricReg;
#define LSNF_HMC_METRIC_FOLD  16u   /* end calls only: fold the state after the decision into the row's window */
#define LSNF_HMC_METRIC_CLOSE 32u   /* with METRIC_FOLD: close the window -- write the new scale, zero the accumulators */
int lsnf_hmc_step_metric(const float* plan, int nz, int width, int depth, int coupling, int B,
                         const float* z_prop, const float* z_out, const float* z_saved, const float* act_saved,
                         const float* ll_prop, const float* grad_g, const float* energy_g,
                         float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                         const float* noise, const float* uniform, const LsnfRng* rng,
                         float* step_rows, float* adapt, const LsnfDualAvg* da,
                         float* scale_rows, float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg, unsigned flags,
                         float* z_next, float* accept_out, float* log_alpha_out, void* stream);
int lsnf_reverse_hmc_step_metric(const float* plan, int nz, int width, int depth, int coupling, int B,
                                 const float* eps_prop, const float* z_saved, const float* act_saved,
                                 const float* grad_g, const float* energy_g,
                                 float* eps_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                                 const float* noise, const float* uniform, const LsnfRng* rng,
                                 float* step_rows, float* adapt, const LsnfDualAvg* da,
                                 float* scale_rows, float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg, unsigned flags,
                                 float* eps_next, float* accept_out, float* log_alpha_out, void* stream);

/* a likelihood temperature per row (tempered transitions, annealed importance sampling) */
#define LSNF_HMC_ANNEAL 64u   /* INIT and end calls: weigh the state after the decision, re-temper it to beta_next */
int lsnf_hmc_step_tempered(const float* plan, int nz, int width, int depth, int coupling, int B,
                           const float* z_prop, const float* z_out, const float* z_saved, const float* act_saved,
                           const float* ll_prop, const float* grad_g, const float* energy_g,
                           float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                           const float* noise, const float* uniform, const LsnfRng* rng,
                           float* step_rows, float* adapt, const LsnfDualAvg* da,
                           float* scale_rows, float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg,
                           float* beta_rows, const float* beta_next, float* like_grad_acc, float* like_u_acc, float* log_w, unsigned flags,
                           float* z_next, float* accept_out, float* log_alpha_out, void* stream);
int lsnf_reverse_hmc_step_tempered(const float* plan, int nz, int width, int depth, int coupling, int B,
                                   const float* eps_prop, const float* z_saved, const float* act_saved,
                                   const float* grad_g, const float* energy_g,
                                   float* eps_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                                   const float* noise, const float* uniform, const LsnfRng* rng,
                                   float* step_rows, float* adapt, const LsnfDualAvg* da,
                                   float* scale_rows, float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg,
                                   float* beta_rows, const float* beta_next, float* like_grad_acc, float* like_u_acc, float* log_w,
                                   unsigned flags, float* eps_next, float* accept_out, float* log_alpha_out, void* stream);

/* replica exchange between the rows of a ladder (parallel tempering) */
#define LSNF_HMC_SWAP 128u       /* end calls: exchange the states of paired rungs after the decision */
#define LSNF_HMC_SWAP_ODD 256u   /* with LSNF_HMC_SWAP: pair rungs (1,2), (3,4), .. instead of (0,1), (2,3), .. */
int lsnf_hmc_step_exchange(const float* plan, int nz, int width, int depth, int coupling, int B,
                           const float* z_prop, const float* z_out, const float* z_saved, const float* act_saved,
                           const float* ll_prop, const float* grad_g, const float* energy_g,
                           float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                           const float* noise, const float* uniform, const LsnfRng* rng,
                           float* step_rows, float* adapt, const LsnfDualAvg* da,
                           float* scale_rows, float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg,
                           float* beta_rows, const float* beta_next, float* like_grad_acc, float* like_u_acc, float* log_w, unsigned flags,
                           float* z_next, float* accept_out, float* log_alpha_out,
                           int ladder, const float* swap_uniform, float* swap_out, float* log_swap_out, void* stream);
int lsnf_reverse_hmc_step_exchange(const float* plan, int nz, int width, int depth, int coupling, int B,
                                   const float* eps_prop, const float* z_saved, const float* act_saved,
                                   const float* grad_g, const float* energy_g,
                                   float* eps_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                                   const float* noise, const float* uniform, const LsnfRng* rng,
                                   float* step_rows, float* adapt, const LsnfDualAvg* da,
                                   float* scale_rows, float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg,
                                   float* beta_rows, const float* beta_next, float* like_grad_acc, float* like_u_acc, float* log_w,
                                   unsigned flags, float* eps_next, float* accept_out, float* log_alpha_out,
                                   int ladder, const float* swap_uniform, float* swap_out, float* log_swap_out, void* stream);

/* resampling between the rows of a group (sequential Monte Carlo) */
#define LSNF_HMC_RESAMPLE 512u   /* annealing end calls: resample the group's states when its effective sample size is low */
int lsnf_hmc_step_resample(const float* plan, int nz, int width, int depth, int coupling, int B,
                           const float* z_prop, const float* z_out, const float* z_saved, const float* act_saved,
                           const float* ll_prop, const float* grad_g, const float* energy_g,
                           float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                           const float* noise, const float* uniform, const LsnfRng* rng,
                           float* step_rows, float* adapt, const LsnfDualAvg* da,
                           float* scale_rows, float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg,
                           float* beta_rows, const float* beta_next, float* like_grad_acc, float* like_u_acc, float* log_w, unsigned flags,
                           float* z_next, float* accept_out, float* log_alpha_out,
                           int group, float ess_frac, const float* resample_uniform, float* ancestor_out, float* ess_out, void* stream);
int lsnf_reverse_hmc_step_resample(const float* plan, int nz, int width, int depth, int coupling, int B,
                                   const float* eps_prop, const float* z_saved, const float* act_saved,
                                   const float* grad_g, const float* energy_g,
                                   float* eps_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                                   const float* noise, const float* uniform, const LsnfRng* rng,
                                   float* step_rows, float* adapt, const LsnfDualAvg* da,
                                   float* scale_rows, float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg,
                                   float* beta_rows, const float* beta_next, float* like_grad_acc, float* like_u_acc, float* log_w,
                                   unsigned flags, float* eps_next, float* accept_out, float* log_alpha_out,
                                   int group, float ess_frac, const float* resample_uniform, float* ancestor_out, float* ess_out,
                                   void* stream);

/* the groups' next temperature searched in the annealing call (adaptive tempering) */
#define LSNF_HMC_SCHEDULE 1024u  /* INIT and end calls with ANNEAL: beta_next is the ceiling, the step is found from the particles */
int lsnf_hmc_step_schedule(const float* plan, int nz, int width, int depth, int coupling, int B,
                           const float* z_prop, const float* z_out, const float* z_saved, const float* act_saved,
                           const float* ll_prop, const float* grad_g, const float* energy_g,
                           float* z_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                           const float* noise, const float* uniform, const LsnfRng* rng,
                           float* step_rows, float* adapt, const LsnfDualAvg* da,
                           float* scale_rows, float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg,
                           float* beta_rows, const float* beta_next, float* like_grad_acc, float* like_u_acc, float* log_w, unsigned flags,
                           float* z_next, float* accept_out, float* log_alpha_out,
                           int group, float ess_frac, const float* resample_uniform, float* ancestor_out, float* ess_out,
                           float cess_frac, float min_step, void* stream);
int lsnf_reverse_hmc_step_schedule(const float* plan, int nz, int width, int depth, int coupling, int B,
                                   const float* eps_prop, const float* z_saved, const float* act_saved,
                                   const float* grad_g, const float* energy_g,
                                   float* eps_acc, float* grad_acc, float* u_acc, float* mom, float* kin0,
                                   const float* noise, const float* uniform, const LsnfRng* rng,
                                   float* step_rows, float* adapt, const LsnfDualAvg* da,
                                   float* scale_rows, float* mean_rows, float* m2_rows, float* count_rows, const LsnfMetricReg* reg,
                                   float* beta_rows, const float* beta_next, float* like_grad_acc, float* like_u_acc, float* log_w,
                                   unsigned flags, float* eps_next, float* accept_out, float* log_alpha_out,
                                   int group, float ess_frac, const float* resample_uniform, float* ancestor_out, float* ess_out,
                                   float cess_frac, float min_step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LSNF_FLOW_MCMC_H */

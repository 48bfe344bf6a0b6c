"""Caller-side harness around the flow prior: the reference's short-run Langevin sampler and flow-MLE step,
restated (they are closures inside train.py and cannot be imported) on top of the fused kernels.

  sample_langevin_post_z_with_flow  <- train.py:307-335 (training) / :602-634 (testing: 20x steps, no noise)
  sample_mala_post_z_with_flow         the same chain Metropolis-adjusted (exact at any step size; per-row acceptance rate)
  sample_hmc_post_z_with_flow          Hamiltonian Monte Carlo on the same target: L leapfrog steps per accept / reject
  sample_hmc_adaptive_post_z_with_flow    ... with a step per row, adapted on the device during a warm-up (dual averaging)
  sample_langevin_post_eps_with_flow   the same sampler in the flow's base space (eps, with z = f^-1(eps)); not in the reference
  sample_mala_post_eps_with_flow       the base-space chain Metropolis-adjusted (per-row acceptance rate)
  sample_hmc_post_eps_with_flow        Hamiltonian Monte Carlo in the base space: L leapfrog steps per accept / reject
  sample_hmc_adaptive_post_eps_with_flow  ... with a step per row, adapted on the device during a warm-up (dual averaging)
  flow_mle_step                     <- train.py:404-415
  sample_x                          <- train.py:472-478 (prior samples for the FID evaluation)

The generator `netG` is any `nn.Module` mapping (B, nz, 1, 1) -> images (the reference's `_netG`, stock PyTorch /
MIOpen, is out of scope of this build and used as is); its z-gradient comes from torch autograd exactly as in the
reference, the flow's comes from `lsnf_langevin_step` (two launches per step instead of ~750 eager kernels)."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn


def sample_langevin_post_z_with_flow(z, x, netG: nn.Module, netF, *, g_l_steps: int, g_l_step_size: float,
                                     g_llhd_sigma: float, g_l_with_noise: bool = True,
                                     generator: Optional[torch.Generator] = None, philox=None):
    """Returns (z_k detached (B,nz,1,1), mean |z_grad_g|, mean |z_grad_f|, f_log_lkhd of the last step's input).
    Noise (train.py:325-326): `torch.randn` draws (optionally from `generator`), or, with `philox` =
    `flow.PhiloxNoise(seed, offset, row0)`, drawn inside the update kernel (step k uses offset + k): no randn
    launch, no (B, nz) noise tensor, and the same draws however the rows are sharded over GPUs.  On return `philox` has
    been ADVANCED by g_l_steps (in place): a generator object kept across training iterations continues its stream
    instead of repeating it."""
    z = z.clone().detach()
    B, nz = z.shape[0], z.shape[1]
    mse = nn.MSELoss(reduction="sum")
    gg_norm = gf_norm = f_log_lkhd = None
    for k in range(g_l_steps):
        z.requires_grad_(True)
        x_hat = netG(z)                                                                      # train.py:312
        g_log_lkhd = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma) * mse(x_hat, x)               # train.py:313
        z_grad_g = torch.autograd.grad(g_log_lkhd, z)[0]                                     # train.py:314
        z2d = z.detach().view(B, nz)
        noise = None
        if g_l_with_noise:                                                                   # train.py:325-326
            noise = philox.step(k) if philox is not None else \
                torch.randn(z2d.shape, device=z2d.device, dtype=z2d.dtype, generator=generator)
        z_new, ll, gf, gg = netF.langevin_step(z2d, z_grad_g.reshape(B, nz), noise, g_l_step_size,    # :316-326
                                               reuse_buffers=True)
        f_log_lkhd = -ll.sum()                                                               # train.py:320
        gg_norm, gf_norm = gg.mean(), gf.mean()                                              # train.py:328-329
        z = z_new.view(B, nz, 1, 1)
    if philox is not None and g_l_with_noise:
        philox.advance(g_l_steps)
    return z.detach(), gg_norm, gf_norm, f_log_lkhd


def sample_mala_post_z_with_flow(z, x, netG: nn.Module, netF, *, g_l_steps: int, g_l_step_size: float, g_llhd_sigma: float, philox):
    """The sampler above Metropolis-adjusted (MALA): the same proposal z' = z - s^2/2 grad U(z) + s xi, accepted with probability
    min(1, pi(z') q(z|z') / (pi(z) q(z'|z))), so the chain is exact for p(z|x) ~ p_flow(z) p(x|G(z)) at any step size and its
    acceptance rate tells whether g_l_step_size is sound.  U = |x - G(z)|^2 / (2 sigma^2) - ll(z) per row; the generator's energy and
    gradient come from torch autograd as in train.py:312-314 (the sum over pixels kept per row), the flow's part, the decision and
    the next proposal from `netF.mala_step`.  K = g_l_steps proposals take K + 1 evaluations: call 0 starts the chain at z, calls
    1 .. K-1 decide a proposal and make the next, call K decides only.  `philox` (a `flow.PhiloxNoise`, required) gives call j its
    uniform and its noise at offset + j and is ADVANCED by K + 1 on return.
    Returns (z_k (B, nz, 1, 1), accept_rate (B) = accepted proposals / K, U(z_k) (B)); g_l_steps = 0 or an empty batch returns the
    input (and None, None)."""
    from . import flow
    B, nz = z.shape[0], z.shape[1]
    if g_l_steps < 1 or B == 0:
        return z.detach().clone().view(B, nz, 1, 1), None, None
    K, c = int(g_l_steps), 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    z_prop = z.detach().reshape(B, nz).contiguous().clone()
    state = flow.new_mala_state(netF._plan(), B, z_prop.device)
    accepted = torch.zeros(B, dtype=torch.float32, device=z_prop.device)
    for j in range(K + 1):
        zr = z_prop.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = c * ((netG(zr) - x) ** 2).flatten(1).sum(1)                                 # train.py:312-313, per row
        grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
        _, acc, _, _ = netF.mala_step(z_prop, grad_g, energy.detach(), state, philox.step(j), g_l_step_size, init=j == 0,
                                      propose=j < K, inplace=True, reuse_buffers=True)
        if j:
            accepted += acc
    philox.advance(K + 1)
    return state.z.view(B, nz, 1, 1), accepted / K, state.energy


def sample_hmc_post_z_with_flow(z, x, netG: nn.Module, netF, *, g_l_steps: int, leapfrog_steps: int, g_l_step_size: float,
                                g_llhd_sigma: float, philox):
    """Hamiltonian Monte Carlo on the target of `sample_mala_post_z_with_flow`: K = g_l_steps trajectories of L = leapfrog_steps
    leapfrog steps of size g_l_step_size, one accept / reject per trajectory -- L times the distance of a MALA proposal for one
    decision (L = 1 is that chain in exact arithmetic).  U = |x - G(z)|^2 / (2 sigma^2) - ll(z) per row; the generator's energy and
    gradient come from torch autograd at every one of the K L + 1 points, exactly as there, the flow's part, the leapfrog
    arithmetic, the decision and the next trajectory's start from `netF.hmc_step`: one "init" call, then per trajectory L - 1
    "inner" calls and one "end" call, the last of which proposes nothing.  `philox` (a `flow.PhiloxNoise`, required) gives the call
    that starts trajectory t + 1 -- the init call is t = 0, end call t is 1 .. K -- its uniform and its momentum draw at offset + t;
    inner calls take no generator; it is ADVANCED by K + 1 on return.
    Returns (z_k (B, nz, 1, 1), accept_rate (B) = accepted trajectories / K, U(z_k) (B)); g_l_steps = 0 or an empty batch returns
    the input (and None, None); leapfrog_steps < 1 raises ValueError."""
    from . import flow
    K, L = int(g_l_steps), int(leapfrog_steps)
    if L < 1:
        raise ValueError(f"leapfrog_steps must be >= 1 (got {leapfrog_steps})")
    B, nz = z.shape[0], z.shape[1]
    if K < 1 or B == 0:
        return z.detach().clone().view(B, nz, 1, 1), None, None
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    z_prop = z.detach().reshape(B, nz).contiguous().clone()
    state = flow.new_hmc_state(netF._plan(), B, z_prop.device)
    accepted = torch.zeros(B, dtype=torch.float32, device=z_prop.device)
    for j in range(K * L + 1):
        zr = z_prop.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = c * ((netG(zr) - x) ** 2).flatten(1).sum(1)                                 # train.py:312-313, per row
        grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
        t, inner = j // L, j % L != 0
        _, acc, _, _ = netF.hmc_step(z_prop, grad_g, energy.detach(), state, None if inner else philox.step(t), g_l_step_size,
                                     phase="inner" if inner else "end" if j else "init", propose=j < K * L, inplace=True,
                                     reuse_buffers=True)
        if j and not inner:
            accepted += acc
    philox.advance(K + 1)
    return state.z.view(B, nz, 1, 1), accepted / K, state.energy


def _adaptive_plan(g_l_steps, leapfrog_steps, warmup_steps, steps):
    """(K, L, W) of an adaptive sampler, checked with `steps`; `mode(t)`: what end call t = 1 .. K does to the rows' steps."""
    from . import flow
    K, L, W = int(g_l_steps), int(leapfrog_steps), int(warmup_steps)
    if steps is not None and not isinstance(steps, flow.HmcRowSteps):
        raise flow.LsnfError("steps must be a flow.HmcRowSteps (new_hmc_row_steps()), or None")
    if L < 1:
        raise ValueError(f"leapfrog_steps must be >= 1 (got {leapfrog_steps})")
    if W < 0 or (K >= 1 and W > K):
        raise ValueError(f"warmup_steps must lie in 0 .. g_l_steps (got {warmup_steps} of {g_l_steps})")
    return K, L, W, (lambda t: None if t > W else "last" if t == W else "update")


def _row_steps(flow, steps, B, device, g_l_step_size, target_accept):
    return flow.new_hmc_row_steps(B, device, g_l_step_size, target_accept=target_accept) if steps is None else steps


def sample_hmc_adaptive_post_z_with_flow(z, x, netG: nn.Module, netF, *, g_l_steps: int, leapfrog_steps: int, warmup_steps: int,
                                         g_l_step_size, g_llhd_sigma: float, philox, target_accept: float = 0.8, steps=None):
    """`sample_hmc_post_z_with_flow` with a step per row, adapted during a warm-up: every row targets its own posterior
    p(z | x_b), so every row gets its own leapfrog step, tuned on the device by dual averaging toward the acceptance rate
    `target_accept` (Hoffman & Gelman 2014, as Stan and NumPyro do it) inside the kernel that decides a trajectory
    (`netF.hmc_step_rows`) -- no host round trip, the flow's side of a step stays at its two launches.  The first `warmup_steps` of the
    K = g_l_steps end calls adapt ("update"), the last of them writes the averaged step ("last"); the remaining K - warmup_steps
    trajectories run at those frozen steps and are an exact chain.  g_l_step_size: the first step, a float or a (B) tensor (the
    update's mu is log(10 * it)); `steps`: a `flow.HmcRowSteps` to go on from instead (g_l_step_size and target_accept are then
    not read) -- it is updated in place.  Calls, draws and `philox` as `sample_hmc_post_z_with_flow`'s; with warmup_steps = 0 and a
    float g_l_step_size the result is that sampler's, bit for bit.
    Returns (z_k (B, nz, 1, 1), accept_rate (B) over the trajectories after the warm-up -- over all K when warmup_steps is 0 or K --,
    U(z_k) (B), the `flow.HmcRowSteps`); g_l_steps = 0 or an empty batch returns the input (and None, None, `steps`)."""
    from . import flow
    K, L, W, mode = _adaptive_plan(g_l_steps, leapfrog_steps, warmup_steps, steps)
    B, nz = z.shape[0], z.shape[1]
    if K < 1 or B == 0:
        return z.detach().clone().view(B, nz, 1, 1), None, None, steps
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    z_prop = z.detach().reshape(B, nz).contiguous().clone()
    steps = _row_steps(flow, steps, B, z_prop.device, g_l_step_size, target_accept)
    state = flow.new_hmc_state(netF._plan(), B, z_prop.device)
    accepted = torch.zeros(B, dtype=torch.float32, device=z_prop.device)
    counted = K - W if W < K else K
    for j in range(K * L + 1):
        zr = z_prop.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = c * ((netG(zr) - x) ** 2).flatten(1).sum(1)                                 # train.py:312-313, per row
        grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
        t, inner = j // L, j % L != 0
        _, acc, _, _ = netF.hmc_step_rows(z_prop, grad_g, energy.detach(), state, None if inner else philox.step(t), steps,
                                          phase="inner" if inner else "end" if j else "init", propose=j < K * L, inplace=True,
                                          reuse_buffers=True, adapt=None if inner or not j else mode(t))
        if j and not inner and (t > W or counted == K):
            accepted += acc
    philox.advance(K + 1)
    return state.z.view(B, nz, 1, 1), accepted / counted, state.energy, steps


def warmup_windows(W: int, init_buffer: int = 75, term_buffer: int = 50, base_window: int = 25):
    """Stan's warm-up schedule for W trajectories, numbered 1 .. W: a fast initial buffer, a slow phase init_buffer + 1 .. W -
    term_buffer of windows in which the metric is estimated -- the first `base_window` long, every next one twice as long, a window
    extended to the slow phase's end when the one after it would not fit entirely --, a fast final buffer.  If the three do not fit
    (init + base + term > W) the buffers become int(0.15 W) and int(0.1 W) and the base window the rest; W < 20 has no window.
    Returns (first, closes): the first trajectory whose end call folds, and the trajectories whose end calls close a window
    (None and [] without a window)."""
    W = int(W)
    if W < 20:
        return None, []
    init, term, size = int(init_buffer), int(term_buffer), int(base_window)
    if init + size + term > W:
        init, term = int(0.15 * W), int(0.1 * W)
        size = W - init - term
    end, close, closes = W - term, init + size, []
    while True:
        if close + 2 * size > end:          # the window after this one would not fit: this one takes the rest
            close = end
        closes.append(close)
        if close >= end:
            return init + 1, closes
        size *= 2
        close += size


def _metric_plan(flow, metric, windows, W):
    """(first, closes) of a metric sampler -- `windows` or `warmup_windows(W)` -- checked with `metric`; `window(t)`: what end call
    t = 1 .. K does to the rows' windows."""
    if metric is not None and not isinstance(metric, flow.HmcRowMetric):
        raise flow.LsnfError("metric must be a flow.HmcRowMetric (new_hmc_row_metric()), or None")
    first, closes = warmup_windows(W) if windows is None else windows
    closes = [int(c) for c in closes]
    if closes and (first is None or any(b <= a for a, b in zip([int(first) - 1] + closes, closes))):
        raise ValueError(f"windows: the closes must increase from first on (got first={first}, closes={closes})")
    last = closes[-1] if closes else 0
    return lambda t: None if not closes or t < first or t > last else "close" if t in closes else "fold"


def sample_hmc_metric_post_z_with_flow(z, x, netG: nn.Module, netF, *, g_l_steps: int, leapfrog_steps: int, warmup_steps: int,
                                       g_l_step_size, g_llhd_sigma: float, philox, target_accept: float = 0.8, steps=None, metric=None,
                                       windows=None):
    """`sample_hmc_adaptive_post_z_with_flow` with a diagonal metric per row, estimated on the device in the warm-up's windows
    (`netF.hmc_step_metric`; Stan's / NumPyro's warm-up): without one the stiffest coordinate of p(z | x_b) sets a row's step and the
    chain barely moves in the soft ones.  The step adapts on every warm-up end call ("last" on the W-th); the end calls of
    trajectories first .. the last close fold the decided state into the row's window and the closes turn a window into the row's
    scales and restart the step adaptation (`windows` = (first, closes), default `warmup_windows(warmup_steps)`).  `metric`: a
    `flow.HmcRowMetric` to go on from (updated in place; default a unit one).  Calls, draws and `philox` are the adaptive sampler's;
    with windows=(None, []) and a fresh unit metric the result is that sampler's, bit for bit.
    Returns that sampler's tuple and the `flow.HmcRowMetric`: (z_k, accept_rate, U(z_k), steps, metric)."""
    from . import flow
    K, L, W, mode = _adaptive_plan(g_l_steps, leapfrog_steps, warmup_steps, steps)
    window = _metric_plan(flow, metric, windows, W)
    B, nz = z.shape[0], z.shape[1]
    if K < 1 or B == 0:
        return z.detach().clone().view(B, nz, 1, 1), None, None, steps, metric
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    z_prop = z.detach().reshape(B, nz).contiguous().clone()
    steps = _row_steps(flow, steps, B, z_prop.device, g_l_step_size, target_accept)
    metric = flow.new_hmc_row_metric(netF._plan(), B, z_prop.device) if metric is None else metric
    state = flow.new_hmc_state(netF._plan(), B, z_prop.device)
    accepted = torch.zeros(B, dtype=torch.float32, device=z_prop.device)
    counted = K - W if W < K else K
    for j in range(K * L + 1):
        zr = z_prop.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = c * ((netG(zr) - x) ** 2).flatten(1).sum(1)                                 # train.py:312-313, per row
        grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
        t, inner = j // L, j % L != 0
        end = bool(j) and not inner
        _, acc, _, _ = netF.hmc_step_metric(z_prop, grad_g, energy.detach(), state, None if inner else philox.step(t), steps, metric,
                                            phase="inner" if inner else "end" if j else "init", propose=j < K * L, inplace=True,
                                            reuse_buffers=True, adapt=mode(t) if end else None, window=window(t) if end else None)
        if end and (t > W or counted == K):
            accepted += acc
    philox.advance(K + 1)
    return state.z.view(B, nz, 1, 1), accepted / counted, state.energy, steps, metric


def sample_langevin_post_eps_with_flow(eps, x, netG: nn.Module, netF, *, g_l_steps: int, g_l_step_size: float,
                                       g_llhd_sigma: float, noise: bool = True, philox=None, fused: bool = False):
    """The sampler above in the flow's BASE space: Langevin on eps with z = f^-1(eps), target
    p(eps | x) ~ N(eps; 0, I) * p(x | g(f^-1(eps))) -- the flow's Jacobian cancels against the prior's density, so the prior's
    gradient is eps itself and the flow enters only through the pull-back of the generator's gradient.  Per step:
        z      = f^-1(eps)                                  the reverse launch, which keeps its backward's stash
        grad_g = d/dz 1/(2 sigma^2) |g(z) - x|^2            torch autograd through netG, as train.py:312-314
        g_eps  = J_{f^-1}(eps)^T grad_g                     `flow.reverse_backward_z`
        eps   <- eps - 0.5 s^2 (eps + g_eps) [+ s * noise]  torch ops
    -- two flow launches per step where `flow.reverse_keep_supported` (the latency bf16x3 reverse, up to the small-batch
    threshold); elsewhere three (reverse, forward at z, backward).  noise: `torch.randn` draws, or, with `philox` =
    `flow.PhiloxNoise`, the in-kernel stream of the other samplers for step k at offset + k (drawn by a sampling launch of its own
    whose x is discarded; `philox` is ADVANCED by g_l_steps on return).
    fused=True: the last two lines are ONE launch, `flow.reverse_langevin_step` -- the backward with the update as its output
    section (fp32 fused multiply-adds: the last bits differ from the torch ops'), the per-row norms from the same kernel, and with
    `philox` the noise of step k drawn inside it at offset + k: the sampling launch disappears, the flow's part of a step is the
    reverse and this launch.  `GraphedEpsLangevinSampler` replays that step from a captured graph.
    eps: (B, nz) or (B, nz, 1, 1).  Returns (eps_k (B, nz), z_k = f^-1(eps_k) (B, nz, 1, 1), mean |g_eps|, mean |eps|): the last two
    are the per-row norms of the likelihood's and the prior's gradient at the last step's input, as the z-space sampler's (None
    if no step ran: g_l_steps = 0, or an empty batch, which comes back as it is without a launch)."""
    from . import flow
    B, nz = eps.shape[0], eps.shape[1]
    eps = eps.detach().reshape(B, nz).contiguous().clone()
    if B == 0:
        return eps, eps.view(0, nz, 1, 1), None, None
    plan = netF._plan()
    keeps = flow.reverse_keep_supported(plan, B)
    act = flow.new_act_saved(plan, B, eps.device)
    mse = nn.MSELoss(reduction="sum")
    gg_norm = gf_norm = None
    s = float(g_l_step_size)
    with torch.no_grad():
        for k in range(g_l_steps):
            if keeps:
                z, _, saved = flow.reverse(plan, eps, None, save_for_backward=True, act_saved=act)
                z_last = eps
            else:
                z, _ = flow.reverse(plan, eps, None)
                z_last, _, _, saved = flow.forward(plan, z, None, want_ll=False, save_for_backward=True, act_saved=act)
            with torch.enable_grad():
                zr = z.view(B, nz, 1, 1).requires_grad_(True)
                g_log_lkhd = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma) * mse(netG(zr), x)        # train.py:312-313
                grad_g = torch.autograd.grad(g_log_lkhd, zr)[0].reshape(B, nz).contiguous()     # train.py:314
            if fused:
                # (the kernel's z_out is the point it updates: eps itself, also where the forward at z wrote its own last output, which
                #  is eps up to the round trip's rounding)
                xi = None if not noise else philox.step(k) if philox is not None else torch.randn_like(eps)
                eps, _, gn, en = flow.reverse_langevin_step(plan, eps, saved, act, grad_g, xi, s)
                gg_norm, gf_norm = gn.mean(), en.mean()
                continue
            g_eps = flow.reverse_backward_z(plan, z_last, saved, act, grad_g, None)
            gg_norm, gf_norm = g_eps.norm(dim=1).mean(), eps.norm(dim=1).mean()
            new = eps - 0.5 * s * s * (eps + g_eps)
            if noise:
                if philox is not None:
                    draw = flow.sample(plan, B, philox.step(k), want_eps=True)[2]
                else:
                    draw = torch.randn_like(eps)
                new = new + s * draw
            eps = new
        z = flow.reverse(plan, eps, None)[0]
    if philox is not None and noise:
        philox.advance(g_l_steps)
    return eps, z.view(B, nz, 1, 1), gg_norm, gf_norm


def sample_mala_post_eps_with_flow(eps, x, netG: nn.Module, netF, *, g_l_steps: int, g_l_step_size: float, g_llhd_sigma: float, philox):
    """The base-space sampler above Metropolis-adjusted (MALA): target p(eps | x) ~ N(eps; 0, I) * p(x | G(f^-1(eps))), i.e.
    U(eps) = |eps|^2 / 2 + |x - G(z)|^2 / (2 sigma^2) with z = f^-1(eps) (the flow's log-determinant cancels), the proposal
    eps' = eps - s^2/2 grad U(eps) + s xi of `flow.reverse_langevin_step`, accepted with probability
    min(1, pi(eps') q(eps|eps') / (pi(eps) q(eps'|eps))): exact at the large steps the flow's preconditioning permits, and the
    acceptance rate tells whether g_l_step_size is sound.  K = g_l_steps proposals take K + 1 evaluations; call j:
        z      = f^-1(eps_prop)                      the reverse launch, keeping its backward's stash where
                                                     `flow.reverse_keep_supported` (else reverse + forward at z)
        energy, grad_g                               torch autograd through netG, per row, as `sample_mala_post_z_with_flow`
        `netF.reverse_mala_step`                     decides eps_prop, updates the state, proposes again (j < K), in place
    with `philox` (a `flow.PhiloxNoise`, required) giving call j its uniform and its noise at offset + j; it is ADVANCED by K + 1
    on return.  eps: (B, nz) or (B, nz, 1, 1).
    Returns (eps_k (B, nz), z_k = f^-1(eps_k) (B, nz, 1, 1) from one final reverse at the state, accept_rate (B) = accepted
    proposals / K, U(eps_k) (B)).  g_l_steps = 0 or an empty batch returns the input without a launch, with None rates:
    (eps, None, None, None), an empty batch with its empty z."""
    from . import flow
    B, nz = eps.shape[0], eps.shape[1]
    eps_prop = eps.detach().reshape(B, nz).contiguous().clone()
    if B == 0:
        return eps_prop, eps_prop.view(0, nz, 1, 1), None, None
    if g_l_steps < 1:
        return eps_prop, None, None, None
    plan = netF._plan()
    K, c = int(g_l_steps), 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    keeps = flow.reverse_keep_supported(plan, B)
    act = flow.new_act_saved(plan, B, eps_prop.device)
    state = flow.new_mala_state(plan, B, eps_prop.device)
    accepted = torch.zeros(B, dtype=torch.float32, device=eps_prop.device)
    with torch.no_grad():
        for j in range(K + 1):
            if keeps:
                z, _, saved = flow.reverse(plan, eps_prop, None, save_for_backward=True, act_saved=act)
            else:
                z, _ = flow.reverse(plan, eps_prop, None)
                saved = flow.forward(plan, z, None, want_ll=False, save_for_backward=True, act_saved=act)[3]
            with torch.enable_grad():
                zr = z.view(B, nz, 1, 1).requires_grad_(True)
                energy = c * ((netG(zr) - x) ** 2).flatten(1).sum(1)                                 # train.py:312-313, per row
                grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
            _, acc, _ = netF.reverse_mala_step(eps_prop, saved, act, grad_g, energy.detach(), state, philox.step(j), g_l_step_size,
                                               init=j == 0, propose=j < K, inplace=True, reuse_buffers=True)
            if j:
                accepted += acc
        z = flow.reverse(plan, state.z, None)[0]
    philox.advance(K + 1)
    return state.z, z.view(B, nz, 1, 1), accepted / K, state.energy


def sample_hmc_post_eps_with_flow(eps, x, netG: nn.Module, netF, *, g_l_steps: int, leapfrog_steps: int, g_l_step_size: float,
                                  g_llhd_sigma: float, philox):
    """Hamiltonian Monte Carlo on the target of `sample_mala_post_eps_with_flow`, U(eps) = |eps|^2 / 2 + |x - G(z)|^2 / (2 sigma^2)
    with z = f^-1(eps): K = g_l_steps trajectories of L = leapfrog_steps leapfrog steps of size g_l_step_size, one accept / reject
    per trajectory (L = 1 is that chain in exact arithmetic).  The flow has whitened the prior, so for the prior's part the identity mass matrix of the
    momentum is the right one (an informative likelihood: `sample_hmc_metric_post_eps_with_flow`) and long trajectories stay stable at steps the z-space chain cannot take.  Each of the K L + 1 points:
        z      = f^-1(eps_prop)                      the reverse launch, keeping its backward's stash where
                                                     `flow.reverse_keep_supported` (else reverse + forward at z)
        energy, grad_g                               torch autograd through netG, per row, as `sample_mala_post_eps_with_flow`
        `netF.reverse_hmc_step`                      the leapfrog arithmetic, the decision and the next trajectory's start, in place:
                                                     one "init" call, then per trajectory L - 1 "inner" calls and one "end" call,
                                                     the last of which proposes nothing
    `philox` (a `flow.PhiloxNoise`, required) gives the call that starts trajectory t + 1 -- the init call is t = 0, end call t is
    1 .. K -- its uniform and its momentum draw at offset + t; inner calls take no generator; it is ADVANCED by K + 1 on return.
    eps: (B, nz) or (B, nz, 1, 1).
    Returns (eps_k (B, nz), z_k = f^-1(eps_k) (B, nz, 1, 1) from one final reverse at the state, accept_rate (B) = accepted
    trajectories / K, U(eps_k) (B)).  g_l_steps = 0 or an empty batch returns the input without a launch, with None rates:
    (eps, None, None, None), an empty batch with its empty z; leapfrog_steps < 1 raises ValueError."""
    from . import flow
    K, L = int(g_l_steps), int(leapfrog_steps)
    if L < 1:
        raise ValueError(f"leapfrog_steps must be >= 1 (got {leapfrog_steps})")
    B, nz = eps.shape[0], eps.shape[1]
    eps_prop = eps.detach().reshape(B, nz).contiguous().clone()
    if B == 0:
        return eps_prop, eps_prop.view(0, nz, 1, 1), None, None
    if K < 1:
        return eps_prop, None, None, None
    plan = netF._plan()
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    keeps = flow.reverse_keep_supported(plan, B)
    act = flow.new_act_saved(plan, B, eps_prop.device)
    state = flow.new_hmc_state(plan, B, eps_prop.device)
    accepted = torch.zeros(B, dtype=torch.float32, device=eps_prop.device)
    with torch.no_grad():
        for j in range(K * L + 1):
            if keeps:
                z, _, saved = flow.reverse(plan, eps_prop, None, save_for_backward=True, act_saved=act)
            else:
                z, _ = flow.reverse(plan, eps_prop, None)
                saved = flow.forward(plan, z, None, want_ll=False, save_for_backward=True, act_saved=act)[3]
            with torch.enable_grad():
                zr = z.view(B, nz, 1, 1).requires_grad_(True)
                energy = c * ((netG(zr) - x) ** 2).flatten(1).sum(1)                                 # train.py:312-313, per row
                grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
            t, inner = j // L, j % L != 0
            _, acc, _ = netF.reverse_hmc_step(eps_prop, saved, act, grad_g, energy.detach(), state, None if inner else philox.step(t),
                                              g_l_step_size, phase="inner" if inner else "end" if j else "init", propose=j < K * L,
                                              inplace=True, reuse_buffers=True)
            if j and not inner:
                accepted += acc
        z = flow.reverse(plan, state.z, None)[0]
    philox.advance(K + 1)
    return state.z, z.view(B, nz, 1, 1), accepted / K, state.energy


def sample_hmc_adaptive_post_eps_with_flow(eps, x, netG: nn.Module, netF, *, g_l_steps: int, leapfrog_steps: int, warmup_steps: int,
                                           g_l_step_size, g_llhd_sigma: float, philox, target_accept: float = 0.8, steps=None):
    """`sample_hmc_post_eps_with_flow` with a step per row, adapted during a warm-up -- the base-space twin of
    `sample_hmc_adaptive_post_z_with_flow`, whose arguments these are: the first `warmup_steps` end calls adapt the rows' steps by dual
    averaging inside `netF.reverse_hmc_step_rows` (the last of them writes the averaged step), the rest run at the frozen steps.
    With warmup_steps = 0 and a float g_l_step_size the result is `sample_hmc_post_eps_with_flow`'s, bit for bit.
    Returns (eps_k (B, nz), z_k = f^-1(eps_k) (B, nz, 1, 1), accept_rate (B) over the trajectories after the warm-up -- over all K
    when warmup_steps is 0 or K --, U(eps_k) (B), the `flow.HmcRowSteps`).  g_l_steps = 0 or an empty batch returns the input without
    a launch: (eps, None, None, None, `steps`), an empty batch with its empty z."""
    from . import flow
    K, L, W, mode = _adaptive_plan(g_l_steps, leapfrog_steps, warmup_steps, steps)
    B, nz = eps.shape[0], eps.shape[1]
    eps_prop = eps.detach().reshape(B, nz).contiguous().clone()
    if B == 0:
        return eps_prop, eps_prop.view(0, nz, 1, 1), None, None, steps
    if K < 1:
        return eps_prop, None, None, None, steps
    plan = netF._plan()
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    steps = _row_steps(flow, steps, B, eps_prop.device, g_l_step_size, target_accept)
    keeps = flow.reverse_keep_supported(plan, B)
    act = flow.new_act_saved(plan, B, eps_prop.device)
    state = flow.new_hmc_state(plan, B, eps_prop.device)
    accepted = torch.zeros(B, dtype=torch.float32, device=eps_prop.device)
    counted = K - W if W < K else K
    with torch.no_grad():
        for j in range(K * L + 1):
            if keeps:
                z, _, saved = flow.reverse(plan, eps_prop, None, save_for_backward=True, act_saved=act)
            else:
                z, _ = flow.reverse(plan, eps_prop, None)
                saved = flow.forward(plan, z, None, want_ll=False, save_for_backward=True, act_saved=act)[3]
            with torch.enable_grad():
                zr = z.view(B, nz, 1, 1).requires_grad_(True)
                energy = c * ((netG(zr) - x) ** 2).flatten(1).sum(1)                                 # train.py:312-313, per row
                grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
            t, inner = j // L, j % L != 0
            _, acc, _ = netF.reverse_hmc_step_rows(eps_prop, saved, act, grad_g, energy.detach(), state, None if inner else philox.step(t),
                                                   steps, phase="inner" if inner else "end" if j else "init", propose=j < K * L,
                                                   inplace=True, reuse_buffers=True, adapt=None if inner or not j else mode(t))
            if j and not inner and (t > W or counted == K):
                accepted += acc
        z = flow.reverse(plan, state.z, None)[0]
    philox.advance(K + 1)
    return state.z, z.view(B, nz, 1, 1), accepted / counted, state.energy, steps


def sample_hmc_metric_post_eps_with_flow(eps, x, netG: nn.Module, netF, *, g_l_steps: int, leapfrog_steps: int, warmup_steps: int,
                                         g_l_step_size, g_llhd_sigma: float, philox, target_accept: float = 0.8, steps=None, metric=None,
                                         windows=None):
    """`sample_hmc_adaptive_post_eps_with_flow` with a diagonal metric per row -- the base-space twin of
    `sample_hmc_metric_post_z_with_flow`, whose arguments these are (`netF.reverse_hmc_step_metric`): the flow whitens the prior, an
    informative likelihood leaves the posterior in eps anisotropic.  With windows=(None, []) and a fresh unit metric the result is
    `sample_hmc_adaptive_post_eps_with_flow`'s, bit for bit.
    Returns that sampler's tuple and the `flow.HmcRowMetric`: (eps_k, z_k, accept_rate, U(eps_k), steps, metric); g_l_steps = 0 or an
    empty batch returns the input without a launch, as there."""
    from . import flow
    K, L, W, mode = _adaptive_plan(g_l_steps, leapfrog_steps, warmup_steps, steps)
    window = _metric_plan(flow, metric, windows, W)
    B, nz = eps.shape[0], eps.shape[1]
    eps_prop = eps.detach().reshape(B, nz).contiguous().clone()
    if B == 0:
        return eps_prop, eps_prop.view(0, nz, 1, 1), None, None, steps, metric
    if K < 1:
        return eps_prop, None, None, None, steps, metric
    plan = netF._plan()
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    steps = _row_steps(flow, steps, B, eps_prop.device, g_l_step_size, target_accept)
    metric = flow.new_hmc_row_metric(plan, B, eps_prop.device) if metric is None else metric
    keeps = flow.reverse_keep_supported(plan, B)
    act = flow.new_act_saved(plan, B, eps_prop.device)
    state = flow.new_hmc_state(plan, B, eps_prop.device)
    accepted = torch.zeros(B, dtype=torch.float32, device=eps_prop.device)
    counted = K - W if W < K else K
    with torch.no_grad():
        for j in range(K * L + 1):
            if keeps:
                z, _, saved = flow.reverse(plan, eps_prop, None, save_for_backward=True, act_saved=act)
            else:
                z, _ = flow.reverse(plan, eps_prop, None)
                saved = flow.forward(plan, z, None, want_ll=False, save_for_backward=True, act_saved=act)[3]
            with torch.enable_grad():
                zr = z.view(B, nz, 1, 1).requires_grad_(True)
                energy = c * ((netG(zr) - x) ** 2).flatten(1).sum(1)                                 # train.py:312-313, per row
                grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
            t, inner = j // L, j % L != 0
            end = bool(j) and not inner
            _, acc, _ = netF.reverse_hmc_step_metric(eps_prop, saved, act, grad_g, energy.detach(), state, None if inner else philox.step(t),
                                                     steps, metric, phase="inner" if inner else "end" if j else "init", propose=j < K * L,
                                                     inplace=True, reuse_buffers=True, adapt=mode(t) if end else None,
                                                     window=window(t) if end else None)
            if end and (t > W or counted == K):
                accepted += acc
        z = flow.reverse(plan, state.z, None)[0]
    philox.advance(K + 1)
    return state.z, z.view(B, nz, 1, 1), accepted / counted, state.energy, steps, metric


def ais_schedule(T: int, kind: str = "sigmoid", delta: float = 4.0) -> torch.Tensor:
    """The T + 1 inverse temperatures of an annealed-importance-sampling run, float64: beta_0 = 0, beta_T = 1, nondecreasing.
    "sigmoid" is Wu et al.'s ("On the quantitative analysis of decoder-based generative models"): sigma(delta (2 t / T - 1)) rescaled
    to [0, 1], which spends its steps near both ends; "linear" is t / T."""
    T = int(T)
    if T < 1:
        raise ValueError(f"T must be >= 1 (got {T})")
    t = torch.arange(T + 1, dtype=torch.float64) / T
    if kind == "linear":
        b = t
    elif kind == "sigmoid":
        s = torch.sigmoid(float(delta) * (2.0 * t - 1.0))
        b = (s - s[0]) / (s[-1] - s[0])
    else:
        raise ValueError(f"kind must be 'sigmoid' or 'linear' (got {kind!r})")
    b = b.clone()
    b[0], b[-1] = 0.0, 1.0
    return b


def _chains_plan(flow, chains, leapfrog_steps, steps, metric):
    """(chains, L) of a run of annealed chains, checked, with its frozen steps and metric."""
    C, L = int(chains), int(leapfrog_steps)
    if L < 1:
        raise ValueError(f"leapfrog_steps must be >= 1 (got {leapfrog_steps})")
    if C < 1:
        raise ValueError(f"chains must be >= 1 (got {chains})")
    if steps is not None and not isinstance(steps, flow.HmcRowSteps):
        raise flow.LsnfError("steps must be a flow.HmcRowSteps (new_hmc_row_steps()), or None")
    if metric is not None and not isinstance(metric, flow.HmcRowMetric):
        raise flow.LsnfError("metric must be a flow.HmcRowMetric (new_hmc_row_metric()), or None")
    return C, L


def _ais_plan(flow, betas, chains, leapfrog_steps, steps, metric, adapt):
    """(betas as a float64 (T + 1) tensor, T, chains, L) of an AIS run, checked."""
    betas = torch.as_tensor(betas, dtype=torch.float64).reshape(-1).cpu()
    T = betas.numel() - 1
    C, L = _chains_plan(flow, chains, leapfrog_steps, steps, metric)
    if T >= 1 and (float(betas[0]) != 0.0 or bool((betas[1:] < betas[:-1]).any())):
        raise ValueError("betas must start at 0 (the chains start from draws of the prior) and must not decrease")
    return betas, T, C, L


def _ais_reduce(temper, N, C, D, sigma):
    """The chain reduction of an AIS run, a few float64 ops on (N, chains): log p(x), the log weights, the effective sample size."""
    import math
    log_w = temper.log_weight().view(N, C)
    lse = torch.logsumexp(log_w, dim=1)
    log_px = lse - math.log(C) - 0.5 * D * math.log(2.0 * math.pi * sigma * sigma)
    ess = torch.exp(2.0 * lse - torch.logsumexp(2.0 * log_w, dim=1))
    return log_px, log_w, ess


_AIS_DOC = """
    betas: the T + 1 inverse temperatures (`ais_schedule`), beta_0 = 0.  The B = N * chains rows are x repeated per chain (row
    n * chains + c is chain c of datum n).  The initial point is ONE `netF.sample(B, philox.step(0), return_eps=True)` launch -- exact
    draws of the prior, which is what beta_0 = 0 targets.  Then the HMC samplers' loop of `netF.*_tempered` calls: one init call with
    anneal = beta_1 (it weighs the start, log_w = -(beta_1 - beta_0) E(z_0), and begins trajectory 1 at beta_1), then per
    t = 1 .. T, L - 1 inner calls and one end call, which for t < T anneals to beta_{t+1} inside the kernel -- the weight's
    increment -(beta_{t+1} - beta_t) E(state_t), the re-tempered kept gradient -- and for t = T neither anneals nor proposes.  The call
    that begins trajectory t takes philox.step(t), the last end call philox.step(T + 1) for its uniform alone; philox.step(0) is the
    sample's and no step ever takes it (the sample's eps and a step's xi are the same function of (seed, offset, row, column): the
    first momentum would equal the starting eps).  philox is advanced by T + 1 on return: the next run's sample at that offset draws
    eps only, the last end call drew a uniform only.
    steps / metric: frozen `flow.HmcRowSteps` / `flow.HmcRowMetric`, e.g. what `sample_hmc_metric_post_*_with_flow` adapted at
    beta = 1: the posterior is the stiffest of the targets, so its step is the conservative choice for every beta (acceptance is
    higher at the smaller ones).  Default: the float (or (B) tensor) g_l_step_size and a unit metric.  adapt=True passes
    adapt="update" on every end call: the transitions then depend on the chain's past, and the estimator is only approximately
    unbiased.
    Returns (log_px (N) float64, log_w (N, chains) float64, ess (N) float64, accept_rate (B), z_T (B, nz, 1, 1), temper):
        log_px = logsumexp_c(log_w) - log(chains) - D / 2 * log(2 pi sigma^2),   D = x[0].numel()
        ess    = exp(2 logsumexp_c(log_w) - logsumexp_c(2 log_w))
    a stochastic lower bound of log p(x) whose expectation of exp is exact.  Only the likelihood's energy E = |x - G(z)|^2 / (2 sigma^2)
    enters a weight; the prior is sampled exactly and a transition is invariant under a constant in its potential, so the flow's
    own +log(2 pi) constant in ll (and the prior's whole normaliser) cancels -- the Gaussian likelihood's normaliser is the one
    constant added.  The chain reduction is a few float64 torch ops on (N, chains), the only torch arithmetic on the flow's side.
    An empty batch returns empty results and T < 1 Nones, both without a launch and without advancing philox."""


def estimate_log_px_ais_z_with_flow(x, netG: nn.Module, netF, *, betas, chains: int, leapfrog_steps: int, g_l_step_size,
                                    g_llhd_sigma: float, philox, steps=None, metric=None, adapt: bool = False):
    """log p(x) of the latent-variable model p_flow(z) N(x; G(z), sigma^2 I) by annealed importance sampling (Neal 2001) with HMC
    transitions in z (Wu et al.'s evaluation protocol), every transition two launches of the flow (`netF.hmc_step_tempered`)."""
    from . import flow
    betas, T, C, L = _ais_plan(flow, betas, chains, leapfrog_steps, steps, metric, adapt)
    N = x.shape[0]
    if T < 1:
        return None, None, None, None, None, None
    if N == 0:
        e = torch.zeros(0, dtype=torch.float64, device=x.device)
        return e, e.view(0, C), e.clone(), None, None, None
    B, D, plan = N * C, x[0].numel(), netF._plan()
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    xs = x.detach().repeat_interleave(C, dim=0)
    z0 = netF.sample(B, philox.step(0), return_eps=True)[0]
    nz = z0.shape[1]
    z_prop = z0.detach().reshape(B, nz).contiguous()
    dev = z_prop.device
    sched = betas.to(torch.float32).to(dev)[:, None].expand(T + 1, B).contiguous()
    steps = _row_steps(flow, steps, B, dev, g_l_step_size, 0.8)
    metric = flow.new_hmc_row_metric(plan, B, dev) if metric is None else metric
    temper = flow.new_hmc_row_temper(plan, B, dev, 0.0)
    state = flow.new_hmc_state(plan, B, dev)
    accepted = torch.zeros(B, dtype=torch.float32, device=dev)
    for j in range(T * L + 1):
        zr = z_prop.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = c * ((netG(zr) - xs) ** 2).flatten(1).sum(1)                                # train.py:312-313, per row
        grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
        t, inner = j // L, j % L != 0
        end = bool(j) and not inner
        _, acc, _, _ = netF.hmc_step_tempered(z_prop, grad_g, energy.detach(), state, None if inner else philox.step(t + 1), steps, metric,
                                              temper, phase="inner" if inner else "end" if j else "init", propose=j < T * L,
                                              inplace=True, reuse_buffers=True, adapt="update" if adapt and end else None,
                                              anneal=sched[t + 1] if not inner and t < T else None)
        if end:
            accepted += acc
    philox.advance(T + 1)
    log_px, log_w, ess = _ais_reduce(temper, N, C, D, float(g_llhd_sigma))
    return log_px, log_w, ess, accepted / T, state.z.view(B, nz, 1, 1), temper


def estimate_log_px_ais_eps_with_flow(x, netG: nn.Module, netF, *, betas, chains: int, leapfrog_steps: int, g_l_step_size,
                                      g_llhd_sigma: float, philox, steps=None, metric=None, adapt: bool = False):
    """`estimate_log_px_ais_z_with_flow` with the transitions in the flow's base space (`netF.reverse_hmc_step_tempered`): the chain
    runs on eps with z = f^-1(eps), the prior is N(0, I) at every temperature and the flow's side of a transition is the reverse and
    ONE more launch.  The starting eps_0 is the sample's own eps.  z_T = f^-1(eps_T)."""
    from . import flow
    betas, T, C, L = _ais_plan(flow, betas, chains, leapfrog_steps, steps, metric, adapt)
    N = x.shape[0]
    if T < 1:
        return None, None, None, None, None, None
    if N == 0:
        e = torch.zeros(0, dtype=torch.float64, device=x.device)
        return e, e.view(0, C), e.clone(), None, None, None
    B, D, plan = N * C, x[0].numel(), netF._plan()
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    xs = x.detach().repeat_interleave(C, dim=0)
    eps0 = netF.sample(B, philox.step(0), return_eps=True)[1]
    nz = eps0.shape[1]
    eps_prop = eps0.detach().reshape(B, nz).contiguous()
    dev = eps_prop.device
    sched = betas.to(torch.float32).to(dev)[:, None].expand(T + 1, B).contiguous()
    steps = _row_steps(flow, steps, B, dev, g_l_step_size, 0.8)
    metric = flow.new_hmc_row_metric(plan, B, dev) if metric is None else metric
    temper = flow.new_hmc_row_temper(plan, B, dev, 0.0)
    keeps = flow.reverse_keep_supported(plan, B)
    act = flow.new_act_saved(plan, B, dev)
    state = flow.new_hmc_state(plan, B, dev)
    accepted = torch.zeros(B, dtype=torch.float32, device=dev)
    with torch.no_grad():
        for j in range(T * L + 1):
            if keeps:
                z, _, saved = flow.reverse(plan, eps_prop, None, save_for_backward=True, act_saved=act)
            else:
                z, _ = flow.reverse(plan, eps_prop, None)
                saved = flow.forward(plan, z, None, want_ll=False, save_for_backward=True, act_saved=act)[3]
            with torch.enable_grad():
                zr = z.view(B, nz, 1, 1).requires_grad_(True)
                energy = c * ((netG(zr) - xs) ** 2).flatten(1).sum(1)                                # train.py:312-313, per row
                grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
            t, inner = j // L, j % L != 0
            end = bool(j) and not inner
            _, acc, _ = netF.reverse_hmc_step_tempered(eps_prop, saved, act, grad_g, energy.detach(), state,
                                                       None if inner else philox.step(t + 1), steps, metric, temper,
                                                       phase="inner" if inner else "end" if j else "init", propose=j < T * L,
                                                       inplace=True, reuse_buffers=True, adapt="update" if adapt and end else None,
                                                       anneal=sched[t + 1] if not inner and t < T else None)
            if end:
                accepted += acc
        z = flow.reverse(plan, state.z, None)[0]
    philox.advance(T + 1)
    log_px, log_w, ess = _ais_reduce(temper, N, C, D, float(g_llhd_sigma))
    return log_px, log_w, ess, accepted / T, z.view(B, nz, 1, 1), temper


estimate_log_px_ais_z_with_flow.__doc__ += _AIS_DOC
estimate_log_px_ais_eps_with_flow.__doc__ += _AIS_DOC


def _particles_plan(chains, particles):
    """The groups' geometry: particles is 2, 4, 8 or 16 and divides chains."""
    P = int(particles)
    if P not in (2, 4, 8, 16) or chains % P:
        raise ValueError(f"particles must be 2, 4, 8 or 16 and divide chains={chains} (got {particles})")
    return P


def _smc_plan(flow, betas, chains, particles, leapfrog_steps, steps, metric):
    """`_ais_plan`'s checks and the groups' geometry."""
    betas, T, C, L = _ais_plan(flow, betas, chains, leapfrog_steps, steps, metric, False)
    return betas, T, C, L, _particles_plan(C, particles)


_SMC_DOC = """
    The loop, the draws and the Philox offsets are `estimate_log_px_ais_*_with_flow`'s (which see for betas, steps, metric and the
    reduction); every launch is the resampling call, and the end call of every t < T carries resample=particles: after its weight
    increment and before trajectory t + 1 begins, each group of `particles` consecutive chains of a datum whose effective sample size
    is below ess_threshold * particles is resampled systematically inside the kernel (one uniform per group, Philox field 4 of the
    group's first row) and its rows continue from the group's mean weight.  More chains than particles are independent islands;
    since resampling keeps a group's mean weight, logsumexp_c(log_w) - log(chains) is still the unbiased estimate.  The init call
    weighs the prior's draws and does not resample.  The chain is frozen: there is no adapt=.
    Returns the AIS tuple plus `resampled`, (N, chains / particles) float32: at how many of the T - 1 resampling end calls each group
    resampled -- accumulated on the device from the calls' ess output, without a host synchronisation inside the loop."""


def estimate_log_px_smc_z_with_flow(x, netG: nn.Module, netF, *, betas, chains: int, particles: int, leapfrog_steps: int,
                                    g_l_step_size, g_llhd_sigma: float, philox, ess_threshold: float = 0.5, steps=None, metric=None):
    """log p(x) of the latent-variable model p_flow(z) N(x; G(z), sigma^2 I) by a sequential Monte Carlo sampler (Del Moral, Doucet &
    Jasra 2006) with HMC transitions in z: annealed importance sampling whose particles are resampled when their weights degenerate,
    every transition two launches of the flow (`netF.hmc_step_resample`)."""
    from . import flow
    betas, T, C, L, P = _smc_plan(flow, betas, chains, particles, leapfrog_steps, steps, metric)
    N = x.shape[0]
    if T < 1:
        return None, None, None, None, None, None, None
    if N == 0:
        e = torch.zeros(0, dtype=torch.float64, device=x.device)
        return e, e.view(0, C), e.clone(), None, None, None, None
    B, D, plan = N * C, x[0].numel(), netF._plan()
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    xs = x.detach().repeat_interleave(C, dim=0)
    z0 = netF.sample(B, philox.step(0), return_eps=True)[0]
    nz = z0.shape[1]
    z_prop = z0.detach().reshape(B, nz).contiguous()
    dev = z_prop.device
    sched = betas.to(torch.float32).to(dev)[:, None].expand(T + 1, B).contiguous()
    steps = _row_steps(flow, steps, B, dev, g_l_step_size, 0.8)
    metric = flow.new_hmc_row_metric(plan, B, dev) if metric is None else metric
    temper = flow.new_hmc_row_temper(plan, B, dev, 0.0)
    state = flow.new_hmc_state(plan, B, dev)
    accepted = torch.zeros(B, dtype=torch.float32, device=dev)
    resampled = torch.zeros(N, C // P, dtype=torch.float32, device=dev)
    edge = torch.tensor(float(ess_threshold), dtype=torch.float32, device=dev) * P
    for j in range(T * L + 1):
        zr = z_prop.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = c * ((netG(zr) - xs) ** 2).flatten(1).sum(1)                                # train.py:312-313, per row
        grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
        t, inner = j // L, j % L != 0
        end = bool(j) and not inner
        move = end and t < T
        _, acc, _, _, _, ess = netF.hmc_step_resample(z_prop, grad_g, energy.detach(), state, None if inner else philox.step(t + 1), steps,
                                                      metric, temper, phase="inner" if inner else "end" if j else "init",
                                                      propose=j < T * L, inplace=True, reuse_buffers=True,
                                                      anneal=sched[t + 1] if not inner and t < T else None,
                                                      resample=P if move else None, ess_threshold=ess_threshold)
        if end:
            accepted += acc
        if move:
            resampled += (ess.view(N, C // P, P)[:, :, 0] < edge).float()
    philox.advance(T + 1)
    log_px, log_w, ess = _ais_reduce(temper, N, C, D, float(g_llhd_sigma))
    return log_px, log_w, ess, accepted / T, state.z.view(B, nz, 1, 1), temper, resampled


def estimate_log_px_smc_eps_with_flow(x, netG: nn.Module, netF, *, betas, chains: int, particles: int, leapfrog_steps: int,
                                      g_l_step_size, g_llhd_sigma: float, philox, ess_threshold: float = 0.5, steps=None, metric=None):
    """`estimate_log_px_smc_z_with_flow` with the transitions in the flow's base space (`netF.reverse_hmc_step_resample`): the chain
    runs on eps with z = f^-1(eps), and the flow's side of a transition is the reverse and ONE more launch.  z_T = f^-1(eps_T)."""
    from . import flow
    betas, T, C, L, P = _smc_plan(flow, betas, chains, particles, leapfrog_steps, steps, metric)
    N = x.shape[0]
    if T < 1:
        return None, None, None, None, None, None, None
    if N == 0:
        e = torch.zeros(0, dtype=torch.float64, device=x.device)
        return e, e.view(0, C), e.clone(), None, None, None, None
    B, D, plan = N * C, x[0].numel(), netF._plan()
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    xs = x.detach().repeat_interleave(C, dim=0)
    eps0 = netF.sample(B, philox.step(0), return_eps=True)[1]
    nz = eps0.shape[1]
    eps_prop = eps0.detach().reshape(B, nz).contiguous()
    dev = eps_prop.device
    sched = betas.to(torch.float32).to(dev)[:, None].expand(T + 1, B).contiguous()
    steps = _row_steps(flow, steps, B, dev, g_l_step_size, 0.8)
    metric = flow.new_hmc_row_metric(plan, B, dev) if metric is None else metric
    temper = flow.new_hmc_row_temper(plan, B, dev, 0.0)
    keeps = flow.reverse_keep_supported(plan, B)
    act = flow.new_act_saved(plan, B, dev)
    state = flow.new_hmc_state(plan, B, dev)
    accepted = torch.zeros(B, dtype=torch.float32, device=dev)
    resampled = torch.zeros(N, C // P, dtype=torch.float32, device=dev)
    edge = torch.tensor(float(ess_threshold), dtype=torch.float32, device=dev) * P
    with torch.no_grad():
        for j in range(T * L + 1):
            if keeps:
                z, _, saved = flow.reverse(plan, eps_prop, None, save_for_backward=True, act_saved=act)
            else:
                z, _ = flow.reverse(plan, eps_prop, None)
                saved = flow.forward(plan, z, None, want_ll=False, save_for_backward=True, act_saved=act)[3]
            with torch.enable_grad():
                zr = z.view(B, nz, 1, 1).requires_grad_(True)
                energy = c * ((netG(zr) - xs) ** 2).flatten(1).sum(1)                                # train.py:312-313, per row
                grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
            t, inner = j // L, j % L != 0
            end = bool(j) and not inner
            move = end and t < T
            _, acc, _, _, ess = netF.reverse_hmc_step_resample(eps_prop, saved, act, grad_g, energy.detach(), state,
                                                               None if inner else philox.step(t + 1), steps, metric, temper,
                                                               phase="inner" if inner else "end" if j else "init", propose=j < T * L,
                                                               inplace=True, reuse_buffers=True,
                                                               anneal=sched[t + 1] if not inner and t < T else None,
                                                               resample=P if move else None, ess_threshold=ess_threshold)
            if end:
                accepted += acc
            if move:
                resampled += (ess.view(N, C // P, P)[:, :, 0] < edge).float()
        z = flow.reverse(plan, state.z, None)[0]
    philox.advance(T + 1)
    log_px, log_w, ess = _ais_reduce(temper, N, C, D, float(g_llhd_sigma))
    return log_px, log_w, ess, accepted / T, z.view(B, nz, 1, 1), temper, resampled


estimate_log_px_smc_z_with_flow.__doc__ += _SMC_DOC
estimate_log_px_smc_eps_with_flow.__doc__ += _SMC_DOC


_SMC_ADAPTIVE_DOC = """
    The loop, the draws and the Philox offsets are `estimate_log_px_smc_*_with_flow`'s with max_steps in the place of T and no
    schedule from the host: every launch is the scheduling call.  The init call and every end call t < max_steps - 1 carry
    schedule=particles with a ceiling of 1: inside the kernel each group of `particles` consecutive chains of a datum steps to the
    temperature at which the conditional effective sample size (CESS) of its incremental weights is cess_target * particles (twelve
    halvings; Zhou, Johansen & Aston 2016), by at least min_step (None: 1 / (4 max_steps)).  End calls t < max_steps carry
    resample=particles as the fixed-schedule sampler's do (ess_threshold <= 0: never -- adaptive AIS within groups).  The end call
    that anneals into the last transition carries no schedule: it goes to beta = 1 in one plain step, so a group that has not arrived
    by then still gets a valid estimate.  A group that has reached 1 goes on with plain HMC at beta = 1; its increments are zero.
    check_every = k > 0 reads beta.min() after every k-th end call and, once every group is at 1, makes the next transition the last
    one: the only host synchronisation; the default of 0 has none and runs all max_steps transitions.  philox is advanced by the
    transitions run + 1.
    The temperatures now depend on the particles, so the estimate is consistent in the number of particles but no longer exactly
    unbiased (Beskos, Jasra, Kantas & Thiery 2016); the fixed-schedule samplers stay the unbiased ones.
    Returns the SMC tuple -- the AIS six and `resampled`, (N, chains / particles) float32: at how many of its resampling end calls each
    group resampled -- plus `steps_used`, (N, chains / particles) float32: the annealing calls each group entered below beta = 1; both
    accumulated on the device; with return_schedule also `schedule`, (annealing calls, N, chains / particles) float32: every group's
    beta after every annealing call."""


def _smc_adaptive_plan(flow, max_steps, chains, particles, leapfrog_steps, steps, metric, cess_target, min_step, check_every):
    """`_smc_plan`'s checks with max_steps in the place of the schedule, and the search's scalars."""
    K = int(max_steps)
    if K < 0:
        raise ValueError(f"max_steps must not be negative (got {max_steps})")
    C, L = _chains_plan(flow, chains, leapfrog_steps, steps, metric)
    P = _particles_plan(C, particles)
    if not 0.0 < float(cess_target) < 1.0:
        raise ValueError(f"cess_target must lie in (0, 1) (got {cess_target})")
    ms = 1.0 / (4.0 * max(K, 1)) if min_step is None else float(min_step)
    if not (math.isfinite(ms) and ms >= 0.0):
        raise ValueError(f"min_step must be finite and not negative (got {min_step})")
    if int(check_every) < 0:
        raise ValueError(f"check_every must not be negative (got {check_every})")
    return K, C, L, P, ms, int(check_every)


def estimate_log_px_smc_adaptive_z_with_flow(x, netG: nn.Module, netF, *, max_steps: int, chains: int, particles: int, leapfrog_steps: int,
                                             g_l_step_size, g_llhd_sigma: float, philox, cess_target: float = 0.95,
                                             ess_threshold: float = 0.5, min_step=None, check_every: int = 0, steps=None, metric=None,
                                             return_schedule: bool = False):
    """`estimate_log_px_smc_z_with_flow` without a temperature schedule: every group's next temperature is chosen from its particles
    inside the annealing call (`netF.hmc_step_schedule`), so that data whose likelihood is sharp take many small steps and data whose
    likelihood is flat few."""
    from . import flow
    T, C, L, P, ms, every = _smc_adaptive_plan(flow, max_steps, chains, particles, leapfrog_steps, steps, metric, cess_target, min_step,
                                               check_every)
    N, extra = x.shape[0], (None,) if return_schedule else ()
    if T < 1:
        return (None,) * 8 + extra
    if N == 0:
        e = torch.zeros(0, dtype=torch.float64, device=x.device)
        return (e, e.view(0, C), e.clone(), None, None, None, None, None) + extra
    B, D, plan = N * C, x[0].numel(), netF._plan()
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    xs = x.detach().repeat_interleave(C, dim=0)
    z0 = netF.sample(B, philox.step(0), return_eps=True)[0]
    nz = z0.shape[1]
    z_prop = z0.detach().reshape(B, nz).contiguous()
    dev = z_prop.device
    ceiling = torch.ones(B, dtype=torch.float32, device=dev)
    steps = _row_steps(flow, steps, B, dev, g_l_step_size, 0.8)
    metric = flow.new_hmc_row_metric(plan, B, dev) if metric is None else metric
    temper = flow.new_hmc_row_temper(plan, B, dev, 0.0)
    state = flow.new_hmc_state(plan, B, dev)
    accepted = torch.zeros(B, dtype=torch.float32, device=dev)
    steps_used = torch.zeros(N, C // P, dtype=torch.float32, device=dev)
    resampled = torch.zeros(N, C // P, dtype=torch.float32, device=dev)
    edge = torch.tensor(float(ess_threshold), dtype=torch.float32, device=dev) * P
    trace = []
    j = 0
    while j < T * L + 1:
        zr = z_prop.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = c * ((netG(zr) - xs) ** 2).flatten(1).sum(1)                                # train.py:312-313, per row
        grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
        t, inner = j // L, j % L != 0
        end = bool(j) and not inner
        anneals = not inner and t < T
        if anneals:
            steps_used += (temper.beta.view(N, C // P, P)[:, :, 0] < 1.0).float()
        _, acc, _, _, _, ess = netF.hmc_step_schedule(z_prop, grad_g, energy.detach(), state, None if inner else philox.step(t + 1), steps,
                                                    metric, temper, phase="inner" if inner else "end" if j else "init",
                                                    propose=j < T * L, inplace=True, reuse_buffers=True,
                                                    anneal=ceiling if anneals else None, resample=P if end and t < T else None,
                                                    ess_threshold=ess_threshold, schedule=P if anneals and t < T - 1 else None,
                                                    cess_target=cess_target, min_step=ms)
        if end:
            accepted += acc
        if end and t < T:
            resampled += (ess.view(N, C // P, P)[:, :, 0] < edge).float()
        if anneals and return_schedule:
            trace.append(temper.beta.view(N, C // P, P)[:, :, 0].clone())
        if every and end and t % every == 0 and t + 1 < T and float(temper.beta.min()) >= 1.0:
            T = t + 1                                         # (every weight is final: the next transition is the last)
        j += 1
    philox.advance(T + 1)
    log_px, log_w, ess = _ais_reduce(temper, N, C, D, float(g_llhd_sigma))
    out = (log_px, log_w, ess, accepted / T, state.z.view(B, nz, 1, 1), temper, resampled, steps_used)
    return out + ((torch.stack(trace),) if return_schedule else ())


def estimate_log_px_smc_adaptive_eps_with_flow(x, netG: nn.Module, netF, *, max_steps: int, chains: int, particles: int,
                                               leapfrog_steps: int, g_l_step_size, g_llhd_sigma: float, philox, cess_target: float = 0.95,
                                               ess_threshold: float = 0.5, min_step=None, check_every: int = 0, steps=None, metric=None,
                                               return_schedule: bool = False):
    """`estimate_log_px_smc_adaptive_z_with_flow` with the transitions in the flow's base space (`netF.reverse_hmc_step_schedule`): the
    chain runs on eps with z = f^-1(eps), and the flow's side of a transition is the reverse and ONE more launch.  z_T = f^-1(eps_T)."""
    from . import flow
    T, C, L, P, ms, every = _smc_adaptive_plan(flow, max_steps, chains, particles, leapfrog_steps, steps, metric, cess_target, min_step,
                                               check_every)
    N, extra = x.shape[0], (None,) if return_schedule else ()
    if T < 1:
        return (None,) * 8 + extra
    if N == 0:
        e = torch.zeros(0, dtype=torch.float64, device=x.device)
        return (e, e.view(0, C), e.clone(), None, None, None, None, None) + extra
    B, D, plan = N * C, x[0].numel(), netF._plan()
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    xs = x.detach().repeat_interleave(C, dim=0)
    eps0 = netF.sample(B, philox.step(0), return_eps=True)[1]
    nz = eps0.shape[1]
    eps_prop = eps0.detach().reshape(B, nz).contiguous()
    dev = eps_prop.device
    ceiling = torch.ones(B, dtype=torch.float32, device=dev)
    steps = _row_steps(flow, steps, B, dev, g_l_step_size, 0.8)
    metric = flow.new_hmc_row_metric(plan, B, dev) if metric is None else metric
    temper = flow.new_hmc_row_temper(plan, B, dev, 0.0)
    keeps = flow.reverse_keep_supported(plan, B)
    act = flow.new_act_saved(plan, B, dev)
    state = flow.new_hmc_state(plan, B, dev)
    accepted = torch.zeros(B, dtype=torch.float32, device=dev)
    steps_used = torch.zeros(N, C // P, dtype=torch.float32, device=dev)
    resampled = torch.zeros(N, C // P, dtype=torch.float32, device=dev)
    edge = torch.tensor(float(ess_threshold), dtype=torch.float32, device=dev) * P
    trace = []
    with torch.no_grad():
        j = 0
        while j < T * L + 1:
            if keeps:
                z, _, saved = flow.reverse(plan, eps_prop, None, save_for_backward=True, act_saved=act)
            else:
                z, _ = flow.reverse(plan, eps_prop, None)
                saved = flow.forward(plan, z, None, want_ll=False, save_for_backward=True, act_saved=act)[3]
            with torch.enable_grad():
                zr = z.view(B, nz, 1, 1).requires_grad_(True)
                energy = c * ((netG(zr) - xs) ** 2).flatten(1).sum(1)                                # train.py:312-313, per row
                grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
            t, inner = j // L, j % L != 0
            end = bool(j) and not inner
            anneals = not inner and t < T
            if anneals:
                steps_used += (temper.beta.view(N, C // P, P)[:, :, 0] < 1.0).float()
            _, acc, _, _, ess = netF.reverse_hmc_step_schedule(eps_prop, saved, act, grad_g, energy.detach(), state,
                                                             None if inner else philox.step(t + 1), steps, metric, temper,
                                                             phase="inner" if inner else "end" if j else "init", propose=j < T * L,
                                                             inplace=True, reuse_buffers=True, anneal=ceiling if anneals else None,
                                                             resample=P if end and t < T else None, ess_threshold=ess_threshold,
                                                             schedule=P if anneals and t < T - 1 else None, cess_target=cess_target,
                                                             min_step=ms)
            if end:
                accepted += acc
            if end and t < T:
                resampled += (ess.view(N, C // P, P)[:, :, 0] < edge).float()
            if anneals and return_schedule:
                trace.append(temper.beta.view(N, C // P, P)[:, :, 0].clone())
            if every and end and t % every == 0 and t + 1 < T and float(temper.beta.min()) >= 1.0:
                T = t + 1                                     # (every weight is final: the next transition is the last)
            j += 1
        z = flow.reverse(plan, state.z, None)[0]
    philox.advance(T + 1)
    log_px, log_w, ess = _ais_reduce(temper, N, C, D, float(g_llhd_sigma))
    out = (log_px, log_w, ess, accepted / T, z.view(B, nz, 1, 1), temper, resampled, steps_used)
    return out + ((torch.stack(trace),) if return_schedule else ())


estimate_log_px_smc_adaptive_z_with_flow.__doc__ += _SMC_ADAPTIVE_DOC
estimate_log_px_smc_adaptive_eps_with_flow.__doc__ += _SMC_ADAPTIVE_DOC


def pt_ladder(R: int, beta_min: float) -> torch.Tensor:
    """The R inverse temperatures of a parallel-tempering ladder, float64, increasing: rung 0 is exactly beta_min, rung R - 1 exactly
    1.0 (the posterior), geometric in between -- beta_r = beta_min^((R - 1 - r) / (R - 1)), the spacing that equalises the swap rates
    of a Gaussian target.  beta_min = 0.0 is allowed and means the prior: rung 0 is then 0.0 and rungs 1 .. R - 1 halve downwards from
    1.0 (beta_r = 2^(r - (R - 1))), since no geometric ladder reaches 0.  R is 2, 4, 8 or 16 (`flow.hmc_step_exchange`'s ladder)."""
    R, beta_min = int(R), float(beta_min)
    if R not in (2, 4, 8, 16):
        raise ValueError(f"R must be 2, 4, 8 or 16 (got {R})")
    if not 0.0 <= beta_min < 1.0:
        raise ValueError(f"beta_min must lie in [0, 1) (got {beta_min})")
    r = torch.arange(R, dtype=torch.float64)
    if beta_min == 0.0:
        b = torch.pow(torch.tensor(2.0, dtype=torch.float64), r - (R - 1))
    else:
        b = torch.pow(torch.tensor(beta_min, dtype=torch.float64), (R - 1 - r) / (R - 1))
    b[0], b[-1] = beta_min, 1.0
    return b


def _pt_plan(flow, betas, g_l_steps, leapfrog_steps, swap_every, steps, metric):
    """(betas as a float64 (R) tensor, R, K, L, swap(t) -> None | "even" | "odd" of end call t = 1 .. K) of a parallel-tempering run,
    checked.  Every swap_every-th end call swaps, the swapping calls alternate even, odd."""
    betas = torch.as_tensor(betas, dtype=torch.float64).reshape(-1).cpu()
    R, K, L, E = betas.numel(), int(g_l_steps), int(leapfrog_steps), int(swap_every)
    if R not in (2, 4, 8, 16):
        raise ValueError(f"betas must hold 2, 4, 8 or 16 temperatures (got {R})")
    if L < 1:
        raise ValueError(f"leapfrog_steps must be >= 1 (got {leapfrog_steps})")
    if E < 1:
        raise ValueError(f"swap_every must be >= 1 (got {swap_every})")
    if steps is not None and not isinstance(steps, flow.HmcRowSteps):
        raise flow.LsnfError("steps must be a flow.HmcRowSteps (new_hmc_row_steps()), or None")
    if metric is not None and not isinstance(metric, flow.HmcRowMetric):
        raise flow.LsnfError("metric must be a flow.HmcRowMetric (new_hmc_row_metric()), or None")

    def swap(t):
        return None if t % E else ("even", "odd")[(t // E - 1) % 2]
    return betas, R, K, L, swap


def _pt_swap_rate(sums, calls, N, R):
    """swap_rate (N, R - 1) of a parallel-tempering run: the mean of `swapped` over the calls that paired rungs (r, r + 1) -- those of
    parity r % 2 --, read at the pair's lower row; 0 for a pair no call tried."""
    rate = torch.zeros((N, R - 1), dtype=torch.float32, device=sums["even"].device)
    for p, name in enumerate(("even", "odd")):
        if calls[name]:
            rate[:, p::2] = sums[name].view(N, R)[:, p:R - 1:2] / calls[name]
    return rate


_PT_DOC = """
    betas: the R inverse temperatures of one ladder (`pt_ladder`), R in {2, 4, 8, 16}.  The B = N * R rows are the start and x repeated
    per rung: row n * R + r is rung r of datum n, at betas[r] for the whole run.  The call schedule is the HMC samplers': one init
    call, then per t = 1 .. K (g_l_steps) L - 1 inner calls and one end call (`netF.*_exchange`).  Every swap_every-th end call
    swaps -- t = swap_every, 2 swap_every, .. -- with the parity alternating even, odd from the first of them; the exchange happens
    inside that call's kernel, after its decision and before the trajectory it begins.  The init call takes philox.step(0) (the first
    momentum), end call t philox.step(t): its uniform, the next momentum and, if it swaps, the pairs' uniforms (counter field 3) all
    come from that one offset.  philox is advanced by K + 1 on return.
    steps / metric: frozen `flow.HmcRowSteps` / `flow.HmcRowMetric` of B rows (nothing adapts here: swapping during a warm-up is not
    built).  Default: the float (or (B) tensor) g_l_step_size and a unit metric.
    Returns (z_k of rung R - 1 -- where `pt_ladder` puts beta = 1 -- (N, nz, 1, 1), accept_rate (B) of the trajectories, swap_rate
    (N, R - 1) per adjacent pair (the mean of `swapped` over the calls that tried the pair), U of the kept states (B), the
    `flow.HmcState`, the `flow.HmcRowTemper`).  Per trajectory the flow's side runs no torch op beside the two tallies of (B) floats.
    g_l_steps = 0 or an empty batch returns (the start (N, nz, 1, 1), None, None, None, None, None) without a launch."""


def sample_hmc_pt_post_z_with_flow(z, x, netG: nn.Module, netF, *, betas, g_l_steps: int, leapfrog_steps: int, g_l_step_size,
                                   g_llhd_sigma: float, philox, swap_every: int = 1, steps=None, metric=None):
    """Parallel tempering (replica exchange) of HMC chains in z on p_flow(z) p(x | G(z))^beta: R replicas per datum at the
    temperatures `betas`, the hot ones crossing between the modes a posterior of an ambiguous x has, the swap fused into the end
    call's kernel (`netF.hmc_step_exchange`)."""
    from . import flow
    betas, R, K, L, swap = _pt_plan(flow, betas, g_l_steps, leapfrog_steps, swap_every, steps, metric)
    N, nz = z.shape[0], z.shape[1]
    if K < 1 or N == 0:
        return z.detach().clone().view(N, nz, 1, 1), None, None, None, None, None
    B, plan = N * R, netF._plan()
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    xs = x.detach().repeat_interleave(R, dim=0)
    z_prop = z.detach().reshape(N, nz).repeat_interleave(R, dim=0).contiguous()
    dev = z_prop.device
    steps = _row_steps(flow, steps, B, dev, g_l_step_size, 0.8)
    metric = flow.new_hmc_row_metric(plan, B, dev) if metric is None else metric
    temper = flow.new_hmc_row_temper(plan, B, dev, betas.to(torch.float32).repeat(N))
    state = flow.new_hmc_state(plan, B, dev)
    accepted = torch.zeros(B, dtype=torch.float32, device=dev)
    sums = {"even": torch.zeros(B, dtype=torch.float32, device=dev), "odd": torch.zeros(B, dtype=torch.float32, device=dev)}
    calls = {"even": 0, "odd": 0}
    for j in range(K * L + 1):
        zr = z_prop.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = c * ((netG(zr) - xs) ** 2).flatten(1).sum(1)                                # train.py:312-313, per row
        grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
        t, inner = j // L, j % L != 0
        end = bool(j) and not inner
        parity = swap(t) if end else None
        _, acc, _, _, swapped, _ = netF.hmc_step_exchange(z_prop, grad_g, energy.detach(), state, None if inner else philox.step(t), steps,
                                                          metric, temper, phase="inner" if inner else "end" if j else "init",
                                                          propose=j < K * L, inplace=True, reuse_buffers=True, swap=parity, ladder=R)
        if end:
            accepted += acc
        if parity:
            sums[parity] += swapped
            calls[parity] += 1
    philox.advance(K + 1)
    z_k = state.z.view(N, R, nz)[:, R - 1].contiguous().view(N, nz, 1, 1)
    return z_k, accepted / K, _pt_swap_rate(sums, calls, N, R), state.energy, state, temper


def sample_hmc_pt_post_eps_with_flow(eps, x, netG: nn.Module, netF, *, betas, g_l_steps: int, leapfrog_steps: int, g_l_step_size,
                                     g_llhd_sigma: float, philox, swap_every: int = 1, steps=None, metric=None):
    """`sample_hmc_pt_post_z_with_flow` with the chains in the flow's base space (`netF.reverse_hmc_step_exchange`): they run on eps
    with z = f^-1(eps), the prior is N(0, I) at every temperature and the flow's side of a leapfrog step is the reverse and ONE more
    launch.  The start is eps (N, nz); state.z holds the replicas' eps_k; the first result is z_k = f^-1(eps_k) of rung R - 1."""
    from . import flow
    betas, R, K, L, swap = _pt_plan(flow, betas, g_l_steps, leapfrog_steps, swap_every, steps, metric)
    N, nz = eps.shape[0], eps.shape[1]
    if K < 1 or N == 0:
        return eps.detach().clone().view(N, nz, 1, 1), None, None, None, None, None
    B, plan = N * R, netF._plan()
    c = 1.0 / (2.0 * g_llhd_sigma * g_llhd_sigma)
    xs = x.detach().repeat_interleave(R, dim=0)
    eps_prop = eps.detach().reshape(N, nz).repeat_interleave(R, dim=0).contiguous()
    dev = eps_prop.device
    steps = _row_steps(flow, steps, B, dev, g_l_step_size, 0.8)
    metric = flow.new_hmc_row_metric(plan, B, dev) if metric is None else metric
    temper = flow.new_hmc_row_temper(plan, B, dev, betas.to(torch.float32).repeat(N))
    keeps = flow.reverse_keep_supported(plan, B)
    act = flow.new_act_saved(plan, B, dev)
    state = flow.new_hmc_state(plan, B, dev)
    accepted = torch.zeros(B, dtype=torch.float32, device=dev)
    sums = {"even": torch.zeros(B, dtype=torch.float32, device=dev), "odd": torch.zeros(B, dtype=torch.float32, device=dev)}
    calls = {"even": 0, "odd": 0}
    with torch.no_grad():
        for j in range(K * L + 1):
            if keeps:
                z, _, saved = flow.reverse(plan, eps_prop, None, save_for_backward=True, act_saved=act)
            else:
                z, _ = flow.reverse(plan, eps_prop, None)
                saved = flow.forward(plan, z, None, want_ll=False, save_for_backward=True, act_saved=act)[3]
            with torch.enable_grad():
                zr = z.view(B, nz, 1, 1).requires_grad_(True)
                energy = c * ((netG(zr) - xs) ** 2).flatten(1).sum(1)                                # train.py:312-313, per row
                grad_g = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()        # train.py:314
            t, inner = j // L, j % L != 0
            end = bool(j) and not inner
            parity = swap(t) if end else None
            _, acc, _, swapped, _ = netF.reverse_hmc_step_exchange(eps_prop, saved, act, grad_g, energy.detach(), state,
                                                                   None if inner else philox.step(t), steps, metric, temper,
                                                                   phase="inner" if inner else "end" if j else "init",
                                                                   propose=j < K * L, inplace=True, reuse_buffers=True, swap=parity,
                                                                   ladder=R)
            if end:
                accepted += acc
            if parity:
                sums[parity] += swapped
                calls[parity] += 1
        z = flow.reverse(plan, state.z.view(N, R, nz)[:, R - 1].contiguous(), None)[0]
    philox.advance(K + 1)
    return z.view(N, nz, 1, 1), accepted / K, _pt_swap_rate(sums, calls, N, R), state.energy, state, temper


sample_hmc_pt_post_z_with_flow.__doc__ += _PT_DOC
sample_hmc_pt_post_eps_with_flow.__doc__ += _PT_DOC


def flow_mle_step(netF, optF, z_g_k, f_max_norm: Optional[float] = None, fused: bool = False):
    """train.py:404-415: one Adam step of the flow on the Langevin-inferred z.  Returns loss_f (detached).
    fused=False restates the reference line by line (autograd through `netF(...)`); fused=True computes the same
    loss and gradients with `netF.mle_grads` (no autograd graph, no element-wise torch launches); with a `FlowAdam` as optF it
    runs `netF.mle_step`: the clip and the update on the device too.  With `netF.deterministic_grads = True` every form takes
    its parameter gradients from the fixed-order contraction (`lsnf_backward_params_det`): bit-reproducible from run to run."""
    import numpy as np
    from .optim import FlowAdam
    if fused and isinstance(optF, FlowAdam):       # clip + Adam on the device, the plan left current (netF.mle_step)
        if f_max_norm is not None and optF.param_groups[0]["max_norm"] != f_max_norm:
            raise flow.LsnfError(f"flow_mle_step: the FlowAdam owns the clip (max_norm={optF.param_groups[0]['max_norm']}); "
                            f"f_max_norm={f_max_norm} disagrees with it")
        return netF.mle_step(z_g_k.reshape(z_g_k.shape[0], -1), optF)
    if fused:
        optF.zero_grad(set_to_none=True)
        loss_f = netF.mle_grads(z_g_k.reshape(z_g_k.shape[0], -1), max_norm=f_max_norm,    # clip: train.py:413-414
                                reuse_buffers=True)
        optF.step()
        return loss_f
    optF.zero_grad()
    z2d = torch.squeeze(z_g_k)
    z1, logdet, _ = netF(z2d, objective=torch.zeros(int(z_g_k.shape[0]), device=z2d.device), init=False)
    prior_ll = -0.5 * (z1 ** 2)
    prior_ll = prior_ll.flatten(1).sum(-1) + np.log(2 * np.pi)
    ll = prior_ll + logdet
    loss_f = -ll.mean()
    loss_f.backward()
    if f_max_norm is not None:
        torch.nn.utils.clip_grad_norm_(netF.parameters(), f_max_norm)                        # train.py:413-414
    optF.step()
    return loss_f.detach()


def sample_x(netG: nn.Module, netF, n: int, philox, temperature: float = 1.0):
    """train.py:472-478 (`sample_x` of the FID evaluation; also :428-437): n images from the prior.  The latent draw and the
    flow's reverse pass are one launch (`netF.sample`: no `torch.randn`, no zeros tensor); the generator runs on the result as
    in the reference.  `philox` is a `flow.PhiloxNoise` (its `row0` = the shard's first global row when the n_fid_samples are
    split over GPUs: the union of the shards is then the one-GPU draw); it is ADVANCED by one on return, as the K-step sampler
    above advances it by K.  Returns netG's output, detached (range mapping and the copy to the host stay with the caller)."""
    with torch.no_grad():
        z_f_k = netF.sample(n, philox, temperature=temperature)                              # train.py:473-475
        x_samples = netG(torch.reshape(z_f_k, (z_f_k.shape[0], z_f_k.shape[1], 1, 1)))       # train.py:476
    if hasattr(philox, "advance"):        # (an int seed has no state to advance)
        philox.advance(1)
    return x_samples.detach()


class GraphedLangevinSampler:
    """The K-step sampler above with ONE step captured in a HIP graph and replayed K times (train.py:311-329).

    At the reference's batch size (B = 100) a Langevin step is ~20 small launches (generator forward + input
    gradient through MIOpen, the flow's two kernels) and the host cannot issue them as fast as the GPU retires
    them; a graph replay issues the whole step with one call.  The step works on static buffers (z is updated in
    place by the fused flow update), the Langevin noise is drawn inside the update kernel from a device-side
    counter that the graph itself advances (`PhiloxNoise(offset_dev=)`), and the flow's prepared weights live in a
    buffer that `netF._plan()` refreshes in place -- so optimizer steps between `run()` calls need no re-capture.

        sampler = GraphedLangevinSampler(netG, netF, B, nz, x_shape, g_l_step_size=0.1, g_llhd_sigma=0.3, seed=1)
        z_k, gg_norm, gf_norm, f = sampler.run(z0, x, g_l_steps=20, offset=it * 20)
    """

    def __init__(self, netG: nn.Module, netF, B: int, nz: int, x_shape, *, g_l_step_size: float, g_llhd_sigma: float,
                 g_l_with_noise: bool = True, seed: int = 0, row0: int = 0, device=None, warmup: int = 3):
        from . import flow
        dev = device or next(netF.parameters()).device
        self.netG, self.netF, self.B, self.nz = netG, netF, B, nz
        self.z = torch.zeros(B, nz, 1, 1, device=dev)
        self.x = torch.zeros(tuple(x_shape), device=dev)
        self.ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        self.noise = flow.PhiloxNoise(seed, 0, row0, offset_dev=self.ctr) if g_l_with_noise else None
        self.s, self.sigma = float(g_l_step_size), float(g_llhd_sigma)
        self.mse = nn.MSELoss(reduction="sum")
        netF._plan()                                   # prepared weights exist before anything is captured
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                  # warm-up off the capture stream (MIOpen finds its solvers here)
            for _ in range(warmup):
                self._step()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.f_log_lkhd, self.gg_norm, self.gf_norm = self._step()

    def _step(self):
        zr = self.z.detach().requires_grad_(True)
        g_log_lkhd = 1.0 / (2.0 * self.sigma * self.sigma) * self.mse(self.netG(zr), self.x)         # train.py:312-313
        z_grad_g = torch.autograd.grad(g_log_lkhd, zr)[0]                                            # train.py:314
        _, ll, gf, gg = self.netF.langevin_step(self.z.view(self.B, self.nz), z_grad_g.reshape(self.B, self.nz),
                                                self.noise, self.s, inplace=True)                    # :316-326, in place
        self.ctr.add_(1)                                                                             # next step's noise
        return -ll.sum(), gg.mean(), gf.mean()

    def run(self, z0: torch.Tensor, x: torch.Tensor, g_l_steps: int, offset: int = 0):
        """Returns (z_k (B,nz,1,1), mean |z_grad_g|, mean |z_grad_f|, f_log_lkhd of the last step's input)."""
        self.z.copy_(z0.reshape(self.z.shape))
        self.x.copy_(x)
        self.ctr.fill_(int(offset))
        self.netF._plan()                              # re-derives the prepared weights in place if a parameter changed
        for _ in range(g_l_steps):
            self.graph.replay()
        return self.z.detach().clone(), self.gg_norm, self.gf_norm, self.f_log_lkhd


class GraphedEpsLangevinSampler:
    """`sample_langevin_post_eps_with_flow(..., fused=True)` with ONE step captured in a HIP graph and replayed K times: the
    stash-keeping reverse, the generator's forward and input gradient, and `flow.reverse_langevin_step` in place on static buffers
    (eps, z, the block outputs, the stash), the noise drawn inside the update kernel from a device-side counter that the graph
    itself advances (`PhiloxNoise(offset_dev=)`).  The host then issues one call per step, as `GraphedLangevinSampler` does for the
    z-space sampler; the results are the eager fused sampler's with `philox = PhiloxNoise(seed, offset, row0)`, bit for bit.
    Only where `flow.reverse_keep_supported(plan, B)` (the reverse must keep the stash itself); `LsnfError` otherwise.

        sampler = GraphedEpsLangevinSampler(netG, netF, B, nz, x_shape, g_l_step_size=0.1, g_llhd_sigma=0.3, seed=1)
        eps_k, z_k, gg_norm, gf_norm = sampler.run(eps0, x, g_l_steps=20, offset=it * 20)
    """

    def __init__(self, netG: nn.Module, netF, B: int, nz: int, x_shape, *, g_l_step_size: float, g_llhd_sigma: float,
                 noise: bool = True, seed: int = 0, row0: int = 0, device=None, warmup: int = 3):
        from . import flow
        dev = device or next(netF.parameters()).device
        plan = netF._plan()                            # prepared weights exist before anything is captured
        if B < 1 or not flow.reverse_keep_supported(plan, B):
            raise flow.LsnfError(f"GraphedEpsLangevinSampler needs the stash-keeping reverse (flow.reverse_keep_supported) for B={B}: "
                                 "a bf16x3-family math mode and B within the small-batch threshold")
        self.netG, self.netF, self.B, self.nz = netG, netF, B, nz
        f32 = dict(dtype=torch.float32, device=dev)
        self.eps = torch.zeros(B, nz, **f32)
        self.z, self.obj = torch.zeros(B, nz, **f32), torch.zeros(B, **f32)
        self.saved = torch.zeros(max(plan.depth - 1, 1), B, nz, **f32)
        self.act = flow.new_act_saved(plan, B, dev)
        self.g_norm, self.eps_norm = torch.zeros(B, **f32), torch.zeros(B, **f32)
        self.x = torch.zeros(tuple(x_shape), device=dev)
        self.ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        self.noise = flow.PhiloxNoise(seed, 0, row0, offset_dev=self.ctr) if noise else None
        self.s, self.sigma = float(g_l_step_size), float(g_llhd_sigma)
        self.mse = nn.MSELoss(reduction="sum")
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                  # warm-up off the capture stream (MIOpen finds its solvers here)
            for _ in range(warmup):
                self._step()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.gg_norm, self.gf_norm = self._step()

    def _step(self):
        from . import flow
        plan = self.netF._plan()
        with torch.no_grad():
            flow.reverse(plan, self.eps, None, out=(self.z, self.obj), act_saved=self.act, z_saved_out=self.saved)
        zr = self.z.view(self.B, self.nz, 1, 1).detach().requires_grad_(True)
        g_log_lkhd = 1.0 / (2.0 * self.sigma * self.sigma) * self.mse(self.netG(zr), self.x)         # train.py:312-313
        grad_g = torch.autograd.grad(g_log_lkhd, zr)[0].reshape(self.B, self.nz).contiguous()        # train.py:314
        with torch.no_grad():
            flow.reverse_langevin_step(plan, self.eps, self.saved if plan.depth > 1 else None, self.act, grad_g, self.noise,
                                       self.s, inplace=True, out=(None, None, self.g_norm, self.eps_norm))
            self.ctr.add_(1)                                                                         # next step's noise
            return self.g_norm.mean(), self.eps_norm.mean()

    def run(self, eps0: torch.Tensor, x: torch.Tensor, g_l_steps: int, offset: int = 0):
        """Returns (eps_k (B, nz), z_k = f^-1(eps_k) (B, nz, 1, 1), mean |g_eps|, mean |eps|) -- the norms of the last step's input,
        None if g_l_steps = 0 -- as `sample_langevin_post_eps_with_flow(..., fused=True)`."""
        from . import flow
        self.eps.copy_(eps0.reshape(self.eps.shape))
        self.x.copy_(x)
        self.ctr.fill_(int(offset))
        plan = self.netF._plan()                       # re-derives the prepared weights in place if a parameter changed
        for _ in range(g_l_steps):
            self.graph.replay()
        eps = self.eps.detach().clone()
        z = flow.reverse(plan, eps, None)[0]
        if g_l_steps < 1:
            return eps, z.view(self.B, self.nz, 1, 1), None, None
        return eps, z.view(self.B, self.nz, 1, 1), self.gg_norm.clone(), self.gf_norm.clone()

"""Markov-chain extensions of the functional host API (C: include/lsnf_flow_mcmc.h), re-exported by flow.py -- use them as
`flow.mala_step`, `flow.reverse_mala_step`, `flow.MalaState`, `flow.new_mala_state`, `flow.hmc_step`, `flow.reverse_hmc_step`,
`flow.HmcState`, `flow.new_hmc_state`, `flow.hmc_step_rows`, `flow.reverse_hmc_step_rows`, `flow.HmcRowSteps`,
`flow.new_hmc_row_steps`, `flow.hmc_step_metric`, `flow.reverse_hmc_step_metric`, `flow.HmcRowMetric`, `flow.new_hmc_row_metric`,
`flow.hmc_step_tempered`, `flow.reverse_hmc_step_tempered`, `flow.HmcRowTemper`, `flow.new_hmc_row_temper`,
`flow.hmc_step_exchange`, `flow.reverse_hmc_step_exchange`, `flow.hmc_step_resample`, `flow.reverse_hmc_step_resample`,
`flow.hmc_step_schedule`, `flow.reverse_hmc_step_schedule`.
Every tensor goes through flow.py's one checking path before anything is launched; like there, all functions raise on CPU tensors:
there is no CPU path."""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Optional

import ctypes
import math

import torch

from ._lib import LsnfDualAvg, LsnfError, LsnfMetricReg
from .flow import (FlowPlan, PhiloxNoise, _anchor, _call, _check_in, _check_like, _check_out, _check_stash, _noise_args, _plan_head,  # noqa: F401
                   _ptr, _stream_buffers, forward, new_act_saved)


MALA_INIT = 1                 # include/lsnf_flow_mcmc.h LSNF_MALA_INIT


@dataclass
class MalaState:
    """The kept state of a Metropolis-adjusted chain (`mala_step`): z (B, nz) the accepted points, grad (B, nz) = grad U(z),
    energy (B) = U(z), with U = energy_g - ll.  Written by an init=True call, updated in place by every later one.
    For the base-space chain of `reverse_mala_step` the same three arrays hold its state: z = the accepted points eps,
    grad = grad U(eps) = eps + J_{f^-1}(eps)^T grad_g, energy = U(eps) = |eps|^2 / 2 + energy_g."""
    z: torch.Tensor
    grad: torch.Tensor
    energy: torch.Tensor


def new_mala_state(plan: FlowPlan, B: int, device) -> MalaState:
    """A zeroed chain state of B rows for `mala_step` (the init=True call fills it)."""
    f32 = dict(dtype=torch.float32, device=device)
    return MalaState(torch.zeros((int(B), plan.nz), **f32), torch.zeros((int(B), plan.nz), **f32), torch.zeros(int(B), **f32))


def _check_chain(plan, point, name, grad_g, energy_g, state, state_cls, noise, uniform, stash=None):
    """The argument checks every chain step makes, in the order a bad argument is reported: the point (the anchor of the call; `name`
    in the messages), the caller's stash (z_saved, act_saved) where the step takes one, grad_g, energy_g, the state (a `state_cls`,
    every array of it), the noise and the uniform.  Returns (B, device, noise tensor or None, rng or None)."""
    B, dev = _anchor(point, name, plan), point.device
    if stash is not None:
        _check_stash(plan, B, dev, *stash, True)
    _check_like(grad_g, "grad_g", point, name)
    _check_in(energy_g, "energy_g", B, dev)
    if not isinstance(state, state_cls):
        raise LsnfError(f"state must be a flow.{state_cls.__name__} ({_NEW_STATE[state_cls]}())")
    for f in fields(state_cls):          # (B, nz) arrays, but for the per-row scalars energy / kin
        _check_out(getattr(state, f.name), "state." + f.name, B if f.name in ("energy", "kin") else B * plan.nz, dev)
    noise, rng = _noise_args(noise, point, name, dev)
    _check_in(uniform, "uniform", B, dev)
    if rng is not None and uniform is not None:
        raise LsnfError("pass either a PhiloxNoise or the tensors (noise, uniform=), not both")
    return B, dev, noise, rng


def _forward_at(plan, z_prop, B, dev, key, reuse_buffers):
    """The first launch of `mala_step` / `hmc_step`: their buffer set (on the plan under `key` with reuse_buffers) and the forward at
    z_prop into it.  Returns (buffers, z1, ll)."""
    def make():
        f32 = dict(dtype=torch.float32, device=dev)
        return {"act": new_act_saved(plan, B, dev), "out": (torch.empty_like(z_prop), torch.empty(B, **f32), torch.empty(B, **f32)),
                "saved": torch.empty((plan.depth - 1, B, plan.nz), **f32) if plan.depth > 1 else None,
                "acc": torch.empty(B, **f32), "la": torch.empty(B, **f32)}
    bufs = _stream_buffers(plan, key, B, dev, make) if reuse_buffers else make()
    _check_stash(plan, B, dev, bufs["saved"], bufs["act"], True)
    z1, _, ll, _ = forward(plan, z_prop, None, want_ll=True, out=bufs["out"], act_saved=bufs["act"], z_saved_out=bufs["saved"])
    return bufs, z1, ll


def mala_step(plan: FlowPlan, z_prop: torch.Tensor, grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor],
              state: MalaState, noise, step_size: float, *, init: bool = False, uniform: Optional[torch.Tensor] = None,
              propose: bool = True, inplace: bool = False, reuse_buffers: bool = False):
    """One Metropolis-adjusted Langevin call (include/lsnf_flow_mcmc.h `lsnf_mala_step`) in two launches: the forward at the
    proposal `z_prop` (ll, block outputs, stash) and the backward whose output section DECIDES z_prop against `state` -- target
    p(z) ~ exp(-U), U = energy_g - ll -- updates the state in place and, with propose, writes the next proposal
    z_next = z_state - 0.5 s^2 grad_state + s * xi.  grad_g (B, nz) / energy_g (B): the caller's gradient and per-row energy at
    z_prop (None = 0).  init=True starts a chain at z_prop: every row accepted, the state written without being read.
    `noise`: a `PhiloxNoise` (the uniform and xi are drawn inside the kernel: xi is `langevin_step`'s draw at the same offset, the
    uniform a stream of its own), or a (B, nz) tensor of N(0,1) draws together with uniform= (B) draws in (0, 1) -- the tensor is
    left out (None) with propose=False, the uniform may be with init=True.  K proposals are K + 1 calls: init, K - 1 deciding and
    proposing calls, one with propose=False.
    Returns (z_next or None, accepted (B) of 1.0 / 0.0, log_alpha (B), ll_prop (B)).  inplace: z_next is z_prop itself.
    reuse_buffers: as `langevin_step`'s -- the last three are then overwritten by the next call."""
    B, dev, noise, rng = _check_chain(plan, z_prop, "z_prop", grad_g, energy_g, state, MalaState, noise, uniform)
    bufs, z1, ll = _forward_at(plan, z_prop, B, dev, "_mala_buffers", reuse_buffers)
    z_next = None if not propose else z_prop if inplace else torch.empty_like(z_prop)
    _call("lsnf_mala_step", dev, *_plan_head(plan), B, _ptr(z_prop), _ptr(z1), _ptr(bufs["saved"]), _ptr(bufs["act"]), _ptr(ll), _ptr(grad_g),
          _ptr(energy_g), _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(noise), _ptr(uniform), rng, float(step_size),
          MALA_INIT if init else 0, _ptr(z_next), _ptr(bufs["acc"]), _ptr(bufs["la"]))
    return z_next, bufs["acc"], bufs["la"], ll


def reverse_mala_step(plan: FlowPlan, eps_prop: torch.Tensor, z_saved: Optional[torch.Tensor], act_saved: torch.Tensor,
                      grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor], state: MalaState, noise, step_size: float, *,
                      init: bool = False, uniform: Optional[torch.Tensor] = None, propose: bool = True, inplace: bool = False,
                      reuse_buffers: bool = False):
    """One Metropolis-adjusted Langevin call in the flow's base space (include/lsnf_flow_mcmc.h `lsnf_reverse_mala_step`) in ONE
    launch: with x = reverse(eps_prop)[0], target pi(eps) ~ exp(-U), U = |eps|^2 / 2 + energy_g, grad U = eps + g,
    g = J_{f^-1}(eps)^T grad_g (`reverse_backward_z(plan, eps_prop, z_saved, act_saved, grad_g)`'s bits).  The reverse-backward's output
    section DECIDES eps_prop against `state` (z = eps, grad = eps + g, energy = U), updates the state in place and, with propose,
    writes the next proposal eps_next = fma(s, xi, fma(-0.5 s^2, grad_state, eps_state)) (`reverse_langevin_step`'s arithmetic).
    eps_prop / z_saved / act_saved: the reverse's input, the block outputs and the stash of the forward AT x -- kept by
    `reverse(plan, eps_prop, save_for_backward=True, act_saved=...)`, or from `forward(plan, x, ...)`.  Unlike `mala_step` this
    call runs no flow pass itself: the caller's generator sits between the reverse and it, as with `reverse_langevin_step`.
    grad_g (B, nz) / energy_g (B): the caller's gradient and per-row energy at x (None = 0: the chain samples N(0, I)).
    init=True starts a chain at eps_prop: every row accepted, the state written without being read.  `noise`: a `PhiloxNoise`
    (the uniform and xi are drawn inside the kernel: xi is `reverse_langevin_step`'s draw at the same offset, the uniform
    `mala_step`'s), or a (B, nz) tensor of N(0,1) draws together with uniform= (B) draws in (0, 1) -- the tensor is left out (None)
    with propose=False, the uniform may be with init=True.  K proposals are K + 1 calls: init, K - 1 deciding and proposing calls,
    one with propose=False.
    Returns (eps_next or None, accepted (B) of 1.0 / 0.0, log_alpha (B)).  inplace: eps_next is eps_prop itself.  reuse_buffers:
    the last two live on the plan and are overwritten by the next call.  Asynchronous on the current stream; nothing but the
    launch, so it can be captured in a graph."""
    B, dev, noise, rng = _check_chain(plan, eps_prop, "eps_prop", grad_g, energy_g, state, MalaState, noise, uniform,
                                      stash=(z_saved, act_saved))

    def make():
        f32 = dict(dtype=torch.float32, device=dev)
        return {"acc": torch.empty(B, **f32), "la": torch.empty(B, **f32)}
    bufs = _stream_buffers(plan, "_rmala_buffers", B, dev, make) if reuse_buffers else make()
    eps_next = None if not propose else eps_prop if inplace else torch.empty_like(eps_prop)
    _call("lsnf_reverse_mala_step", dev, *_plan_head(plan), B, _ptr(eps_prop), _ptr(z_saved), _ptr(act_saved), _ptr(grad_g),
          _ptr(energy_g), _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(noise), _ptr(uniform), rng, float(step_size),
          MALA_INIT if init else 0, _ptr(eps_next), _ptr(bufs["acc"]), _ptr(bufs["la"]))
    return eps_next, bufs["acc"], bufs["la"]


HMC_INIT, HMC_INNER = 1, 2    # include/lsnf_flow_mcmc.h LSNF_HMC_INIT, LSNF_HMC_INNER
_HMC_PHASES = {"init": HMC_INIT, "inner": HMC_INNER, "end": 0}


@dataclass
class HmcState:
    """The kept state of a Hamiltonian Monte Carlo chain (`hmc_step`): `MalaState`'s z (B, nz), grad (B, nz) = grad U(z) and
    energy (B) = U(z), plus mom (B, nz), the momentum of the running trajectory (read and written by every call), and kin (B),
    the kinetic energy 0.5 |xi|^2 that trajectory began with.
    For the base-space chain of `reverse_hmc_step` the same five arrays hold its state, as `MalaState` does for `reverse_mala_step`:
    z = the accepted points eps, grad = grad U(eps) = eps + J_{f^-1}(eps)^T grad_g, energy = U(eps) = |eps|^2 / 2 + energy_g."""
    z: torch.Tensor
    grad: torch.Tensor
    energy: torch.Tensor
    mom: torch.Tensor
    kin: torch.Tensor


def new_hmc_state(plan: FlowPlan, B: int, device) -> HmcState:
    """A zeroed chain state of B rows for `hmc_step` / `reverse_hmc_step` (the phase="init" call fills it)."""
    f32 = dict(dtype=torch.float32, device=device)
    rows, one = (lambda: torch.zeros((int(B), plan.nz), **f32)), (lambda: torch.zeros(int(B), **f32))
    return HmcState(rows(), rows(), one(), rows(), one())


_NEW_STATE = {MalaState: "new_mala_state", HmcState: "new_hmc_state"}      # (named where a step is given another state)


def hmc_step(plan: FlowPlan, z_prop: torch.Tensor, grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor],
             state: HmcState, noise, step_size: float, *, phase: str = "end", uniform: Optional[torch.Tensor] = None,
             propose: bool = True, inplace: bool = False, reuse_buffers: bool = False):
    """One call of Hamiltonian Monte Carlo in z (include/lsnf_flow_mcmc.h `lsnf_hmc_step`) in two launches: the forward at the
    point `z_prop` of a trajectory (ll, block outputs, stash) and the backward whose output section is the leapfrog tail -- target
    p(z) ~ exp(-U), U = energy_g - ll, momentum ~ N(0, I), step s.  grad_g (B, nz) / energy_g (B): the caller's gradient and per-row
    energy at z_prop (None = 0).  phase:
      "init"   starts a chain at z_prop (every row accepted, the state written without being read) and begins the first trajectory:
               mom = xi - s/2 grad, z_next = z + s mom, kin = |xi|^2 / 2;
      "inner"  a leapfrog step inside a trajectory: mom -= s grad U(z_prop), z_next = z_prop + s mom.  It draws and decides nothing:
               noise and uniform must be None, propose True; state.z / grad / energy / kin are not touched;
      "end"    finishes the trajectory at z_prop (mom -= s/2 grad U), decides it against `state` with
               log_alpha = (U_state - U_prop) + (kin - |mom|^2 / 2), updates the state in place and, with propose, begins the next
               trajectory from it; with propose=False the full-step momentum at z_prop is left in state.mom.
    `noise`: a `PhiloxNoise` (the uniform and xi are drawn inside the kernel, as `mala_step`'s), or a (B, nz) tensor of N(0,1) draws
    together with uniform= (B) draws in (0, 1) -- the tensor is left out (None) with propose=False, the uniform may be with "init".
    K trajectories of L leapfrog steps are K L + 1 calls: "init", then K times (L - 1 "inner", one "end"), the last with
    propose=False.  Returns (z_next or None, accepted (B) of 1.0 / 0.0, log_alpha (B), ll_prop (B)); accepted and log_alpha are None
    for an inner call.  inplace: z_next is z_prop itself.  reuse_buffers: as `mala_step`'s."""
    if phase not in _HMC_PHASES:
        raise LsnfError(f"phase must be one of 'init', 'inner', 'end' (got {phase!r})")
    inner = phase == "inner"
    B, dev, noise, rng = _check_chain(plan, z_prop, "z_prop", grad_g, energy_g, state, HmcState, noise, uniform)
    if inner and (noise is not None or rng is not None or uniform is not None or not propose):
        raise LsnfError("an inner leapfrog step draws and decides nothing: noise and uniform must be None, propose True")
    bufs, z1, ll = _forward_at(plan, z_prop, B, dev, "_hmc_buffers", reuse_buffers)
    z_next = None if not propose else z_prop if inplace else torch.empty_like(z_prop)
    acc, la = (None, None) if inner else (bufs["acc"], bufs["la"])
    _call("lsnf_hmc_step", dev, *_plan_head(plan), B, _ptr(z_prop), _ptr(z1), _ptr(bufs["saved"]), _ptr(bufs["act"]), _ptr(ll), _ptr(grad_g),
          _ptr(energy_g), _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(state.mom), _ptr(state.kin), _ptr(noise),
          _ptr(uniform), rng, float(step_size), _HMC_PHASES[phase], _ptr(z_next), _ptr(acc), _ptr(la))
    return z_next, acc, la, ll


def reverse_hmc_step(plan: FlowPlan, eps_prop: torch.Tensor, z_saved: Optional[torch.Tensor], act_saved: torch.Tensor,
                     grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor], state: HmcState, noise, step_size: float, *,
                     phase: str = "end", uniform: Optional[torch.Tensor] = None, propose: bool = True, inplace: bool = False,
                     reuse_buffers: bool = False):
    """One call of Hamiltonian Monte Carlo in the flow's base space (include/lsnf_flow_mcmc.h `lsnf_reverse_hmc_step`) in ONE launch:
    with x = reverse(eps_prop)[0], target pi(eps) ~ exp(-U), U = |eps|^2 / 2 + energy_g, grad U = eps + g, g = J_{f^-1}(eps)^T grad_g
    (`reverse_backward_z(plan, eps_prop, z_saved, act_saved, grad_g)`'s bits), momentum ~ N(0, I) -- the flow has whitened the prior,
    so for the prior alone the identity mass matrix is the right one (else: `reverse_hmc_step_metric`) --, step s.  The reverse-backward's output section is the leapfrog tail at the point
    eps_prop of a trajectory.  eps_prop / z_saved / act_saved: the reverse's input, the block outputs and the stash of the forward
    AT x, as `reverse_mala_step`'s; like it this call runs no flow pass itself (the caller's generator sits between the reverse and
    it) and can be captured in a graph.  grad_g (B, nz) / energy_g (B): the caller's gradient and per-row energy at x (None = 0: the
    chain samples N(0, I)).  `state`: an `HmcState` (z = eps, grad = eps + g, energy = U, mom, kin).  phase:
      "init"   starts a chain at eps_prop (every row accepted, the state written without being read: `reverse_mala_step(init=True)`'s
               bits) and begins the first trajectory: mom = xi - s/2 grad, eps_next = eps + s mom, kin = |xi|^2 / 2;
      "inner"  a leapfrog step inside a trajectory: mom -= s grad U(eps_prop), eps_next = eps_prop + s mom.  It draws and decides
               nothing: noise and uniform must be None, propose True; state.z / grad / energy / kin are not touched;
      "end"    finishes the trajectory at eps_prop (mom -= s/2 grad U), decides it against `state` with
               log_alpha = (U_state - U_prop) + (kin - |mom|^2 / 2), updates the state in place and, with propose, begins the next
               trajectory from it; with propose=False the full-step momentum at eps_prop is left in state.mom.
    `noise`: a `PhiloxNoise` (the uniform and xi are drawn inside the kernel, as `reverse_mala_step`'s), or a (B, nz) tensor of N(0,1)
    draws together with uniform= (B) draws in (0, 1) -- the tensor is left out (None) with propose=False, the uniform may be with
    "init".  K trajectories of L leapfrog steps are K L + 1 calls: "init", then K times (L - 1 "inner", one "end"), the last with
    propose=False; L = 1 is `reverse_mala_step`'s chain in exact arithmetic.
    Returns (eps_next or None, accepted (B) of 1.0 / 0.0, log_alpha (B)); accepted and log_alpha are None for an inner call.
    inplace: eps_next is eps_prop itself.  reuse_buffers: the last two live on the plan and are overwritten by the next call."""
    if phase not in _HMC_PHASES:
        raise LsnfError(f"phase must be one of 'init', 'inner', 'end' (got {phase!r})")
    inner = phase == "inner"
    B, dev, noise, rng = _check_chain(plan, eps_prop, "eps_prop", grad_g, energy_g, state, HmcState, noise, uniform,
                                      stash=(z_saved, act_saved))
    if inner and (noise is not None or rng is not None or uniform is not None or not propose):
        raise LsnfError("an inner leapfrog step draws and decides nothing: noise and uniform must be None, propose True")
    acc = la = None
    if not inner:
        def make():
            f32 = dict(dtype=torch.float32, device=dev)
            return {"acc": torch.empty(B, **f32), "la": torch.empty(B, **f32)}
        bufs = _stream_buffers(plan, "_rhmc_buffers", B, dev, make) if reuse_buffers else make()
        acc, la = bufs["acc"], bufs["la"]
    eps_next = None if not propose else eps_prop if inplace else torch.empty_like(eps_prop)
    _call("lsnf_reverse_hmc_step", dev, *_plan_head(plan), B, _ptr(eps_prop), _ptr(z_saved), _ptr(act_saved), _ptr(grad_g), _ptr(energy_g),
          _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(state.mom), _ptr(state.kin), _ptr(noise), _ptr(uniform), rng,
          float(step_size), _HMC_PHASES[phase], _ptr(eps_next), _ptr(acc), _ptr(la))
    return eps_next, acc, la


HMC_ADAPT, HMC_ADAPT_LAST = 4, 8      # include/lsnf_flow_mcmc.h LSNF_HMC_ADAPT, LSNF_HMC_ADAPT_LAST
_HMC_ADAPT = {None: 0, "update": HMC_ADAPT, "last": HMC_ADAPT | HMC_ADAPT_LAST}


@dataclass
class HmcRowSteps:
    """The step of every row of a Hamiltonian Monte Carlo chain (`hmc_step_rows`, `reverse_hmc_step_rows`) and the state of its
    adaptation: step (B), read by every call and written only by an adapting end call; adapt (B, 4) = {log_step_bar, hbar, count,
    mu} per row, the dual-averaging state (Hoffman & Gelman 2014; mu = log(10 * the first step), set by `new_hmc_row_steps`); and
    the update's constants (include/lsnf_flow_mcmc.h `LsnfDualAvg`)."""
    step: torch.Tensor
    adapt: torch.Tensor
    target_accept: float = 0.8
    gamma: float = 0.05
    t0: float = 10.0
    kappa: float = 0.75
    step_min: float = 1e-4
    step_max: float = 1e2


def new_hmc_row_steps(B: int, device, step_size, target_accept: float = 0.8, gamma: float = 0.05, t0: float = 10.0, kappa: float = 0.75,
                      step_min: float = 1e-4, step_max: float = 1e2) -> HmcRowSteps:
    """The steps of B rows, all `step_size` (a float) or row b's `step_size[b]` (a (B) tensor), with a fresh adaptation state:
    count = hbar = log_step_bar = 0, mu = log(10 * step) in fp32."""
    B = int(B)
    if isinstance(step_size, torch.Tensor):
        if step_size.numel() != B:
            raise LsnfError(f"step_size has {step_size.numel()} elements, the chain {B} rows")
        step = step_size.detach().to(device=device, dtype=torch.float32).reshape(B).contiguous().clone()
    else:
        step = torch.full((B,), float(step_size), dtype=torch.float32, device=device)
    adapt = torch.zeros((B, 4), dtype=torch.float32, device=device)
    adapt[:, 3] = torch.log(10.0 * step)
    return HmcRowSteps(step, adapt, float(target_accept), float(gamma), float(t0), float(kappa), float(step_min), float(step_max))


def _row_step_mode(steps, phase, adapt):
    """What the per-row calls check before `_check_chain`, tensors apart: `steps` is an `HmcRowSteps`, the phase and the adaptation
    mode are known ones, and the mode goes with an end call.  Returns the call's flags."""
    if phase not in _HMC_PHASES:
        raise LsnfError(f"phase must be one of 'init', 'inner', 'end' (got {phase!r})")
    if not isinstance(steps, HmcRowSteps):
        raise LsnfError("steps must be a flow.HmcRowSteps (new_hmc_row_steps())")
    if adapt not in _HMC_ADAPT:
        raise LsnfError(f"adapt must be None, 'update' or 'last' (got {adapt!r})")
    if adapt is not None and phase != "end":
        raise LsnfError("the steps adapt on the decision of an end call: adapt goes with phase='end'")
    return _HMC_PHASES[phase] | _HMC_ADAPT[adapt]


def _row_step_args(steps, B, dev, adapt):
    """After `_check_chain`: the two arrays of `steps` through the one checking path (B steps, B quads, on the call's device).
    Returns the three arguments of the C call: step_rows, adapt (None unless adapting), the LsnfDualAvg (likewise)."""
    _check_out(steps.step, "steps.step", B, dev)
    _check_out(steps.adapt, "steps.adapt", 4 * B, dev)
    if adapt is None:
        return _ptr(steps.step), None, None
    da = LsnfDualAvg(steps.target_accept, steps.gamma, steps.t0, steps.kappa, steps.step_min, steps.step_max)
    return _ptr(steps.step), _ptr(steps.adapt), ctypes.byref(da)


def hmc_step_rows(plan: FlowPlan, z_prop: torch.Tensor, grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor],
                  state: HmcState, noise, steps: HmcRowSteps, *, phase: str = "end", uniform: Optional[torch.Tensor] = None,
                  propose: bool = True, inplace: bool = False, reuse_buffers: bool = False, adapt: Optional[str] = None):
    """`hmc_step` with a step per row (include/lsnf_flow_mcmc.h `lsnf_hmc_step_rows`): row b runs at steps.step[b] and, without
    adapt, gets the bits of `hmc_step` at that scalar in every phase.  adapt (end calls only): "update" finishes and decides the
    trajectory at the old step, then -- inside the kernel, per row, from its own log_alpha -- updates steps.adapt by dual averaging
    toward steps.target_accept and writes the new step, with which the next trajectory begins (propose); "last" writes the
    averaged step exp(log_step_bar) instead: the call that ends a warm-up, after which the chain is exact.  Everything else, and
    what is returned, is `hmc_step`'s."""
    flags, inner = _row_step_mode(steps, phase, adapt), phase == "inner"
    B, dev, noise, rng = _check_chain(plan, z_prop, "z_prop", grad_g, energy_g, state, HmcState, noise, uniform)
    step_ptr, adapt_ptr, da = _row_step_args(steps, B, dev, adapt)
    if inner and (noise is not None or rng is not None or uniform is not None or not propose):
        raise LsnfError("an inner leapfrog step draws and decides nothing: noise and uniform must be None, propose True")
    bufs, z1, ll = _forward_at(plan, z_prop, B, dev, "_hmc_buffers", reuse_buffers)
    z_next = None if not propose else z_prop if inplace else torch.empty_like(z_prop)
    acc, la = (None, None) if inner else (bufs["acc"], bufs["la"])
    _call("lsnf_hmc_step_rows", dev, *_plan_head(plan), B, _ptr(z_prop), _ptr(z1), _ptr(bufs["saved"]), _ptr(bufs["act"]), _ptr(ll),
          _ptr(grad_g), _ptr(energy_g), _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(state.mom), _ptr(state.kin), _ptr(noise),
          _ptr(uniform), rng, step_ptr, adapt_ptr, da, flags, _ptr(z_next), _ptr(acc), _ptr(la))
    return z_next, acc, la, ll


def reverse_hmc_step_rows(plan: FlowPlan, eps_prop: torch.Tensor, z_saved: Optional[torch.Tensor], act_saved: torch.Tensor,
                          grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor], state: HmcState, noise, steps: HmcRowSteps, *,
                          phase: str = "end", uniform: Optional[torch.Tensor] = None, propose: bool = True, inplace: bool = False,
                          reuse_buffers: bool = False, adapt: Optional[str] = None):
    """`reverse_hmc_step` with a step per row (include/lsnf_flow_mcmc.h `lsnf_reverse_hmc_step_rows`): row b runs at steps.step[b]
    and, without adapt, gets the bits of `reverse_hmc_step` at that scalar in every phase.  adapt: as `hmc_step_rows`'s -- "update"
    / "last" on an end call adapt the rows' steps by dual averaging inside the kernel, after the decision at the old step and
    before the next trajectory begins.  ONE launch and nothing else, so an adaptive chain can be captured in a graph.  Everything
    else, and what is returned, is `reverse_hmc_step`'s."""
    flags, inner = _row_step_mode(steps, phase, adapt), phase == "inner"
    B, dev, noise, rng = _check_chain(plan, eps_prop, "eps_prop", grad_g, energy_g, state, HmcState, noise, uniform,
                                      stash=(z_saved, act_saved))
    step_ptr, adapt_ptr, da = _row_step_args(steps, B, dev, adapt)
    if inner and (noise is not None or rng is not None or uniform is not None or not propose):
        raise LsnfError("an inner leapfrog step draws and decides nothing: noise and uniform must be None, propose True")
    acc = la = None
    if not inner:
        def make():
            f32 = dict(dtype=torch.float32, device=dev)
            return {"acc": torch.empty(B, **f32), "la": torch.empty(B, **f32)}
        bufs = _stream_buffers(plan, "_rhmc_buffers", B, dev, make) if reuse_buffers else make()
        acc, la = bufs["acc"], bufs["la"]
    eps_next = None if not propose else eps_prop if inplace else torch.empty_like(eps_prop)
    _call("lsnf_reverse_hmc_step_rows", dev, *_plan_head(plan), B, _ptr(eps_prop), _ptr(z_saved), _ptr(act_saved), _ptr(grad_g),
          _ptr(energy_g), _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(state.mom), _ptr(state.kin), _ptr(noise), _ptr(uniform),
          rng, step_ptr, adapt_ptr, da, flags, _ptr(eps_next), _ptr(acc), _ptr(la))
    return eps_next, acc, la


HMC_METRIC_FOLD, HMC_METRIC_CLOSE = 16, 32      # include/lsnf_flow_mcmc.h LSNF_HMC_METRIC_FOLD, LSNF_HMC_METRIC_CLOSE
_HMC_WINDOW = {None: 0, "fold": HMC_METRIC_FOLD, "close": HMC_METRIC_FOLD | HMC_METRIC_CLOSE}


@dataclass
class HmcRowMetric:
    """The diagonal metric of every row of a Hamiltonian Monte Carlo chain (`hmc_step_metric`, `reverse_hmc_step_metric`): scale
    (B, nz), the square root of the diagonal inverse mass (a standard deviation per column), read by every call and written only by
    a closing end call; mean (B, nz), m2 (B, nz) and count (B), the Welford accumulators of the running warm-up window; and the
    close's constants (include/lsnf_flow_mcmc.h `LsnfMetricReg`; n0 and var0 are Stan's)."""
    scale: torch.Tensor
    mean: torch.Tensor
    m2: torch.Tensor
    count: torch.Tensor
    n0: float = 5.0
    var0: float = 1e-3
    scale_min: float = 1e-3
    scale_max: float = 1e3


def new_hmc_row_metric(plan: FlowPlan, B: int, device, scale=1.0) -> HmcRowMetric:
    """The metric of B rows: every scale `scale` (a float) or row b's columns `scale[b]` (a (B, nz) tensor), with an empty window."""
    B = int(B)
    f32 = dict(dtype=torch.float32, device=device)
    if isinstance(scale, torch.Tensor):
        if scale.numel() != B * plan.nz:
            raise LsnfError(f"scale has {scale.numel()} elements, the chain {B} rows of {plan.nz}")
        sd = scale.detach().to(**f32).reshape(B, plan.nz).contiguous().clone()
    else:
        sd = torch.full((B, plan.nz), float(scale), **f32)
    return HmcRowMetric(sd, torch.zeros((B, plan.nz), **f32), torch.zeros((B, plan.nz), **f32), torch.zeros(B, **f32))


def _row_metric_mode(metric, phase, window):
    """What the metric calls check before `_check_chain`, beside `_row_step_mode`: `metric` is an `HmcRowMetric`, the window mode is
    a known one and goes with an end call.  Returns the window's flags."""
    if not isinstance(metric, HmcRowMetric):
        raise LsnfError("metric must be a flow.HmcRowMetric (new_hmc_row_metric())")
    if window not in _HMC_WINDOW:
        raise LsnfError(f"window must be None, 'fold' or 'close' (got {window!r})")
    if window is not None and phase != "end":
        raise LsnfError("a window folds the state an end call decided: window goes with phase='end'")
    return _HMC_WINDOW[window]


def _row_metric_args(plan, metric, B, dev, window):
    """After `_check_chain`: the four arrays of `metric` through the one checking path.  Returns the five arguments of the C call:
    scale_rows, then mean_rows, m2_rows, count_rows and the LsnfMetricReg (None unless folding)."""
    _check_out(metric.scale, "metric.scale", B * plan.nz, dev)
    _check_out(metric.mean, "metric.mean", B * plan.nz, dev)
    _check_out(metric.m2, "metric.m2", B * plan.nz, dev)
    _check_out(metric.count, "metric.count", B, dev)
    if window is None:
        return _ptr(metric.scale), None, None, None, None
    reg = LsnfMetricReg(metric.n0, metric.var0, metric.scale_min, metric.scale_max)
    return _ptr(metric.scale), _ptr(metric.mean), _ptr(metric.m2), _ptr(metric.count), ctypes.byref(reg)


def hmc_step_metric(plan: FlowPlan, z_prop: torch.Tensor, grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor],
                    state: HmcState, noise, steps: HmcRowSteps, metric: HmcRowMetric, *, phase: str = "end",
                    uniform: Optional[torch.Tensor] = None, propose: bool = True, inplace: bool = False, reuse_buffers: bool = False,
                    adapt: Optional[str] = None, window: Optional[str] = None):
    """`hmc_step_rows` with a diagonal metric per row (include/lsnf_flow_mcmc.h `lsnf_hmc_step_metric`): HMC with identity mass in
    y = z / metric.scale, i.e. mom -= s (scale * grad), z += s (scale * mom); with a unit scale a row gets the bits of
    `hmc_step_rows`.  window (end calls only): "fold" folds the state after the decision into metric.mean / m2 / count; "close"
    does that, then writes the window's regularised standard deviation to metric.scale, zeroes the accumulators, begins the next
    trajectory with the new scale and -- with adapt="update" -- restarts the dual averaging at mu = log(10 * the new step).
    Everything else, and what is returned, is `hmc_step_rows`'s."""
    flags, inner = _row_step_mode(steps, phase, adapt), phase == "inner"
    flags |= _row_metric_mode(metric, phase, window)
    B, dev, noise, rng = _check_chain(plan, z_prop, "z_prop", grad_g, energy_g, state, HmcState, noise, uniform)
    step_ptr, adapt_ptr, da = _row_step_args(steps, B, dev, adapt)
    metric_args = _row_metric_args(plan, metric, B, dev, window)
    if inner and (noise is not None or rng is not None or uniform is not None or not propose):
        raise LsnfError("an inner leapfrog step draws and decides nothing: noise and uniform must be None, propose True")
    bufs, z1, ll = _forward_at(plan, z_prop, B, dev, "_hmc_buffers", reuse_buffers)
    z_next = None if not propose else z_prop if inplace else torch.empty_like(z_prop)
    acc, la = (None, None) if inner else (bufs["acc"], bufs["la"])
    _call("lsnf_hmc_step_metric", dev, *_plan_head(plan), B, _ptr(z_prop), _ptr(z1), _ptr(bufs["saved"]), _ptr(bufs["act"]), _ptr(ll),
          _ptr(grad_g), _ptr(energy_g), _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(state.mom), _ptr(state.kin), _ptr(noise),
          _ptr(uniform), rng, step_ptr, adapt_ptr, da, *metric_args, flags, _ptr(z_next), _ptr(acc), _ptr(la))
    return z_next, acc, la, ll


def reverse_hmc_step_metric(plan: FlowPlan, eps_prop: torch.Tensor, z_saved: Optional[torch.Tensor], act_saved: torch.Tensor,
                            grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor], state: HmcState, noise, steps: HmcRowSteps,
                            metric: HmcRowMetric, *, phase: str = "end", uniform: Optional[torch.Tensor] = None, propose: bool = True,
                            inplace: bool = False, reuse_buffers: bool = False, adapt: Optional[str] = None, window: Optional[str] = None):
    """`reverse_hmc_step_rows` with a diagonal metric per row (include/lsnf_flow_mcmc.h `lsnf_reverse_hmc_step_metric`): the flow
    whitens the prior, not the posterior, so an informative likelihood leaves eps as anisotropic as z.  metric and window: as
    `hmc_step_metric`'s.  ONE launch and nothing else, so a chain that adapts and folds can be captured in a graph.  Everything else,
    and what is returned, is `reverse_hmc_step_rows`'s."""
    flags, inner = _row_step_mode(steps, phase, adapt), phase == "inner"
    flags |= _row_metric_mode(metric, phase, window)
    B, dev, noise, rng = _check_chain(plan, eps_prop, "eps_prop", grad_g, energy_g, state, HmcState, noise, uniform,
                                      stash=(z_saved, act_saved))
    step_ptr, adapt_ptr, da = _row_step_args(steps, B, dev, adapt)
    metric_args = _row_metric_args(plan, metric, B, dev, window)
    if inner and (noise is not None or rng is not None or uniform is not None or not propose):
        raise LsnfError("an inner leapfrog step draws and decides nothing: noise and uniform must be None, propose True")
    acc = la = None
    if not inner:
        def make():
            f32 = dict(dtype=torch.float32, device=dev)
            return {"acc": torch.empty(B, **f32), "la": torch.empty(B, **f32)}
        bufs = _stream_buffers(plan, "_rhmc_buffers", B, dev, make) if reuse_buffers else make()
        acc, la = bufs["acc"], bufs["la"]
    eps_next = None if not propose else eps_prop if inplace else torch.empty_like(eps_prop)
    _call("lsnf_reverse_hmc_step_metric", dev, *_plan_head(plan), B, _ptr(eps_prop), _ptr(z_saved), _ptr(act_saved), _ptr(grad_g),
          _ptr(energy_g), _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(state.mom), _ptr(state.kin), _ptr(noise), _ptr(uniform),
          rng, step_ptr, adapt_ptr, da, *metric_args, flags, _ptr(eps_next), _ptr(acc), _ptr(la))
    return eps_next, acc, la


HMC_ANNEAL = 64               # include/lsnf_flow_mcmc.h LSNF_HMC_ANNEAL


@dataclass
class HmcRowTemper:
    """The likelihood temperature of every row of a Hamiltonian Monte Carlo chain (`hmc_step_tempered`, `reverse_hmc_step_tempered`):
    beta (B), read by every call and written only by an annealing one; like_grad (B, nz) and like_energy (B), the likelihood's part
    of the kept state's gradient and potential (written wherever state.z is), from which the kept state is re-tempered when beta
    changes; and log_w (B, 2), the Kahan pair {sum, compensation} of the row's log importance weight."""
    beta: torch.Tensor
    like_grad: torch.Tensor
    like_energy: torch.Tensor
    log_w: torch.Tensor

    def log_weight(self) -> torch.Tensor:
        """The rows' log importance weights, (B) float64: log_w[:, 0] - log_w[:, 1]."""
        return self.log_w[:, 0].double() - self.log_w[:, 1].double()


def new_hmc_row_temper(plan: FlowPlan, B: int, device, beta=0.0) -> HmcRowTemper:
    """The temperatures of B rows: every one `beta` (a float) or row b's `beta[b]` (a (B) tensor); the other arrays start as zeros."""
    B = int(B)
    f32 = dict(dtype=torch.float32, device=device)
    if isinstance(beta, torch.Tensor):
        if beta.numel() != B:
            raise LsnfError(f"beta has {beta.numel()} elements, the chain {B} rows")
        bt = beta.detach().to(**f32).reshape(B).contiguous().clone()
    else:
        bt = torch.full((B,), float(beta), **f32)
    return HmcRowTemper(bt, torch.zeros((B, plan.nz), **f32), torch.zeros(B, **f32), torch.zeros((B, 2), **f32))


def _row_temper_mode(temper, phase, anneal):
    """What the tempered calls check before `_check_chain`, beside `_row_metric_mode`: `temper` is an `HmcRowTemper`, and an
    annealing call is an init or an end call.  Returns the anneal's flag."""
    if not isinstance(temper, HmcRowTemper):
        raise LsnfError("temper must be a flow.HmcRowTemper (new_hmc_row_temper())")
    if anneal is not None and not isinstance(anneal, torch.Tensor):
        raise LsnfError("anneal must be None or a (B) float32 tensor of the rows' next beta")
    if anneal is not None and phase == "inner":
        raise LsnfError("the temperature changes between two trajectories: anneal goes with phase='init' or 'end'")
    return 0 if anneal is None else HMC_ANNEAL


def _row_temper_args(plan, temper, B, dev, anneal):
    """After `_check_chain`: the arrays of `temper` and the next temperatures through the one checking path, in the order the C call
    names them.  Returns its five arguments: beta_rows, beta_next, like_grad_acc, like_u_acc, log_w (the second and the last None
    unless annealing)."""
    _check_out(temper.beta, "temper.beta", B, dev)
    _check_in(anneal, "anneal", B, dev)
    _check_out(temper.like_grad, "temper.like_grad", B * plan.nz, dev)
    _check_out(temper.like_energy, "temper.like_energy", B, dev)
    _check_out(temper.log_w, "temper.log_w", 2 * B, dev)
    if anneal is None:
        return _ptr(temper.beta), None, _ptr(temper.like_grad), _ptr(temper.like_energy), None
    return _ptr(temper.beta), _ptr(anneal), _ptr(temper.like_grad), _ptr(temper.like_energy), _ptr(temper.log_w)


def hmc_step_tempered(plan: FlowPlan, z_prop: torch.Tensor, grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor],
                      state: HmcState, noise, steps: HmcRowSteps, metric: HmcRowMetric, temper: HmcRowTemper, *, phase: str = "end",
                      uniform: Optional[torch.Tensor] = None, propose: bool = True, inplace: bool = False, reuse_buffers: bool = False,
                      adapt: Optional[str] = None, window: Optional[str] = None, anneal: Optional[torch.Tensor] = None):
    """`hmc_step_metric` with a likelihood temperature per row (include/lsnf_flow_mcmc.h `lsnf_hmc_step_tempered`): row b's target is
    p_flow(z) exp(-temper.beta[b] energy_g), i.e. grad_g and energy_g enter with the weight beta[b], the prior's part with 1; with
    beta == 1 a row gets the bits of `hmc_step_metric`.  temper.like_grad / like_energy keep grad_g / energy_g of the kept state.
    anneal (phase "init" or "end"): a (B) float32 tensor of the rows' next beta.  After the decision (and the adapt / window) the
    kernel adds -(anneal - beta) * like_energy of the state after the decision to temper.log_w (a compensated sum), re-tempers
    state.grad / state.energy of EVERY row to the next beta, writes temper.beta = anneal and begins the next trajectory (propose)
    from the re-tempered gradient: one transition of annealed importance sampling, without a torch op.  Everything else, and what is
    returned, is `hmc_step_metric`'s."""
    flags, inner = _row_step_mode(steps, phase, adapt), phase == "inner"
    flags |= _row_metric_mode(metric, phase, window)
    flags |= _row_temper_mode(temper, phase, anneal)
    B, dev, noise, rng = _check_chain(plan, z_prop, "z_prop", grad_g, energy_g, state, HmcState, noise, uniform)
    step_ptr, adapt_ptr, da = _row_step_args(steps, B, dev, adapt)
    metric_args = _row_metric_args(plan, metric, B, dev, window)
    temper_args = _row_temper_args(plan, temper, B, dev, anneal)
    if inner and (noise is not None or rng is not None or uniform is not None or not propose):
        raise LsnfError("an inner leapfrog step draws and decides nothing: noise and uniform must be None, propose True")
    bufs, z1, ll = _forward_at(plan, z_prop, B, dev, "_hmc_buffers", reuse_buffers)
    z_next = None if not propose else z_prop if inplace else torch.empty_like(z_prop)
    acc, la = (None, None) if inner else (bufs["acc"], bufs["la"])
    _call("lsnf_hmc_step_tempered", dev, *_plan_head(plan), B, _ptr(z_prop), _ptr(z1), _ptr(bufs["saved"]), _ptr(bufs["act"]), _ptr(ll),
          _ptr(grad_g), _ptr(energy_g), _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(state.mom), _ptr(state.kin), _ptr(noise),
          _ptr(uniform), rng, step_ptr, adapt_ptr, da, *metric_args, *temper_args, flags, _ptr(z_next), _ptr(acc), _ptr(la))
    return z_next, acc, la, ll


def reverse_hmc_step_tempered(plan: FlowPlan, eps_prop: torch.Tensor, z_saved: Optional[torch.Tensor], act_saved: torch.Tensor,
                              grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor], state: HmcState, noise, steps: HmcRowSteps,
                              metric: HmcRowMetric, temper: HmcRowTemper, *, phase: str = "end", uniform: Optional[torch.Tensor] = None,
                              propose: bool = True, inplace: bool = False, reuse_buffers: bool = False, adapt: Optional[str] = None,
                              window: Optional[str] = None, anneal: Optional[torch.Tensor] = None):
    """`reverse_hmc_step_metric` with a likelihood temperature per row (include/lsnf_flow_mcmc.h `lsnf_reverse_hmc_step_tempered`):
    row b's target is N(eps; 0, I) exp(-temper.beta[b] energy_g); temper.like_grad keeps the kernel's own J_{f^-1}(eps)^T grad_g of the
    kept state, unscaled.  temper and anneal: as `hmc_step_tempered`'s.  ONE launch and nothing else, so an annealed chain can be
    captured in a graph.  Everything else, and what is returned, is `reverse_hmc_step_metric`'s."""
    flags, inner = _row_step_mode(steps, phase, adapt), phase == "inner"
    flags |= _row_metric_mode(metric, phase, window)
    flags |= _row_temper_mode(temper, phase, anneal)
    B, dev, noise, rng = _check_chain(plan, eps_prop, "eps_prop", grad_g, energy_g, state, HmcState, noise, uniform,
                                      stash=(z_saved, act_saved))
    step_ptr, adapt_ptr, da = _row_step_args(steps, B, dev, adapt)
    metric_args = _row_metric_args(plan, metric, B, dev, window)
    temper_args = _row_temper_args(plan, temper, B, dev, anneal)
    if inner and (noise is not None or rng is not None or uniform is not None or not propose):
        raise LsnfError("an inner leapfrog step draws and decides nothing: noise and uniform must be None, propose True")
    acc = la = None
    if not inner:
        def make():
            f32 = dict(dtype=torch.float32, device=dev)
            return {"acc": torch.empty(B, **f32), "la": torch.empty(B, **f32)}
        bufs = _stream_buffers(plan, "_rhmc_buffers", B, dev, make) if reuse_buffers else make()
        acc, la = bufs["acc"], bufs["la"]
    eps_next = None if not propose else eps_prop if inplace else torch.empty_like(eps_prop)
    _call("lsnf_reverse_hmc_step_tempered", dev, *_plan_head(plan), B, _ptr(eps_prop), _ptr(z_saved), _ptr(act_saved), _ptr(grad_g),
          _ptr(energy_g), _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(state.mom), _ptr(state.kin), _ptr(noise), _ptr(uniform),
          rng, step_ptr, adapt_ptr, da, *metric_args, *temper_args, flags, _ptr(eps_next), _ptr(acc), _ptr(la))
    return eps_next, acc, la


HMC_SWAP, HMC_SWAP_ODD = 128, 256     # include/lsnf_flow_mcmc.h LSNF_HMC_SWAP, LSNF_HMC_SWAP_ODD


def _row_exchange_mode(swap, ladder, phase, adapt, window, anneal):
    """What the exchanging calls check before `_check_chain`, beside `_row_temper_mode`: swap is None, "even" or "odd"; a swapping
    call is an end call that neither adapts, folds, closes nor anneals, and its ladder is 2, 4, 8 or 16.  Returns the swap's flags."""
    if swap is None:
        return 0
    if swap not in ("even", "odd"):
        raise LsnfError(f"swap must be None, 'even' or 'odd' (got {swap!r})")
    if phase != "end" or adapt is not None or window is not None or anneal is not None:
        raise LsnfError("replicas are exchanged between two trajectories of a frozen chain: swap goes with phase='end', "
                        "without adapt, window and anneal")
    if ladder not in (2, 4, 8, 16):
        raise LsnfError(f"ladder must be 2, 4, 8 or 16 (got {ladder!r})")
    return HMC_SWAP | (HMC_SWAP_ODD if swap == "odd" else 0)


def _row_exchange_args(plan, swap, ladder, swap_uniform, rng, B, dev, reuse_buffers):
    """After `_check_chain`: the swap's uniforms through the one checking path and its two outputs.  Returns (the four arguments in the
    order the C call names them: ladder, swap_uniform, swap_out, log_swap_out; swapped; log_swap) -- the last two None without swap."""
    _check_in(swap_uniform, "swap_uniform", B, dev)
    if swap is None:
        if swap_uniform is not None:
            raise LsnfError("swap_uniform goes with swap='even' or 'odd'")
        return (0, None, None, None), None, None
    if B % ladder:
        raise LsnfError(f"the chain's {B} rows are not a multiple of ladder={ladder}")
    if (rng is None) != (swap_uniform is not None):
        raise LsnfError("the swap draws as the trajectory does: swap_uniform with the tensors (noise, uniform=), none with a PhiloxNoise")

    def make():
        f32 = dict(dtype=torch.float32, device=dev)
        return {"swapped": torch.empty(B, **f32), "log_swap": torch.empty(B, **f32)}
    bufs = _stream_buffers(plan, "_hmcx_buffers", B, dev, make) if reuse_buffers else make()
    return (int(ladder), _ptr(swap_uniform), _ptr(bufs["swapped"]), _ptr(bufs["log_swap"])), bufs["swapped"], bufs["log_swap"]


def hmc_step_exchange(plan: FlowPlan, z_prop: torch.Tensor, grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor],
                      state: HmcState, noise, steps: HmcRowSteps, metric: HmcRowMetric, temper: HmcRowTemper, *, phase: str = "end",
                      uniform: Optional[torch.Tensor] = None, propose: bool = True, inplace: bool = False, reuse_buffers: bool = False,
                      adapt: Optional[str] = None, window: Optional[str] = None, anneal: Optional[torch.Tensor] = None,
                      swap: Optional[str] = None, ladder: int = 0, swap_uniform: Optional[torch.Tensor] = None):
    """`hmc_step_tempered` with a replica-exchange move between the rows of a ladder (include/lsnf_flow_mcmc.h
    `lsnf_hmc_step_exchange`): parallel tempering.  Rows [k * ladder, (k + 1) * ladder) are the rungs of ladder k at the temperatures
    temper.beta holds; ladder is 2, 4, 8 or 16 and divides B.
    swap (phase "end" only, without adapt / window / anneal): "even" pairs rungs (0,1), (2,3), ..; "odd" pairs (1,2), (3,4), .. and
    leaves the end rungs idle.  After the trajectory's decision the pair (a, b) swaps iff log(u) < (beta_a - beta_b) * (E_a - E_b),
    E the kept state's like_energy, u = swap_uniform[a] (with tensor noise) or drawn in-kernel (PhiloxNoise).  The STATES are
    exchanged: a swapping row takes the partner's state.z / like_grad / like_energy and its state.grad / state.energy re-tempered to
    the row's own beta, and begins the next trajectory (propose) from them; beta, step, scale and the adaptation stay with the row.
    Without swap this is `hmc_step_tempered` to the bit.  Returns that call's tuple plus (swapped, log_swap), both (B) -- 1.0 on both
    rows of an exchanged pair, and the pair's log ratio (0.0 on an idle rung) -- or (None, None) without swap."""
    flags, inner = _row_step_mode(steps, phase, adapt), phase == "inner"
    flags |= _row_metric_mode(metric, phase, window)
    flags |= _row_temper_mode(temper, phase, anneal)
    flags |= _row_exchange_mode(swap, ladder, phase, adapt, window, anneal)
    B, dev, noise, rng = _check_chain(plan, z_prop, "z_prop", grad_g, energy_g, state, HmcState, noise, uniform)
    step_ptr, adapt_ptr, da = _row_step_args(steps, B, dev, adapt)
    metric_args = _row_metric_args(plan, metric, B, dev, window)
    temper_args = _row_temper_args(plan, temper, B, dev, anneal)
    exchange_args, swapped, log_swap = _row_exchange_args(plan, swap, ladder, swap_uniform, rng, B, dev, reuse_buffers)
    if inner and (noise is not None or rng is not None or uniform is not None or not propose):
        raise LsnfError("an inner leapfrog step draws and decides nothing: noise and uniform must be None, propose True")
    bufs, z1, ll = _forward_at(plan, z_prop, B, dev, "_hmc_buffers", reuse_buffers)
    z_next = None if not propose else z_prop if inplace else torch.empty_like(z_prop)
    acc, la = (None, None) if inner else (bufs["acc"], bufs["la"])
    _call("lsnf_hmc_step_exchange", dev, *_plan_head(plan), B, _ptr(z_prop), _ptr(z1), _ptr(bufs["saved"]), _ptr(bufs["act"]), _ptr(ll),
          _ptr(grad_g), _ptr(energy_g), _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(state.mom), _ptr(state.kin), _ptr(noise),
          _ptr(uniform), rng, step_ptr, adapt_ptr, da, *metric_args, *temper_args, flags, _ptr(z_next), _ptr(acc), _ptr(la), *exchange_args)
    return z_next, acc, la, ll, swapped, log_swap


def reverse_hmc_step_exchange(plan: FlowPlan, eps_prop: torch.Tensor, z_saved: Optional[torch.Tensor], act_saved: torch.Tensor,
                              grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor], state: HmcState, noise, steps: HmcRowSteps,
                              metric: HmcRowMetric, temper: HmcRowTemper, *, phase: str = "end", uniform: Optional[torch.Tensor] = None,
                              propose: bool = True, inplace: bool = False, reuse_buffers: bool = False, adapt: Optional[str] = None,
                              window: Optional[str] = None, anneal: Optional[torch.Tensor] = None, swap: Optional[str] = None,
                              ladder: int = 0, swap_uniform: Optional[torch.Tensor] = None):
    """`reverse_hmc_step_tempered` with a replica-exchange move between the rows of a ladder (include/lsnf_flow_mcmc.h
    `lsnf_reverse_hmc_step_exchange`); swap, ladder and swap_uniform: as `hmc_step_exchange`'s, with the state (eps, eps + beta *
    like_grad, |eps|^2 / 2 + beta * like_energy).  ONE launch and nothing else, so a swapping end call can be captured in a graph.
    Returns `reverse_hmc_step_tempered`'s tuple plus (swapped, log_swap), (None, None) without swap."""
    flags, inner = _row_step_mode(steps, phase, adapt), phase == "inner"
    flags |= _row_metric_mode(metric, phase, window)
    flags |= _row_temper_mode(temper, phase, anneal)
    flags |= _row_exchange_mode(swap, ladder, phase, adapt, window, anneal)
    B, dev, noise, rng = _check_chain(plan, eps_prop, "eps_prop", grad_g, energy_g, state, HmcState, noise, uniform,
                                      stash=(z_saved, act_saved))
    step_ptr, adapt_ptr, da = _row_step_args(steps, B, dev, adapt)
    metric_args = _row_metric_args(plan, metric, B, dev, window)
    temper_args = _row_temper_args(plan, temper, B, dev, anneal)
    exchange_args, swapped, log_swap = _row_exchange_args(plan, swap, ladder, swap_uniform, rng, B, dev, reuse_buffers)
    if inner and (noise is not None or rng is not None or uniform is not None or not propose):
        raise LsnfError("an inner leapfrog step draws and decides nothing: noise and uniform must be None, propose True")
    acc = la = None
    if not inner:
        def make():
            f32 = dict(dtype=torch.float32, device=dev)
            return {"acc": torch.empty(B, **f32), "la": torch.empty(B, **f32)}
        bufs = _stream_buffers(plan, "_rhmc_buffers", B, dev, make) if reuse_buffers else make()
        acc, la = bufs["acc"], bufs["la"]
    eps_next = None if not propose else eps_prop if inplace else torch.empty_like(eps_prop)
    _call("lsnf_reverse_hmc_step_exchange", dev, *_plan_head(plan), B, _ptr(eps_prop), _ptr(z_saved), _ptr(act_saved), _ptr(grad_g),
          _ptr(energy_g), _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(state.mom), _ptr(state.kin), _ptr(noise), _ptr(uniform),
          rng, step_ptr, adapt_ptr, da, *metric_args, *temper_args, flags, _ptr(eps_next), _ptr(acc), _ptr(la), *exchange_args)
    return eps_next, acc, la, swapped, log_swap


HMC_RESAMPLE = 512     # include/lsnf_flow_mcmc.h LSNF_HMC_RESAMPLE
HMC_SCHEDULE = 1024    # include/lsnf_flow_mcmc.h LSNF_HMC_SCHEDULE


def _row_resample_mode(resample, phase, adapt, window, anneal, schedule=None, cess_target=0.95, min_step=0.0):
    """What the resampling and the scheduling calls check before `_check_chain`, beside `_row_temper_mode`: resample is None or the
    group's length P; a resampling call is an annealing end call that neither adapts, folds nor closes, and P is 2, 4, 8 or 16.
    schedule (the scheduling calls only) is None or the group's length as well: a scheduling call is an annealing init or end call
    that neither adapts, folds nor closes; with resample both lengths are equal.  Returns the moves' flags."""
    flags = 0
    if schedule is not None:
        if schedule not in (2, 4, 8, 16):
            raise LsnfError(f"schedule must be None, 2, 4, 8 or 16 (got {schedule!r})")
        if phase == "inner" or adapt is not None or window is not None or anneal is None:
            raise LsnfError("the next temperature is searched where a frozen chain anneals: schedule goes with phase='init' or 'end' "
                            "and anneal= (the ceiling), without adapt and window")
        if resample is not None and resample != schedule:
            raise LsnfError(f"schedule={schedule!r} and resample={resample!r} name the same groups: they must be equal")
        if not 0.0 < float(cess_target) < 1.0:
            raise LsnfError(f"cess_target must lie in (0, 1) (got {cess_target!r})")
        if not (math.isfinite(float(min_step)) and float(min_step) >= 0.0):
            raise LsnfError(f"min_step must be finite and not negative (got {min_step!r})")
        flags |= HMC_SCHEDULE
    if resample is None:
        return flags
    if resample not in (2, 4, 8, 16):
        raise LsnfError(f"resample must be None, 2, 4, 8 or 16 (got {resample!r})")
    if phase != "end" or adapt is not None or window is not None or anneal is None:
        raise LsnfError("particles are resampled between the weight increment and the next trajectory of a frozen chain: resample "
                        "goes with phase='end' and anneal=, without adapt and window")
    return flags | HMC_RESAMPLE


def _row_resample_args(plan, resample, ess_threshold, resample_uniform, rng, B, dev, reuse_buffers, schedule=None):
    """After `_check_chain`: the move's uniforms through the one checking path and its two outputs.  Returns (the five arguments in the
    order the C call names them: group, ess_frac, resample_uniform, ancestor_out, ess_out; ancestor; ess) -- the last two None without
    resample.  schedule (the scheduling calls only): the group's length where the call searches and does not resample."""
    _check_in(resample_uniform, "resample_uniform", B, dev)
    if schedule is not None and B % schedule:
        raise LsnfError(f"the chain's {B} rows are not a multiple of schedule={schedule}")
    if resample is None:
        if resample_uniform is not None:
            raise LsnfError("resample_uniform goes with resample=P")
        return (0 if schedule is None else int(schedule), 0.0, None, None, None), None, None
    if B % resample:
        raise LsnfError(f"the chain's {B} rows are not a multiple of resample={resample}")
    if (rng is None) != (resample_uniform is not None):
        raise LsnfError("the move draws as the trajectory does: resample_uniform with the tensors (noise, uniform=), none with a "
                        "PhiloxNoise")

    def make():
        f32 = dict(dtype=torch.float32, device=dev)
        return {"ancestor": torch.empty(B, **f32), "ess": torch.empty(B, **f32)}
    bufs = _stream_buffers(plan, "_hmcs_buffers", B, dev, make) if reuse_buffers else make()
    return ((int(resample), float(ess_threshold), _ptr(resample_uniform), _ptr(bufs["ancestor"]), _ptr(bufs["ess"])),
            bufs["ancestor"], bufs["ess"])


def hmc_step_resample(plan: FlowPlan, z_prop: torch.Tensor, grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor],
                      state: HmcState, noise, steps: HmcRowSteps, metric: HmcRowMetric, temper: HmcRowTemper, *, phase: str = "end",
                      uniform: Optional[torch.Tensor] = None, propose: bool = True, inplace: bool = False, reuse_buffers: bool = False,
                      adapt: Optional[str] = None, window: Optional[str] = None, anneal: Optional[torch.Tensor] = None,
                      resample: Optional[int] = None, ess_threshold: float = 0.5, resample_uniform: Optional[torch.Tensor] = None):
    """`hmc_step_tempered` with a resampling move between the rows of a group (include/lsnf_flow_mcmc.h `lsnf_hmc_step_resample`): the
    step of a sequential Monte Carlo sampler.  Rows [k * P, (k + 1) * P) are the particles of group k; P = resample is 2, 4, 8 or 16
    and divides B.
    resample (phase "end" with anneal=, without adapt / window): after the trajectory's decision and the weight increment, a group
    whose effective sample size (sum w)^2 / sum w^2 is below ess_threshold * P is resampled systematically with ONE uniform, u =
    resample_uniform[first row of the group] (with tensor noise) or drawn in-kernel (PhiloxNoise).  A row whose ancestor is another
    row takes that row's state.z / like_grad / like_energy and its state.grad / state.energy re-tempered to the row's own beta, and
    begins the next trajectory (propose) from them; every row of the group gets the group's mean weight, log_w = {log mean w, 0}.
    beta, step, scale and the adaptation stay with the row.  Without resample this is `hmc_step_tempered` to the bit.  Returns that
    call's tuple plus (ancestor, ess), both (B) -- the rung a row's state came from (its own where nothing moved), and the group's
    effective sample size -- or (None, None) without resample."""
    return _hmc_step_group("lsnf_hmc_step_resample", plan, z_prop, grad_g, energy_g, state, noise, steps, metric, temper,
                           phase=phase, uniform=uniform, propose=propose, inplace=inplace, reuse_buffers=reuse_buffers, adapt=adapt,
                           window=window, anneal=anneal, resample=resample, ess_threshold=ess_threshold, resample_uniform=resample_uniform)


def _hmc_step_group(entry, plan, z_prop, grad_g, energy_g, state, noise, steps, metric, temper, *, phase, uniform, propose, inplace,
                    reuse_buffers, adapt, window, anneal, resample, ess_threshold, resample_uniform, search=None):
    """The body of `hmc_step_resample` and `hmc_step_schedule`: entry is the C call; search: None, or the scheduling entry's
    (schedule, cess_target, min_step), whose last two the C call takes behind ess_out."""
    schedule, cess_target, min_step = (None, 0.95, 0.0) if search is None else search
    tail = () if search is None else (float(cess_target), float(min_step))
    flags, inner = _row_step_mode(steps, phase, adapt), phase == "inner"
    flags |= _row_metric_mode(metric, phase, window)
    flags |= _row_temper_mode(temper, phase, anneal)
    flags |= _row_resample_mode(resample, phase, adapt, window, anneal, schedule, cess_target, min_step)
    B, dev, noise, rng = _check_chain(plan, z_prop, "z_prop", grad_g, energy_g, state, HmcState, noise, uniform)
    step_ptr, adapt_ptr, da = _row_step_args(steps, B, dev, adapt)
    metric_args = _row_metric_args(plan, metric, B, dev, window)
    temper_args = _row_temper_args(plan, temper, B, dev, anneal)
    resample_args, ancestor, ess = _row_resample_args(plan, resample, ess_threshold, resample_uniform, rng, B, dev, reuse_buffers, schedule)
    if inner and (noise is not None or rng is not None or uniform is not None or not propose):
        raise LsnfError("an inner leapfrog step draws and decides nothing: noise and uniform must be None, propose True")
    bufs, z1, ll = _forward_at(plan, z_prop, B, dev, "_hmc_buffers", reuse_buffers)
    z_next = None if not propose else z_prop if inplace else torch.empty_like(z_prop)
    acc, la = (None, None) if inner else (bufs["acc"], bufs["la"])
    _call(entry, dev, *_plan_head(plan), B, _ptr(z_prop), _ptr(z1), _ptr(bufs["saved"]), _ptr(bufs["act"]), _ptr(ll),
          _ptr(grad_g), _ptr(energy_g), _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(state.mom), _ptr(state.kin), _ptr(noise),
          _ptr(uniform), rng, step_ptr, adapt_ptr, da, *metric_args, *temper_args, flags, _ptr(z_next), _ptr(acc), _ptr(la), *resample_args,
          *tail)
    return z_next, acc, la, ll, ancestor, ess


def reverse_hmc_step_resample(plan: FlowPlan, eps_prop: torch.Tensor, z_saved: Optional[torch.Tensor], act_saved: torch.Tensor,
                              grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor], state: HmcState, noise, steps: HmcRowSteps,
                              metric: HmcRowMetric, temper: HmcRowTemper, *, phase: str = "end", uniform: Optional[torch.Tensor] = None,
                              propose: bool = True, inplace: bool = False, reuse_buffers: bool = False, adapt: Optional[str] = None,
                              window: Optional[str] = None, anneal: Optional[torch.Tensor] = None, resample: Optional[int] = None,
                              ess_threshold: float = 0.5, resample_uniform: Optional[torch.Tensor] = None):
    """`reverse_hmc_step_tempered` with a resampling move between the rows of a group (include/lsnf_flow_mcmc.h
    `lsnf_reverse_hmc_step_resample`); resample, ess_threshold and resample_uniform: as `hmc_step_resample`'s, with the state (eps,
    eps + beta * like_grad, |eps|^2 / 2 + beta * like_energy).  ONE launch and nothing else, so a resampling end call can be captured
    in a graph.  Returns `reverse_hmc_step_tempered`'s tuple plus (ancestor, ess), (None, None) without resample."""
    return _reverse_hmc_step_group("lsnf_reverse_hmc_step_resample", plan, eps_prop, z_saved, act_saved, grad_g, energy_g, state, noise, steps,
                                   metric, temper, phase=phase, uniform=uniform, propose=propose, inplace=inplace,
                                   reuse_buffers=reuse_buffers, adapt=adapt, window=window, anneal=anneal, resample=resample,
                                   ess_threshold=ess_threshold, resample_uniform=resample_uniform)


def _reverse_hmc_step_group(entry, plan, eps_prop, z_saved, act_saved, grad_g, energy_g, state, noise, steps, metric, temper, *, phase,
                            uniform, propose, inplace, reuse_buffers, adapt, window, anneal, resample, ess_threshold, resample_uniform,
                            search=None):
    """The body of `reverse_hmc_step_resample` and `reverse_hmc_step_schedule`, as `_hmc_step_group`."""
    schedule, cess_target, min_step = (None, 0.95, 0.0) if search is None else search
    tail = () if search is None else (float(cess_target), float(min_step))
    flags, inner = _row_step_mode(steps, phase, adapt), phase == "inner"
    flags |= _row_metric_mode(metric, phase, window)
    flags |= _row_temper_mode(temper, phase, anneal)
    flags |= _row_resample_mode(resample, phase, adapt, window, anneal, schedule, cess_target, min_step)
    B, dev, noise, rng = _check_chain(plan, eps_prop, "eps_prop", grad_g, energy_g, state, HmcState, noise, uniform,
                                      stash=(z_saved, act_saved))
    step_ptr, adapt_ptr, da = _row_step_args(steps, B, dev, adapt)
    metric_args = _row_metric_args(plan, metric, B, dev, window)
    temper_args = _row_temper_args(plan, temper, B, dev, anneal)
    resample_args, ancestor, ess = _row_resample_args(plan, resample, ess_threshold, resample_uniform, rng, B, dev, reuse_buffers, schedule)
    if inner and (noise is not None or rng is not None or uniform is not None or not propose):
        raise LsnfError("an inner leapfrog step draws and decides nothing: noise and uniform must be None, propose True")
    acc = la = None
    if not inner:
        def make():
            f32 = dict(dtype=torch.float32, device=dev)
            return {"acc": torch.empty(B, **f32), "la": torch.empty(B, **f32)}
        bufs = _stream_buffers(plan, "_rhmc_buffers", B, dev, make) if reuse_buffers else make()
        acc, la = bufs["acc"], bufs["la"]
    eps_next = None if not propose else eps_prop if inplace else torch.empty_like(eps_prop)
    _call(entry, dev, *_plan_head(plan), B, _ptr(eps_prop), _ptr(z_saved), _ptr(act_saved), _ptr(grad_g),
          _ptr(energy_g), _ptr(state.z), _ptr(state.grad), _ptr(state.energy), _ptr(state.mom), _ptr(state.kin), _ptr(noise), _ptr(uniform),
          rng, step_ptr, adapt_ptr, da, *metric_args, *temper_args, flags, _ptr(eps_next), _ptr(acc), _ptr(la), *resample_args, *tail)
    return eps_next, acc, la, ancestor, ess


def hmc_step_schedule(plan: FlowPlan, z_prop: torch.Tensor, grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor],
                      state: HmcState, noise, steps: HmcRowSteps, metric: HmcRowMetric, temper: HmcRowTemper, *, phase: str = "end",
                      uniform: Optional[torch.Tensor] = None, propose: bool = True, inplace: bool = False, reuse_buffers: bool = False,
                      adapt: Optional[str] = None, window: Optional[str] = None, anneal: Optional[torch.Tensor] = None,
                      resample: Optional[int] = None, ess_threshold: float = 0.5, resample_uniform: Optional[torch.Tensor] = None,
                      schedule: Optional[int] = None, cess_target: float = 0.95, min_step: float = 0.0):
    """`hmc_step_resample` with the groups' next temperature searched inside the kernel (include/lsnf_flow_mcmc.h
    `lsnf_hmc_step_schedule`): adaptive tempering.  schedule = P (2, 4, 8 or 16, dividing B; equal to resample where both are given)
    on an annealing init or end call (anneal=, without adapt / window) makes anneal the groups' CEILING: every group of P rows steps
    from temper.beta to the temperature at which the conditional effective sample size of its incremental weights is cess_target * P
    (twelve halvings), by at least min_step and no further than the ceiling; temper.beta holds the chosen value afterwards, equal on
    the rows of a group.  temper.beta and anneal are read at the group's first row: keep both equal within a group.  The weight
    increment, the re-tempering and the resampling move (if asked for) then run as in `hmc_step_resample` with the chosen value.
    Without schedule this is `hmc_step_resample` to the bit.  ONE launch and nothing else.  Returns `hmc_step_resample`'s tuple."""
    return _hmc_step_group("lsnf_hmc_step_schedule", plan, z_prop, grad_g, energy_g, state, noise, steps, metric, temper,
                           phase=phase, uniform=uniform, propose=propose, inplace=inplace, reuse_buffers=reuse_buffers, adapt=adapt,
                           window=window, anneal=anneal, resample=resample, ess_threshold=ess_threshold, resample_uniform=resample_uniform,
                           search=(schedule, cess_target, min_step))


def reverse_hmc_step_schedule(plan: FlowPlan, eps_prop: torch.Tensor, z_saved: Optional[torch.Tensor], act_saved: torch.Tensor,
                              grad_g: Optional[torch.Tensor], energy_g: Optional[torch.Tensor], state: HmcState, noise, steps: HmcRowSteps,
                              metric: HmcRowMetric, temper: HmcRowTemper, *, phase: str = "end", uniform: Optional[torch.Tensor] = None,
                              propose: bool = True, inplace: bool = False, reuse_buffers: bool = False, adapt: Optional[str] = None,
                              window: Optional[str] = None, anneal: Optional[torch.Tensor] = None, resample: Optional[int] = None,
                              ess_threshold: float = 0.5, resample_uniform: Optional[torch.Tensor] = None,
                              schedule: Optional[int] = None, cess_target: float = 0.95, min_step: float = 0.0):
    """`reverse_hmc_step_resample` with the groups' next temperature searched inside the kernel (include/lsnf_flow_mcmc.h
    `lsnf_reverse_hmc_step_schedule`); schedule, cess_target and min_step: as `hmc_step_schedule`'s.  ONE launch and nothing else, so a
    scheduling call can be captured in a graph.  Returns `reverse_hmc_step_resample`'s tuple."""
    return _reverse_hmc_step_group("lsnf_reverse_hmc_step_schedule", plan, eps_prop, z_saved, act_saved, grad_g, energy_g, state, noise, steps,
                                   metric, temper, phase=phase, uniform=uniform, propose=propose, inplace=inplace,
                                   reuse_buffers=reuse_buffers, adapt=adapt, window=window, anneal=anneal, resample=resample,
                                   ess_threshold=ess_threshold, resample_uniform=resample_uniform,
                                   search=(schedule, cess_target, min_step))

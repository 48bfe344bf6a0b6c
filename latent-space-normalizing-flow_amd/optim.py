"""`FlowAdam`: torch.optim.Adam for the flow prior with the clip and the update on the device in one or two launches
(`flow.adam_step`, csrc/lsnf_optim.hip) instead of a foreach clip over 60 tensors plus `Adam.step()` over 70 parameters
(reference train.py:295, 413-415).  Opt-in: `torch.optim.Adam(netF.parameters())` keeps working as before."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import flow
from ._lib import LsnfError


class FlowAdam(torch.optim.Optimizer):
    """Adam (no amsgrad, no `maximize`, L2 weight decay -- torch.optim.Adam's defaults) over `netF.parameters()` in ONE param
    group, with an optional global-norm clip (`max_norm`, `clip_grad_norm_`'s formula) that runs inside `step()`.

        optF = FlowAdam(netF, lr=f_lr, betas=(f_beta1, f_beta2), weight_decay=f_decay, max_norm=f_max_norm)   # train.py:295
        lr_scheduleF = torch.optim.lr_scheduler.ExponentialLR(optF, f_gamma)                                   # train.py:298

    `step()` reads `.grad` of the flow's live parameters (None: that tensor is skipped, as in torch -- the reference's dead
    `fc_*.b` parameters and frozen tensors), launches the kernels on the current stream and bumps the parameters' version
    counters (the stale-weights guard and the plan cache see the write).  It returns nothing and never synchronises; bits are
    reproducible run to run.  `last_grad_norm`: the pre-clip global norm of the last step as a 0-dim device tensor (a view
    into the optimizer state, overwritten by the next step), set when max_norm is given.
    capturable=True keeps the learning rate in a device float, so that a `step()` captured in a graph follows later changes
    of `param_groups[0]['lr']` (a scheduler's): `step()` refreshes the device value whenever the group's value changed, and
    `sync_lr()` does the same before a replay, which runs no Python.
    `state_dict()` / `load_state_dict()` speak torch.optim.Adam's format over the same parameter order (per parameter `step`,
    `exp_avg`, `exp_avg_sq`; only parameters that have taken a step carry state), so an `optF` entry of a reference checkpoint
    loads here and this optimizer's state loads into torch.optim.Adam.  ONE step count serves all tensors.
    There is no CPU path: a module that is not on the GPU raises LsnfError."""

    def __init__(self, netF, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0, max_norm: Optional[float] = None, capturable: bool = False):
        if not hasattr(netF, "_param_list"):
            raise LsnfError("FlowAdam optimizes a lsnf_amd._netF (pass the module, not its parameters)")
        live = netF._param_list()
        netF._require_gpu(live)
        super().__init__(netF.parameters(), dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, max_norm=max_norm))
        self._check_group(self.param_groups[0])
        self._netF = netF
        self.capturable = bool(capturable)
        hps = netF.hps
        self._geo = (netF.nz, hps.f_width, hps.f_depth, hps.f_flow_coupling)
        self._flat = flow.new_adam_state(*self._geo, live[0].device)
        self._steps, self._norm, self._m, self._v = flow.adam_state_views(self._flat, *self._geo)
        self._stepped = set()            # ABI slots of the live tensors that have taken a step (they carry state)
        self._lr_dev = self._lr_on_dev = None
        self.last_grad_norm: Optional[torch.Tensor] = None

    @staticmethod
    def _check_group(g) -> None:
        lr, (b1, b2), eps, wd, mn = g["lr"], g["betas"], g["eps"], g["weight_decay"], g.get("max_norm")
        if isinstance(lr, torch.Tensor):
            raise LsnfError("FlowAdam: lr must be a Python float (capturable=True keeps the device copy itself)")
        if not (lr >= 0.0 and eps >= 0.0 and wd >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise LsnfError(f"FlowAdam: invalid hyper-parameters lr={lr} betas={(b1, b2)} eps={eps} weight_decay={wd}")
        if mn is not None and not mn > 0.0:
            raise LsnfError(f"FlowAdam: max_norm must be positive or None (got {mn})")
        for k in ("amsgrad", "maximize", "decoupled_weight_decay"):
            if g.get(k):
                raise LsnfError(f"FlowAdam has no {k}")

    def add_param_group(self, param_group):
        if self.param_groups:
            raise LsnfError("FlowAdam has a single param group")
        super().add_param_group(param_group)

    def sync_lr(self) -> None:
        """capturable=True: copy `param_groups[0]['lr']` into the device float if it changed (one fill launch, no
        synchronisation).  `step()` calls it; call it yourself before replaying a captured step after a change of lr."""
        lr = float(self.param_groups[0]["lr"])
        if self._lr_dev is None:
            self._lr_dev = torch.empty(1, dtype=torch.float32, device=self._flat.device)
        if self._lr_on_dev != lr:
            self._lr_dev.fill_(lr)
            self._lr_on_dev = lr

    def _live(self):
        live = self._netF._param_list()
        if live[0].device != self._flat.device:
            raise LsnfError(f"the module moved to {live[0].device}; FlowAdam's state lives on {self._flat.device}")
        return live

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise LsnfError("FlowAdam.step takes no closure")
        g = self.param_groups[0]
        self._check_group(g)
        live = self._live()
        grads = [p.grad for p in live]
        if self.capturable:
            self.sync_lr()
        norm = flow.adam_step(live, grads, self._flat, *self._geo, lr=g["lr"], betas=g["betas"],
                              eps=g["eps"], weight_decay=g["weight_decay"], max_norm=g["max_norm"],
                              lr_dev=self._lr_dev if self.capturable else None)
        written = [p for p, gr in zip(live, grads) if gr is not None]
        if written:       # the kernel wrote through raw pointers (as the actnorm init does)
            torch.autograd.graph.increment_version(written)
        self._stepped.update(i for i, gr in enumerate(grads) if gr is not None)
        if norm is not None:
            self.last_grad_norm = norm

    # ---- torch.optim.Adam's state format ----------------------------------------------------------------------------------
    def _slot_of(self):
        """position in param_groups[0]['params'] -> ABI slot of the live tensors (dead parameters have none)"""
        slot = {id(p): i for i, p in enumerate(self._live())}
        return [slot.get(id(p)) for p in self.param_groups[0]["params"]]

    def state_dict(self):
        g = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        g.update(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False,
                 params=list(range(len(self.param_groups[0]["params"]))))
        state = {}
        if self._stepped:
            step = torch.tensor(float(self._steps[0].item()), dtype=torch.float32)
            for pos, slot in enumerate(self._slot_of()):
                if slot in self._stepped:
                    state[pos] = {"step": step.clone(), "exp_avg": self._m[slot].clone(), "exp_avg_sq": self._v[slot].clone()}
        return {"state": state, "param_groups": [g]}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.param_groups[0]["params"]):
            raise LsnfError("FlowAdam.load_state_dict: expected one param group over the module's parameters")
        new = {k: v for k, v in groups[0].items() if k in ("lr", "betas", "eps", "weight_decay", "max_norm", "initial_lr")}
        merged = dict(self.param_groups[0], **new)
        merged["betas"] = tuple(merged["betas"])
        self._check_group(dict(merged, **{k: groups[0].get(k) for k in ("amsgrad", "maximize", "decoupled_weight_decay")}))
        slots = self._slot_of()
        pos_of = {pid: pos for pos, pid in enumerate(groups[0]["params"])}
        steps, entries = set(), {}
        for pid, st in state_dict["state"].items():
            slot = slots[pos_of[pid]]
            if slot is None:
                raise LsnfError(f"FlowAdam.load_state_dict: parameter {pid} carries state but does not reach the kernels")
            if "max_exp_avg_sq" in st:
                raise LsnfError("FlowAdam has no amsgrad")
            steps.add(int(float(st["step"])))
            entries[slot] = st
        if len(steps) > 1:
            raise LsnfError(f"FlowAdam keeps one step count for all tensors; the state has {sorted(steps)}")
        for slot, (m, v) in enumerate(zip(self._m, self._v)):
            st = entries.get(slot)
            if st is None:
                m.zero_(); v.zero_()
            else:
                if st["exp_avg"].shape != m.shape or st["exp_avg_sq"].shape != v.shape:
                    raise LsnfError(f"FlowAdam.load_state_dict: state of tensor {slot} has shape {tuple(st['exp_avg'].shape)}, expected {tuple(m.shape)}")
                m.copy_(st["exp_avg"]); v.copy_(st["exp_avg_sq"])
        self._steps.fill_(steps.pop() if steps else 0)
        self._stepped = set(entries)
        self.param_groups[0].update(merged)

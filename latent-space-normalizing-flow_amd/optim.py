"""`FlowAdam`: torch.optim.Adam for the flow prior with the clip and the update on the device in one or two launches
(`flow.adam_step`, csrc/lsnf_optim.hip) instead of a foreach clip over 60 tensors plus `Adam.step()` over 70 parameters
(reference train.py:295, 413-415).  Opt-in: `torch.optim.Adam(netF.parameters())` keeps working as before.
`FlowAdamW`: the same with AdamW's decoupled weight decay and torch.optim.AdamW's default of 1e-2."""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional, Tuple

import torch

from . import flow
from ._lib import LsnfError


class FlowAdam(torch.optim.Optimizer):
    """Adam (torch.optim.Adam's arithmetic: L2 weight decay unless decoupled_weight_decay, optional amsgrad / maximize) over
    `netF.parameters()` in ONE param group, with an optional global-norm clip (`max_norm`, `clip_grad_norm_`'s formula) that
    runs inside `step()`.

        optF = FlowAdam(netF, lr=f_lr, betas=(f_beta1, f_beta2), weight_decay=f_decay, max_norm=f_max_norm)   # train.py:295
        lr_scheduleF = torch.optim.lr_scheduler.ExponentialLR(optF, f_gamma)                                   # train.py:298

    `step()` reads `.grad` of the flow's live parameters (None: that tensor is skipped, as in torch -- the reference's dead
    `fc_*.b` parameters and frozen tensors), launches the kernels on the current stream and bumps the parameters' version
    counters (the stale-weights guard and the plan cache see the write).  It returns nothing and never synchronises; bits are
    reproducible run to run.  `last_grad_norm`: the pre-clip global norm of the last step as a 0-dim device tensor (a view
    into the optimizer state, overwritten by the next step), set when max_norm or skip_nonfinite is given.
    capturable=True keeps the learning rate in a device float, so that a `step()` captured in a graph follows later changes
    of `param_groups[0]['lr']` (a scheduler's): `step()` refreshes the device value whenever the group's value changed, and
    `sync_lr()` does the same before a replay, which runs no Python.  (Decoupled decay reads that device value too.)
    amsgrad, maximize, decoupled_weight_decay: as in torch.optim.Adam.  amsgrad sizes the state, so it is fixed at
    construction; the other two live in the param group and may change between steps.
    ema_decay: keep e <- e + (1 - ema_decay) (p - e) of the parameters as each step stores them, on the device, inside the
    same launch (`ema_parameters()`, `ema_state_dict()`, `copy_ema_to()`); the average starts from the parameters the first
    step finds, and tensors without a gradient take part.  Fixed at construction as a yes / no; the value lives in the group.
    skip_nonfinite: a step whose global gradient norm is inf or NaN writes nothing -- no parameter, no moment, no average, no
    step count -- but the norm and `skipped_steps` (a 0-dim int64 device view); nothing synchronises to find out.
    `state_dict()` / `load_state_dict()` speak torch.optim.Adam's format over the same parameter order (per parameter `step`,
    `exp_avg`, `exp_avg_sq`, under amsgrad `max_exp_avg_sq`, under ema_decay `ema`; only parameters that have taken a step
    carry state), so an `optF` entry of a reference checkpoint loads here and this optimizer's state loads into
    torch.optim.Adam / AdamW.  ONE step count serves all tensors.
    There is no CPU path: a module that is not on the GPU raises LsnfError."""

    def __init__(self, netF, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0, max_norm: Optional[float] = None, capturable: bool = False, amsgrad: bool = False,
                 maximize: bool = False, decoupled_weight_decay: bool = False, ema_decay: Optional[float] = None,
                 skip_nonfinite: bool = False):
        if not hasattr(netF, "_param_list"):
            raise LsnfError("FlowAdam optimizes a lsnf_amd._netF (pass the module, not its parameters)")
        live = netF._param_list()
        netF._require_gpu(live)
        super().__init__(netF.parameters(), dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, max_norm=max_norm,
                                                 amsgrad=bool(amsgrad), maximize=bool(maximize),
                                                 decoupled_weight_decay=bool(decoupled_weight_decay), ema_decay=ema_decay,
                                                 skip_nonfinite=bool(skip_nonfinite)))
        self._amsgrad, self._ema = bool(amsgrad), ema_decay is not None       # these two size the state: fixed from here on
        self._check_group(self.param_groups[0])
        self._netF = netF
        self.capturable = bool(capturable)
        hps = netF.hps
        self._geo = (netF.nz, hps.f_width, hps.f_depth, hps.f_flow_coupling)
        self._flat = flow.new_adam_state(*self._geo, live[0].device, amsgrad=self._amsgrad, ema=self._ema)
        self._steps, self._norm, self._m, self._v = flow.adam_state_views(self._flat, *self._geo)
        self._vmax, self._avg, self._skipped = flow.adam_state_extra_views(self._flat, *self._geo, self._amsgrad, self._ema)
        self._stepped = set()            # ABI slots of the live tensors that have taken a step (they carry state)
        self._lr_dev = self._lr_on_dev = None
        self.last_grad_norm: Optional[torch.Tensor] = None

    def _check_group(self, g) -> None:
        lr, (b1, b2), eps, wd, mn = g["lr"], g["betas"], g["eps"], g["weight_decay"], g.get("max_norm")
        if isinstance(lr, torch.Tensor):
            raise LsnfError("FlowAdam: lr must be a Python float (capturable=True keeps the device copy itself)")
        if not (lr >= 0.0 and eps >= 0.0 and wd >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise LsnfError(f"FlowAdam: invalid hyper-parameters lr={lr} betas={(b1, b2)} eps={eps} weight_decay={wd}")
        if mn is not None and not mn > 0.0:
            raise LsnfError(f"FlowAdam: max_norm must be positive or None (got {mn})")
        ed = g["ema_decay"]
        if g["amsgrad"] != self._amsgrad:
            raise LsnfError(f"FlowAdam: amsgrad={g['amsgrad']} but the optimizer was built with amsgrad={self._amsgrad} "
                            "(it sizes the state buffer: build a new FlowAdam)")
        if (ed is not None) != self._ema:
            raise LsnfError(f"FlowAdam: ema_decay={ed} but the optimizer was built {'with' if self._ema else 'without'} a weight "
                            "average (it sizes the state buffer: build a new FlowAdam)")
        if ed is not None and not 0.0 <= ed < 1.0:
            raise LsnfError(f"FlowAdam: ema_decay must lie in [0, 1) or be None (got {ed})")

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
                              lr_dev=self._lr_dev if self.capturable else None, amsgrad=self._amsgrad,
                              maximize=g["maximize"], decoupled_weight_decay=g["decoupled_weight_decay"],
                              ema_decay=g["ema_decay"], skip_nonfinite=g["skip_nonfinite"])
        written = [p for p, gr in zip(live, grads) if gr is not None]
        if written:       # the kernel wrote through raw pointers (as the actnorm init does)
            torch.autograd.graph.increment_version(written)
        self._stepped.update(i for i, gr in enumerate(grads) if gr is not None)
        if norm is not None:
            self.last_grad_norm = norm

    # ---- non-finite skip and the weight average ---------------------------------------------------------------------------
    @property
    def skipped_steps(self) -> torch.Tensor:
        """How many steps skip_nonfinite refused so far: a 0-dim int64 view into the optimizer state on the device (reading
        it synchronises, `step()` does not).  `load_state_dict` leaves it alone."""
        return self._skipped

    def ema_parameters(self) -> List[torch.Tensor]:
        """The averages of the depth*12 live tensors in ABI order, as views into the optimizer state (the next step overwrites
        them).  Before the first step they are zero: the average starts from the parameters that step finds."""
        if not self._ema:
            raise LsnfError("FlowAdam was built without ema_decay: there is no weight average")
        return list(self._avg)

    def _averaged(self) -> List[torch.Tensor]:
        """ema_parameters(), or the live parameters themselves while no step has started the average."""
        avg = self.ema_parameters()
        return avg if int(self._steps[0].item()) > 0 else [p.detach() for p in self._live()]

    def ema_state_dict(self):
        """The module's `state_dict()` with every live tensor replaced by (a copy of) its average; the other entries -- the
        reference's dead `fc_*.b` -- are copied as they are.  `netF_eval.load_state_dict(optF.ema_state_dict())` evaluates and
        samples with the averaged weights.  Synchronises (it reads the step count)."""
        slot = {p.data_ptr(): i for i, p in enumerate(self._live())}
        avg = self._averaged()
        out = OrderedDict()
        for k, t in self._netF.state_dict().items():
            i = slot.get(t.data_ptr())
            out[k] = (t if i is None else avg[i]).detach().clone()
        return out

    @torch.no_grad()
    def copy_ema_to(self, other) -> None:
        """Write the averages into the live parameters of `other`, a `_netF` of the same geometry on the same device (not this
        optimizer's own module: there is no in-place swap).  Bumps the version counters, so `other`'s plan refreshes."""
        hps = getattr(other, "hps", None)
        if not hasattr(other, "_param_list") or (other.nz, hps.f_width, hps.f_depth, hps.f_flow_coupling) != self._geo:
            raise LsnfError("copy_ema_to needs a lsnf_amd._netF of the optimizer's geometry")
        if other is self._netF:
            raise LsnfError("copy_ema_to: the target is the module being optimized (load ema_state_dict() into a second module)")
        dst = other._param_list()
        if dst[0].device != self._flat.device:
            raise LsnfError(f"copy_ema_to: the target lives on {dst[0].device}, the averages on {self._flat.device}")
        for q, e in zip(dst, self._averaged()):
            q.copy_(e)                   # (in place through the Parameter: the version counter moves)

    # ---- torch.optim.Adam's state format ----------------------------------------------------------------------------------
    def _slot_of(self):
        """position in param_groups[0]['params'] -> ABI slot of the live tensors (dead parameters have none)"""
        slot = {id(p): i for i, p in enumerate(self._live())}
        return [slot.get(id(p)) for p in self.param_groups[0]["params"]]

    def state_dict(self):
        g = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        g.update(amsgrad=self._amsgrad, maximize=bool(g.get("maximize")), foreach=None, capturable=False, differentiable=False, fused=None,
                 decoupled_weight_decay=bool(g.get("decoupled_weight_decay")),
                 params=list(range(len(self.param_groups[0]["params"]))))
        if g.get("ema_decay") is None:           # without the options the group is the one a plain FlowAdam always emitted
            g.pop("ema_decay", None)
        if not g.get("skip_nonfinite"):
            g.pop("skip_nonfinite", None)
        state = {}
        count = int(self._steps[0].item()) if self._stepped else 0
        if count > 0:                            # (0 with slots marked: every step so far was skipped)
            step = torch.tensor(float(count), dtype=torch.float32)
            for pos, slot in enumerate(self._slot_of()):
                if slot in self._stepped:
                    st = state[pos] = {"step": step.clone(), "exp_avg": self._m[slot].clone(), "exp_avg_sq": self._v[slot].clone()}
                    if self._amsgrad:
                        st["max_exp_avg_sq"] = self._vmax[slot].clone()
                    if self._ema:
                        st["ema"] = self._avg[slot].clone()
        return {"state": state, "param_groups": [g]}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.param_groups[0]["params"]):
            raise LsnfError("FlowAdam.load_state_dict: expected one param group over the module's parameters")
        # lr and its like are adopted from the dict, and so are maximize and decoupled_weight_decay (an AdamW checkpoint turns
        # the decay decoupled); amsgrad and the presence of an average must be the ones this optimizer was built with
        adopt = ("lr", "betas", "eps", "weight_decay", "max_norm", "initial_lr", "maximize", "decoupled_weight_decay", "amsgrad",
                 "ema_decay", "skip_nonfinite")
        new = {k: v for k, v in groups[0].items() if k in adopt}
        if self._ema and new.get("ema_decay") is None:       # a torch checkpoint: no word on an average, keep this one's decay
            new.pop("ema_decay", None)
        new.setdefault("amsgrad", False)
        merged = dict(self.param_groups[0], **new)
        merged["betas"] = tuple(merged["betas"])
        for k in ("amsgrad", "maximize", "decoupled_weight_decay", "skip_nonfinite"):
            merged[k] = bool(merged[k])
        self._check_group(merged)
        slots = self._slot_of()
        pos_of = {pid: pos for pos, pid in enumerate(groups[0]["params"])}
        steps, entries = set(), {}
        for pid, st in state_dict["state"].items():
            slot = slots[pos_of[pid]]
            if slot is None:
                raise LsnfError(f"FlowAdam.load_state_dict: parameter {pid} carries state but does not reach the kernels")
            if ("max_exp_avg_sq" in st) != self._amsgrad:
                raise LsnfError(f"FlowAdam.load_state_dict: the state of parameter {pid} is {'' if 'max_exp_avg_sq' in st else 'not '}"
                                f"amsgrad's, the optimizer was built with amsgrad={self._amsgrad}")
            if "ema" in st and not self._ema:
                raise LsnfError("FlowAdam.load_state_dict: the state carries a weight average, the optimizer was built without ema_decay")
            steps.add(int(float(st["step"])))
            entries[slot] = st
        if len(steps) > 1:
            raise LsnfError(f"FlowAdam keeps one step count for all tensors; the state has {sorted(steps)}")
        names = [("exp_avg", self._m), ("exp_avg_sq", self._v)] + ([("max_exp_avg_sq", self._vmax)] if self._amsgrad else [])
        for slot in range(len(self._m)):
            st = entries.get(slot)
            for name, views in names:
                if st is not None and st[name].shape != views[slot].shape:
                    raise LsnfError(f"FlowAdam.load_state_dict: {name} of tensor {slot} has shape {tuple(st[name].shape)}, "
                                    f"expected {tuple(views[slot].shape)}")
        live = self._live()
        for slot in range(len(self._m)):
            st = entries.get(slot)
            for name, views in names:
                if st is None:
                    views[slot].zero_()
                else:
                    views[slot].copy_(st[name])
            if self._ema:                        # no average in the state: it starts from the parameters as they are now
                self._avg[slot].copy_(st["ema"] if st is not None and "ema" in st else live[slot].detach())
        self._steps.fill_(steps.pop() if steps else 0)
        self._stepped = set(entries)
        self.param_groups[0].update(merged)


class FlowAdamW(FlowAdam):
    """`FlowAdam` with decoupled weight decay and torch.optim.AdamW's default decay of 1e-2: p <- p (1 - lr weight_decay) before
    the Adam update, the gradient left alone.  Its `state_dict()` loads into torch.optim.AdamW and the other way round."""

    def __init__(self, netF, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_norm: Optional[float] = None, capturable: bool = False, amsgrad: bool = False,
                 maximize: bool = False, ema_decay: Optional[float] = None, skip_nonfinite: bool = False):
        super().__init__(netF, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_norm=max_norm, capturable=capturable,
                         amsgrad=amsgrad, maximize=maximize, decoupled_weight_decay=True, ema_decay=ema_decay,
                         skip_nonfinite=skip_nonfinite)

"""`_netF`: drop-in replacement for the reference's flow prior (reference model.py:460-498).

Same constructor (`_netF(hps, nz)`), same `forward` signature and return conventions, the same
85-key `state_dict` (so reference checkpoints load unchanged, train.py:343-348), the same initial
distributions drawn in the same RNG order -- but every number is produced by the HIP kernels of
liblsnf_flow.so.  The sub-modules below only hold parameters under the reference's names; the
compute path is a single `torch.autograd.Function` around the fused stack kernels.

There is no CPU path: calling the module on CPU tensors raises `LsnfError`.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn

from . import flow
from ._lib import LsnfError


# ---------------------------------------------------------------------------------------------
# parameter holders (names / shapes / init mirror reference model.py:171-177, 227-233, 312-319,
# 334-342, 296-303, 367-387, 352-356)
# ---------------------------------------------------------------------------------------------
class actnorm(nn.Module):
    def __init__(self, nz):
        super().__init__()
        self.b = nn.Parameter(torch.randn(1, nz) * 0.05)
        self.register_parameter(name="bias", param=self.b)      # the reference's duplicate key (model.py:231)
        self.logs = nn.Parameter(torch.randn(1, nz) * 0.05)


class invertible_1x1_conv(nn.Module):
    def __init__(self, width, nz):
        super().__init__()
        w_init = np.linalg.qr(np.random.randn(nz, nz))[0].astype("float32")   # random orthogonal (model.py:176)
        self.w = nn.Parameter(torch.tensor(w_init, dtype=torch.float))


class fc(nn.Module):
    def __init__(self, n_in, width):
        super().__init__()
        self.width = width
        self.actnorm = actnorm(nz=width)
        self.w = nn.Parameter(torch.randn(n_in, width) * 0.05)
        self.b = nn.Parameter(torch.zeros(1, width))            # unused by the reference's forward (model.py:327-330)


class fc_zeros(nn.Module):
    def __init__(self, n_in, width):
        super().__init__()
        self.width = width
        self.w = nn.Parameter(torch.zeros(n_in, width))
        self.b = nn.Parameter(torch.zeros(1, width))
        self.logs = nn.Parameter(torch.zeros(1, width))


class f(nn.Module):
    def __init__(self, width, n_in=None, n_out=None):
        super().__init__()
        self.n_out = n_out
        self.fc_1 = fc(n_in, width)
        self.fc_2 = fc(width, width)
        self.fc_zeros = fc_zeros(width, n_out)


class revnet2d_step(nn.Module):
    def __init__(self, id, hps, nz):
        super().__init__()
        self.actnorm = actnorm(nz=nz)
        if hps.f_flow_permutation == 2:
            self.invertible_1x1_conv = invertible_1x1_conv(hps.f_width, nz=nz)
            self.shuffle_features = None
        else:
            # the reference's permutations 0 and 1 do not run; only the 1x1 conv exists here
            raise Exception("only f_flow_permutation == 2 (invertible 1x1 conv) is supported")
        self.id = id
        assert nz % 2 == 0
        if hps.f_flow_coupling == 1:
            self.f = f(hps.f_width, nz // 2, nz)
        elif hps.f_flow_coupling == 0:
            self.f = f(hps.f_width, nz // 2, nz // 2)      # additive coupling: shift only (model.py:385,407-408)
        else:
            raise Exception()

    def live_parameters(self) -> List[nn.Parameter]:
        """The 12 tensors that reach the kernels, in the ABI's order (include/lsnf_flow.h)."""
        ff = self.f
        return [self.actnorm.b, self.actnorm.logs, self.invertible_1x1_conv.w,
                ff.fc_1.w, ff.fc_1.actnorm.b, ff.fc_1.actnorm.logs,
                ff.fc_2.w, ff.fc_2.actnorm.b, ff.fc_2.actnorm.logs,
                ff.fc_zeros.w, ff.fc_zeros.b, ff.fc_zeros.logs]


class revnet2d(nn.Module):
    def __init__(self, hps, nz):
        super().__init__()
        self.hps = hps
        self.revnet2d_step_s = nn.ModuleList([revnet2d_step(str(i), hps, nz=nz) for i in range(hps.f_depth)])


# ---------------------------------------------------------------------------------------------
# autograd bridge
# ---------------------------------------------------------------------------------------------
class _Upstream:
    """Hand-over between the two autograd nodes below (filled by _FlowStackFn.backward)."""
    __slots__ = ("g_z1", "g_logdet", "z", "z1", "saved", "plan_key", "act", "ws", "det", "empty")

    def __init__(self):
        self.g_z1 = self.g_logdet = self.z = self.z1 = self.saved = self.plan_key = self.act = self.ws = None
        self.det = False         # the module's deterministic_grads when the evaluation began (its workspace is sized by it)
        self.empty = False       # set by _FlowReverseFn.backward on an empty batch: the parameters get no gradient


class _ParamGate(torch.autograd.Function):
    """(*live_params) -> scalar token.  Exists so that parameter gradients are computed ONLY when the
    autograd engine actually needs them: `torch.autograd.grad(f, z)` in the Langevin loop (train.py:323)
    never executes this node's backward, `loss_f.backward()` (train.py:411) does."""

    @staticmethod
    def forward(ctx, module, holder, *params):
        ctx.module, ctx.holder, ctx.n = module, holder, len(params)
        return params[0].new_zeros(())

    @staticmethod
    def backward(ctx, _g_token):
        h, module = ctx.holder, ctx.module
        if h.empty:
            return (None, None) + (None,) * ctx.n
        if h.z1 is None:
            raise LsnfError("parameter gradients requested before the flow's backward ran")
        if module._current_key() != h.plan_key:     # the LIVE parameters, not the key cached at the last _plan() call
            raise LsnfError("flow parameters were modified between forward and backward")
        grads = flow.backward_params(module._plan(), module._param_list(), h.z, h.z1, h.saved, h.g_z1, h.g_logdet,
                                     act_saved=h.act if h.ws is not None else None, workspace=h.ws,
                                     deterministic=h.det)
        grads = [g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:])]
        return (None, None, *grads)


class _FlowStackFn(torch.autograd.Function):
    """(z, objective, token) -> (z1, logdet).  Forward: lsnf_forward (block outputs kept for the backward);
    backward: lsnf_backward_z for z; the upstream gradients are handed to _ParamGate for the parameters."""

    @staticmethod
    def forward(ctx, module, holder, z, objective, token):
        plan = module._plan()
        # z needs a gradient (the Langevin sampler, train.py:316-323): also keep the sigmoid / relu-mask stash so
        # that lsnf_backward_z does not recompute the coupling MLP.  z is a constant and the parameters are the leaves
        # (the flow-MLE step, train.py:404-411): keep the stash AND let the forward write the hidden activations into
        # the parameter-gradient workspace, so that lsnf_backward_params runs from the stash (flow.params_fast_path).
        B = z.shape[0]
        for_params = bool(B) and not ctx.needs_input_grad[2] and ctx.needs_input_grad[4] and flow.params_fast_path()
        act = flow.new_act_saved(plan, B, z.device) if (B and (ctx.needs_input_grad[2] or for_params)) else None
        ctx.det = bool(module.deterministic_grads)
        ws = flow.new_params_workspace(plan, B, z.device, deterministic=ctx.det) if for_params else None
        if ws is not None and z.data_ptr() % 16:
            z = z.clone()        # the fast path wants 16-byte aligned rows at large B (lsnf_forward, params_workspace)
        z1, logdet, _, saved = flow.forward(plan, z, objective, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
        ctx.module, ctx.holder = module, holder
        ctx.plan_key = module._plan_key
        ctx.act, ctx.ws = act, ws
        ctx.save_for_backward(z, z1, saved if saved is not None else z1.new_empty(0))
        return z1, logdet

    @staticmethod
    def backward(ctx, g_z1, g_logdet):
        module, h = ctx.module, ctx.holder
        z, z1, saved = ctx.saved_tensors
        if module._current_key() != ctx.plan_key:   # the LIVE parameters: an optimizer step / load_state_dict / EMA copy
            # between forward and backward would otherwise re-prepare the plan in place and pair new weights with the
            # activations saved from the old ones (PyTorch autograd raises a version-counter error in the same situation)
            raise LsnfError("flow parameters were modified between forward and backward")
        saved_t = saved if saved.numel() else None
        g_z1 = None if g_z1 is None else g_z1.contiguous()
        g_logdet = None if g_logdet is None else g_logdet.contiguous()
        g_z = flow.backward_z(module._plan(), z1, saved_t, g_z1, g_logdet, act_saved=ctx.act) if ctx.needs_input_grad[2] else None
        g_obj = g_logdet if ctx.needs_input_grad[3] else None
        g_tok = None
        if ctx.needs_input_grad[4]:
            h.g_z1, h.g_logdet, h.z, h.z1, h.saved, h.plan_key = g_z1, g_logdet, z, z1, saved_t, ctx.plan_key
            h.act, h.ws, h.det = ctx.act, ctx.ws, ctx.det
            g_tok = z1.new_zeros(())
        return None, None, g_z, g_obj, g_tok


class _FlowReverseFn(torch.autograd.Function):
    """(eps, objective, token) -> (x, objective_out) of the sampling direction.  Forward: the lsnf_reverse launch of the
    no_grad call (same bits).  Backward: lsnf_forward on the saved x (block outputs + stash), then lsnf_reverse_backward_z for
    eps; the parameters follow from the implicit-function theorem -- dL/dtheta of the reverse is lsnf_backward_params of the
    FORWARD at x with upstream gradients (-g_eps, -g_obj) -- so they are handed to _ParamGate like the forward direction's.
    With `module.reverse_keeps_stash` (where flow.reverse_keep_supported): the reverse launch itself keeps the block outputs and the
    stash (lsnf_reverse_keep), and the backward goes straight to lsnf_reverse_backward_z."""

    @staticmethod
    def _keeps(module, plan, B):
        return bool(module.reverse_keeps_stash) and B > 0 and flow.reverse_keep_supported(plan, B)

    @staticmethod
    def _keep_buffers(ctx, plan, B, want_tok):
        """(act, ws) of a stash-keeping forward: the workspace only if a parameter requires grad and the fast path is on."""
        ctx.act = flow.new_act_saved(plan, B, plan.device)
        ctx.ws = flow.new_params_workspace(plan, B, plan.device, deterministic=ctx.det) if (want_tok and flow.params_fast_path()) else None
        return ctx.act, ctx.ws

    @staticmethod
    def forward(ctx, module, holder, z, objective, token):
        plan = module._plan()
        ctx.module, ctx.holder = module, holder
        ctx.plan_key = module._plan_key
        ctx.obj_shape = objective.shape
        ctx.set_materialize_grads(False)
        ctx.det = bool(module.deterministic_grads)
        ctx.keeps = _FlowReverseFn._keeps(module, plan, z.shape[0])
        if ctx.keeps:
            act, ws = _FlowReverseFn._keep_buffers(ctx, plan, z.shape[0], ctx.needs_input_grad[4])
            x, obj, saved = flow.reverse(plan, z, objective, save_for_backward=True, act_saved=act, params_ws=ws)
            ctx.save_for_backward(x, z, saved if saved is not None else x.new_empty(0))
        else:
            x, obj = flow.reverse(plan, z, objective)
            ctx.save_for_backward(x)
        return x, obj

    @staticmethod
    def _backward(ctx, g_x, g_obj, want_tok):
        """(g_eps, g_obj made contiguous, g_tok) from the saved x: shared with _FlowSampleFn, which saves the same."""
        module, h = ctx.module, ctx.holder
        x = ctx.saved_tensors[0]
        if module._current_key() != ctx.plan_key:   # (see _FlowStackFn.backward)
            raise LsnfError("flow parameters were modified between forward and backward")
        plan = module._plan()
        B = x.shape[0]
        g_x = None if g_x is None else g_x.contiguous()
        g_obj = None if g_obj is None else g_obj.contiguous()
        h.empty = B == 0                                    # (an empty batch leaves the parameters without a gradient)
        need_tok = want_tok and B > 0
        if ctx.keeps:            # the reverse launch kept everything: z1 is its own input, the last block's output
            _, z1, saved = ctx.saved_tensors
            saved = saved if saved.numel() else None
            act, ws = ctx.act, ctx.ws
        else:
            for_params = need_tok and flow.params_fast_path()
            act = flow.new_act_saved(plan, B, x.device)
            ws = flow.new_params_workspace(plan, B, x.device, deterministic=ctx.det) if for_params else None
            if ws is not None and x.data_ptr() % 16:
                x = x.clone()        # the fast path wants 16-byte aligned rows at large B (lsnf_forward, params_workspace)
            z1, _, _, saved = flow.forward(plan, x, None, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
        g_eps = flow.reverse_backward_z(plan, z1, saved, act, g_x, g_obj)
        g_tok = None
        if need_tok:
            h.g_z1, h.g_logdet = g_eps.neg(), (None if g_obj is None else g_obj.neg())
            h.z, h.z1, h.saved, h.plan_key = x, z1, saved, ctx.plan_key
            h.act, h.ws, h.det = act, ws, ctx.det
            g_tok = z1.new_zeros(())
        return g_eps, g_obj, g_tok

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_x, g_obj):
        g_eps, g_obj, g_tok = _FlowReverseFn._backward(ctx, g_x, g_obj, ctx.needs_input_grad[4])
        return (None, None, g_eps if ctx.needs_input_grad[2] else None, g_obj.reshape(ctx.obj_shape) if (ctx.needs_input_grad[3] and g_obj is not None) else None, g_tok)


class _FlowSampleFn(torch.autograd.Function):
    """(token) -> (x, objective_out, eps, ll) of `_netF.sample`: _FlowReverseFn with the sampling launch (lsnf_sample) in place of
    lsnf_reverse.  eps is drawn, not an input: the only leaves are the parameters.  The node saves x alone, as the reverse does, so
    the backward is the reverse's; an upstream gradient on ll joins the objective's (ll = const(eps) - objective_out)."""

    @staticmethod
    def forward(ctx, module, holder, token, n, rng, temperature):
        plan = module._plan()
        ctx.module, ctx.holder = module, holder
        ctx.plan_key = module._plan_key
        ctx.set_materialize_grads(False)
        ctx.det = bool(module.deterministic_grads)
        ctx.keeps = _FlowReverseFn._keeps(module, plan, n)
        if ctx.keeps:
            act, ws = _FlowReverseFn._keep_buffers(ctx, plan, n, ctx.needs_input_grad[2])
            x, obj, eps, ll, saved = flow.sample(plan, n, rng, temperature=temperature, want_eps=True, want_ll=True,
                                                 save_for_backward=True, act_saved=act, params_ws=ws)
            ctx.save_for_backward(x, eps, saved if saved is not None else x.new_empty(0))
        else:
            x, obj, eps, ll = flow.sample(plan, n, rng, temperature=temperature, want_eps=True, want_ll=True)
            ctx.save_for_backward(x)
        ctx.mark_non_differentiable(eps)
        return x, obj, eps, ll

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_x, g_obj, _g_eps, g_ll):
        if g_ll is not None:
            g_obj = g_ll.neg() if g_obj is None else g_obj - g_ll
        _, _, g_tok = _FlowReverseFn._backward(ctx, g_x, g_obj, ctx.needs_input_grad[2])
        return None, None, g_tok, None, None, None


class _netF(nn.Module):
    """Reference model.py:460-498.  `hps` needs f_n_levels, f_depth, f_flow_permutation, f_width,
    f_flow_coupling (model.py:355-356,372-387,465)."""

    def __init__(self, hps, nz, *args, **kwargs):
        super().__init__(*args, **kwargs)
        revnet2d_s = []
        self.hps = hps
        self.nz = nz
        for i in range(hps.f_n_levels):
            revnet2d_s.append(revnet2d(hps, nz=nz))
            if i < hps.f_n_levels - 1:
                raise NotImplementedError      # as the reference (model.py:467-470): no split layer
        self.revnet2d_s = nn.ModuleList(revnet2d_s)
        self._cached_plan: Optional[flow.FlowPlan] = None
        self._plan_key = None
        # True: the differentiable reverse / sample launches keep the backward's stash themselves (lsnf_reverse_keep /
        # lsnf_sample_keep) where flow.reverse_keep_supported -- the backward then skips the forward pass at x; elsewhere (large
        # batches, MATH_FP32) the default bridge runs.  Default False: the bridge that recomputes the forward at x.
        self.reverse_keeps_stash = False
        # True: every route to parameter gradients -- the autograd bridges (forward, reverse, sample), mle_grads, mle_step and
        # langevin.flow_mle_step -- uses lsnf_backward_params_det and its workspace: fixed-order sums over the batch, the same bits
        # on every run.  Read once per evaluation, when its forward (or reverse / sample) runs.  This attribute alone decides; torch.use_deterministic_algorithms is not consulted.
        self.deterministic_grads = False

    # ---- prepared weights, re-derived only when a parameter changed -------------------------------
    def _param_list(self) -> List[nn.Parameter]:
        """The depth*12 live Parameter objects in ABI order (cached: module traversal costs ~80 us per call;
        `.to()`, optimizer steps and load_state_dict keep the Parameter objects, only their storage changes)."""
        cached = self.__dict__.get("_live_params")
        if cached is None:
            cached = []
            for step in self.revnet2d_s[0].revnet2d_step_s:
                cached += step.live_parameters()
            self.__dict__["_live_params"] = cached
        return cached

    def _apply(self, fn, *args, **kwargs):     # .to() / .cuda() / .float(): drop caches that hold device state
        self.__dict__.pop("_live_params", None)
        self._cached_plan, self._plan_key = None, None
        return super()._apply(fn, *args, **kwargs)

    def _current_key(self):
        """Identity of the live parameter values as autograd sees them: (storage address, version counter) per tensor.
        In-place updates through the Parameter (optimizer steps, `load_state_dict`, `p.mul_()` under no_grad) bump the
        version; writes through `p.data` (`p.data.copy_()`, `p.data.clamp_()`) do NOT -- `.data` has its own counter --
        so code that edits weights that way must call `invalidate_plan()`."""
        return tuple((p.data_ptr(), p._version) for p in self._param_list())

    def invalidate_plan(self) -> None:
        """Force the next call to re-derive the prepared weights (after writes through `p.data`, which no version
        counter records)."""
        self._plan_key = None

    @staticmethod
    def _require_gpu(params) -> None:
        for p in params:
            if not p.is_cuda:
                raise LsnfError("_netF lives on %s: move it to the GPU (netF.to(device)); there is no CPU path" % p.device)

    def _plan(self) -> flow.FlowPlan:
        params = self._param_list()
        key = self._current_key()
        if self._cached_plan is None or key != self._plan_key or self._cached_plan.device != params[0].device:
            self._require_gpu(params)
            reuse = self._cached_plan if (self._cached_plan is not None and
                                          self._cached_plan.device == params[0].device) else None
            with torch.no_grad():
                tensors = [p.detach().contiguous() for p in params]
                self._cached_plan = flow.prepare(tensors, self.nz, self.hps.f_width, self.hps.f_depth,
                                                 self.hps.f_flow_coupling, plan=reuse)
            self._plan_key = key
        return self._cached_plan

    # ---- reference forward signature (model.py:473) ---------------------------------------------
    def forward(self, z, objective, init=False, reverse=False, eps=None, eps_std=None, z2_s=None, return_obj=False):
        if init and not reverse and not (z.is_cuda and all(p.is_cuda for p in self._param_list())):
            raise NotImplementedError("data-dependent init (init=True) has no CPU path: move the module and z to the GPU")
        if z.dim() != 2:
            raise ValueError(f"z must be (B, nz); got shape {tuple(z.shape)} (note: the reference's "
                             f"torch.squeeze(z) call site breaks for B == 1, train.py:316)")
        z = z.contiguous()
        objective = objective.contiguous()
        if not reverse:
            params = self._param_list()
            if init:      # model.py:238-241,253-262: fit the actnorms to this batch, then the plain forward with the new values
                if z.shape[0] == 0:
                    raise LsnfError("data-dependent init needs a non-empty batch")
                flow.actnorm_init([p.detach() for p in params], z.detach(), self.nz, self.hps.f_width, self.hps.f_depth,
                                  self.hps.f_flow_coupling)
                # the kernels wrote through raw pointers: bump the version counters so that the cached plan is re-derived
                # and a graph recorded before this call refuses to back-propagate (_current_key)
                written = [p for i, p in enumerate(params) if i % flow.LSNF_PARAMS_PER_BLOCK in (0, 1, 4, 5, 7, 8)]
                torch.autograd.graph.increment_version(written)
            if torch.is_grad_enabled() and (z.requires_grad or objective.requires_grad or
                                            any(p.requires_grad for p in params)):
                holder = _Upstream()
                token = _ParamGate.apply(self, holder, *params)
                z1, logdet = _FlowStackFn.apply(self, holder, z, objective, token)
            else:
                z1, logdet, _, _ = flow.forward(self._plan(), z.detach(), objective.detach(), want_ll=False)
            return z1, logdet, []
        if torch.is_grad_enabled() and (z.requires_grad or objective.requires_grad or
                                        any(p.requires_grad for p in self._param_list())):
            # differentiable sampling (the reference's reverse is plain eager PyTorch, model.py:424-456,484-498)
            holder = _Upstream()
            token = _ParamGate.apply(self, holder, *self._param_list())
            x, obj = _FlowReverseFn.apply(self, holder, z, objective, token)
        else:
            x, obj = flow.reverse(self._plan(), z.detach(), objective.detach())
        if not return_obj:
            return x
        return x, -obj

    # ---- fused prior sampling (train.py:472-475: `torch.randn` + `netF(z, zeros, reverse=True)`) ----------
    def sample(self, n, philox, temperature=1.0, return_eps=False, return_log_prob=False):
        """n samples x = f^-1(temperature * eps) of the flow prior in ONE launch: eps ~ N(0, 1) is drawn inside the reverse
        kernel (`flow.sample`), so there is no `randn` launch and no (n, nz) latent tensor, and the draw is a pure function of
        (seed, offset, row0 + row, column) -- the same rows however they are sharded over GPUs.
        philox: a `flow.PhiloxNoise` (not advanced: pass `philox.step()` next time) or an int seed.
        Returns x, or (x, eps if return_eps, log_prob if return_log_prob) with log_prob = log p(x) under the prior
        (= `log_prob(x)[2]`, without the second pass).  With grad enabled and parameters that require grad, x and log_prob are
        differentiable w.r.t. the parameters through the reverse bridge (eps is a constant); otherwise nothing is recorded."""
        params = self._param_list()
        self._require_gpu(params)
        rng = philox if isinstance(philox, flow.PhiloxNoise) else flow.PhiloxNoise(int(philox))
        n, temperature = int(n), float(temperature)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            holder = _Upstream()
            token = _ParamGate.apply(self, holder, *params)
            x, _, eps, ll = _FlowSampleFn.apply(self, holder, token, n, rng, temperature)
        else:
            x, _, eps, ll = flow.sample(self._plan(), n, rng, temperature=temperature, want_eps=return_eps, want_ll=return_log_prob)
        if not (return_eps or return_log_prob):
            return x
        return (x,) + ((eps,) if return_eps else ()) + ((ll,) if return_log_prob else ())

    # ---- fused extras (not in the reference; train.py:316-323 collapsed into two launches) ---------
    def log_prob(self, z, stats=None):
        """(z1, logdet, ll) with ll = -0.5*sum z1^2 + log(2*pi) + logdet (train.py:317-319), one launch.
        stats: optional buffer from `flow.new_stats()` (or a `PipelinedStatsReducer` row): the launch also leaves
        [sum ll, sum logdet, rows] in stats[4:7] (train.py:320 -- what a row-sharded evaluation all-reduces)."""
        z1, logdet, ll, _ = flow.forward(self._plan(), z.detach().contiguous(), None, want_ll=True, stats=stats)
        return z1, logdet, ll

    def log_prob_and_grad(self, z, scale=-1.0):
        """ll and d(scale * sum ll)/dz (train.py:320-323 uses scale = -1), two launches."""
        plan = self._plan()
        act = flow.new_act_saved(plan, z.shape[0], z.device)
        z1, logdet, ll, saved = flow.forward(plan, z.detach().contiguous(), None, want_ll=True, save_for_backward=True,
                                             act_saved=act)
        g = flow.backward_z(plan, z1, saved, ll_scale=scale, act_saved=act)
        return ll, g

    def langevin_step(self, z, grad_g=None, noise=None, step_size=0.1, inplace=False, reuse_buffers=False):
        """z <- z - 0.5 s^2 (grad_g + d(-sum ll)/dz) + s*noise (train.py:316-326), flow part fused into two launches.
        noise: None, a tensor of N(0,1) draws, or a `flow.PhiloxNoise` (drawn inside the kernel).
        Returns (z_new, ll_of_input_z, |grad_f| per row, |grad_g| per row or None)."""
        if isinstance(noise, torch.Tensor):
            noise = noise.detach().contiguous()
        return flow.langevin_step(self._plan(), z.detach().contiguous(),
                                  None if grad_g is None else grad_g.detach().contiguous(), noise, step_size,
                                  inplace=inplace, reuse_buffers=reuse_buffers)

    def mala_step(self, z_prop, grad_g=None, energy_g=None, state=None, noise=None, step_size=0.1, *, init=False, uniform=None,
                  propose=True, inplace=False, reuse_buffers=False):
        """One Metropolis-adjusted Langevin call at the proposal z_prop against the kept chain `state` (`flow.mala_step`: the
        forward at z_prop, then the backward that decides, updates the state and proposes again).
        Returns (z_next or None, accepted, log_alpha, ll_prop)."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.mala_step(self._plan(), det(z_prop), det(grad_g), det(energy_g), state, det(noise), step_size, init=init,
                              uniform=det(uniform), propose=propose, inplace=inplace, reuse_buffers=reuse_buffers)

    def hmc_step(self, z_prop, grad_g=None, energy_g=None, state=None, noise=None, step_size=0.1, *, phase="end", uniform=None,
                 propose=True, inplace=False, reuse_buffers=False):
        """One Hamiltonian Monte Carlo call at the point z_prop of a trajectory against the kept chain `state` (`flow.hmc_step`:
        the forward at z_prop, then the backward with the leapfrog tail; phase "init", "inner" or "end").
        Returns (z_next or None, accepted, log_alpha, ll_prop); accepted and log_alpha are None for an inner call."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.hmc_step(self._plan(), det(z_prop), det(grad_g), det(energy_g), state, det(noise), step_size, phase=phase,
                             uniform=det(uniform), propose=propose, inplace=inplace, reuse_buffers=reuse_buffers)

    def reverse_mala_step(self, eps_prop, z_saved, act_saved, grad_g=None, energy_g=None, state=None, noise=None, step_size=0.1, *,
                          init=False, uniform=None, propose=True, inplace=False, reuse_buffers=False):
        """One Metropolis-adjusted Langevin call in the base space at the proposal eps_prop against the kept chain `state`
        (`flow.reverse_mala_step`: ONE launch on the stash of the reverse at eps_prop; the caller's generator ran in between).
        Returns (eps_next or None, accepted, log_alpha)."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.reverse_mala_step(self._plan(), det(eps_prop), det(z_saved), det(act_saved), det(grad_g), det(energy_g), state,
                                      det(noise), step_size, init=init, uniform=det(uniform), propose=propose, inplace=inplace,
                                      reuse_buffers=reuse_buffers)

    def reverse_hmc_step(self, eps_prop, z_saved, act_saved, grad_g=None, energy_g=None, state=None, noise=None, step_size=0.1, *,
                         phase="end", uniform=None, propose=True, inplace=False, reuse_buffers=False):
        """One Hamiltonian Monte Carlo call in the base space at the point eps_prop of a trajectory against the kept chain `state`
        (`flow.reverse_hmc_step`: ONE launch on the stash of the reverse at eps_prop, the leapfrog tail as its output section; phase
        "init", "inner" or "end"; the caller's generator ran in between).
        Returns (eps_next or None, accepted, log_alpha); accepted and log_alpha are None for an inner call."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.reverse_hmc_step(self._plan(), det(eps_prop), det(z_saved), det(act_saved), det(grad_g), det(energy_g), state,
                                     det(noise), step_size, phase=phase, uniform=det(uniform), propose=propose, inplace=inplace,
                                     reuse_buffers=reuse_buffers)

    def hmc_step_rows(self, z_prop, grad_g=None, energy_g=None, state=None, noise=None, steps=None, *, phase="end", uniform=None,
                      propose=True, inplace=False, reuse_buffers=False, adapt=None):
        """`hmc_step` with a step per row (`flow.hmc_step_rows`; steps: a `flow.HmcRowSteps`); adapt="update" / "last" on an end
        call adapts the rows' steps by dual averaging inside the kernel.  Returns what `hmc_step` returns."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.hmc_step_rows(self._plan(), det(z_prop), det(grad_g), det(energy_g), state, det(noise), steps, phase=phase,
                                  uniform=det(uniform), propose=propose, inplace=inplace, reuse_buffers=reuse_buffers, adapt=adapt)

    def reverse_hmc_step_rows(self, eps_prop, z_saved, act_saved, grad_g=None, energy_g=None, state=None, noise=None, steps=None, *,
                              phase="end", uniform=None, propose=True, inplace=False, reuse_buffers=False, adapt=None):
        """`reverse_hmc_step` with a step per row (`flow.reverse_hmc_step_rows`; steps: a `flow.HmcRowSteps`); adapt="update" /
        "last" on an end call adapts the rows' steps by dual averaging inside the kernel.  Returns what `reverse_hmc_step` returns."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.reverse_hmc_step_rows(self._plan(), det(eps_prop), det(z_saved), det(act_saved), det(grad_g), det(energy_g), state,
                                          det(noise), steps, phase=phase, uniform=det(uniform), propose=propose, inplace=inplace,
                                          reuse_buffers=reuse_buffers, adapt=adapt)

    def hmc_step_metric(self, z_prop, grad_g=None, energy_g=None, state=None, noise=None, steps=None, metric=None, *, phase="end",
                        uniform=None, propose=True, inplace=False, reuse_buffers=False, adapt=None, window=None):
        """`hmc_step_rows` with a diagonal metric per row (`flow.hmc_step_metric`; metric: a `flow.HmcRowMetric`); window="fold" /
        "close" on an end call folds the decided state into the row's warm-up window / closes it.  Returns what `hmc_step` returns."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.hmc_step_metric(self._plan(), det(z_prop), det(grad_g), det(energy_g), state, det(noise), steps, metric, phase=phase,
                                    uniform=det(uniform), propose=propose, inplace=inplace, reuse_buffers=reuse_buffers, adapt=adapt,
                                    window=window)

    def reverse_hmc_step_metric(self, eps_prop, z_saved, act_saved, grad_g=None, energy_g=None, state=None, noise=None, steps=None,
                                metric=None, *, phase="end", uniform=None, propose=True, inplace=False, reuse_buffers=False, adapt=None,
                                window=None):
        """`reverse_hmc_step_rows` with a diagonal metric per row (`flow.reverse_hmc_step_metric`; metric: a `flow.HmcRowMetric`);
        window as `hmc_step_metric`'s.  Returns what `reverse_hmc_step` returns."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.reverse_hmc_step_metric(self._plan(), det(eps_prop), det(z_saved), det(act_saved), det(grad_g), det(energy_g), state,
                                            det(noise), steps, metric, phase=phase, uniform=det(uniform), propose=propose,
                                            inplace=inplace, reuse_buffers=reuse_buffers, adapt=adapt, window=window)

    def hmc_step_tempered(self, z_prop, grad_g=None, energy_g=None, state=None, noise=None, steps=None, metric=None, temper=None, *,
                          phase="end", uniform=None, propose=True, inplace=False, reuse_buffers=False, adapt=None, window=None,
                          anneal=None):
        """`hmc_step_metric` with a likelihood temperature per row (`flow.hmc_step_tempered`; temper: a `flow.HmcRowTemper`);
        anneal = a (B) tensor of the next beta on an init or end call weighs the decided state and re-tempers it inside the kernel.
        Returns what `hmc_step` returns."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.hmc_step_tempered(self._plan(), det(z_prop), det(grad_g), det(energy_g), state, det(noise), steps, metric, temper,
                                      phase=phase, uniform=det(uniform), propose=propose, inplace=inplace, reuse_buffers=reuse_buffers,
                                      adapt=adapt, window=window, anneal=det(anneal))

    def reverse_hmc_step_tempered(self, eps_prop, z_saved, act_saved, grad_g=None, energy_g=None, state=None, noise=None, steps=None,
                                  metric=None, temper=None, *, phase="end", uniform=None, propose=True, inplace=False,
                                  reuse_buffers=False, adapt=None, window=None, anneal=None):
        """`reverse_hmc_step_metric` with a likelihood temperature per row (`flow.reverse_hmc_step_tempered`; temper: a
        `flow.HmcRowTemper`); anneal as `hmc_step_tempered`'s.  Returns what `reverse_hmc_step` returns."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.reverse_hmc_step_tempered(self._plan(), det(eps_prop), det(z_saved), det(act_saved), det(grad_g), det(energy_g),
                                              state, det(noise), steps, metric, temper, phase=phase, uniform=det(uniform),
                                              propose=propose, inplace=inplace, reuse_buffers=reuse_buffers, adapt=adapt, window=window,
                                              anneal=det(anneal))

    def hmc_step_exchange(self, z_prop, grad_g=None, energy_g=None, state=None, noise=None, steps=None, metric=None, temper=None, *,
                          phase="end", uniform=None, propose=True, inplace=False, reuse_buffers=False, adapt=None, window=None,
                          anneal=None, swap=None, ladder=0, swap_uniform=None):
        """`hmc_step_tempered` with a replica-exchange move between the rows of a ladder (`flow.hmc_step_exchange`): swap = "even" or
        "odd" on an end call exchanges the states of paired rungs inside the kernel.  Returns what `hmc_step` returns plus
        (swapped, log_swap)."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.hmc_step_exchange(self._plan(), det(z_prop), det(grad_g), det(energy_g), state, det(noise), steps, metric, temper,
                                      phase=phase, uniform=det(uniform), propose=propose, inplace=inplace, reuse_buffers=reuse_buffers,
                                      adapt=adapt, window=window, anneal=det(anneal), swap=swap, ladder=ladder,
                                      swap_uniform=det(swap_uniform))

    def reverse_hmc_step_exchange(self, eps_prop, z_saved, act_saved, grad_g=None, energy_g=None, state=None, noise=None, steps=None,
                                  metric=None, temper=None, *, phase="end", uniform=None, propose=True, inplace=False,
                                  reuse_buffers=False, adapt=None, window=None, anneal=None, swap=None, ladder=0, swap_uniform=None):
        """`reverse_hmc_step_tempered` with a replica-exchange move between the rows of a ladder (`flow.reverse_hmc_step_exchange`).
        Returns what `reverse_hmc_step` returns plus (swapped, log_swap)."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.reverse_hmc_step_exchange(self._plan(), det(eps_prop), det(z_saved), det(act_saved), det(grad_g), det(energy_g),
                                              state, det(noise), steps, metric, temper, phase=phase, uniform=det(uniform),
                                              propose=propose, inplace=inplace, reuse_buffers=reuse_buffers, adapt=adapt, window=window,
                                              anneal=det(anneal), swap=swap, ladder=ladder, swap_uniform=det(swap_uniform))

    def hmc_step_resample(self, z_prop, grad_g=None, energy_g=None, state=None, noise=None, steps=None, metric=None, temper=None, *,
                          phase="end", uniform=None, propose=True, inplace=False, reuse_buffers=False, adapt=None, window=None,
                          anneal=None, resample=None, ess_threshold=0.5, resample_uniform=None):
        """`hmc_step_tempered` with a resampling move between the rows of a group (`flow.hmc_step_resample`): resample = P on an
        annealing end call resamples, inside the kernel, every group of P rows whose effective sample size is below
        ess_threshold * P.  Returns what `hmc_step` returns plus (ancestor, ess)."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.hmc_step_resample(self._plan(), det(z_prop), det(grad_g), det(energy_g), state, det(noise), steps, metric, temper,
                                      phase=phase, uniform=det(uniform), propose=propose, inplace=inplace, reuse_buffers=reuse_buffers,
                                      adapt=adapt, window=window, anneal=det(anneal), resample=resample, ess_threshold=ess_threshold,
                                      resample_uniform=det(resample_uniform))

    def reverse_hmc_step_resample(self, eps_prop, z_saved, act_saved, grad_g=None, energy_g=None, state=None, noise=None, steps=None,
                                  metric=None, temper=None, *, phase="end", uniform=None, propose=True, inplace=False,
                                  reuse_buffers=False, adapt=None, window=None, anneal=None, resample=None, ess_threshold=0.5,
                                  resample_uniform=None):
        """`reverse_hmc_step_tempered` with a resampling move between the rows of a group (`flow.reverse_hmc_step_resample`).
        Returns what `reverse_hmc_step` returns plus (ancestor, ess)."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.reverse_hmc_step_resample(self._plan(), det(eps_prop), det(z_saved), det(act_saved), det(grad_g), det(energy_g),
                                              state, det(noise), steps, metric, temper, phase=phase, uniform=det(uniform),
                                              propose=propose, inplace=inplace, reuse_buffers=reuse_buffers, adapt=adapt, window=window,
                                              anneal=det(anneal), resample=resample, ess_threshold=ess_threshold,
                                              resample_uniform=det(resample_uniform))

    def hmc_step_schedule(self, z_prop, grad_g=None, energy_g=None, state=None, noise=None, steps=None, metric=None, temper=None, *,
                          phase="end", uniform=None, propose=True, inplace=False, reuse_buffers=False, adapt=None, window=None,
                          anneal=None, resample=None, ess_threshold=0.5, resample_uniform=None, schedule=None, cess_target=0.95,
                          min_step=0.0):
        """`hmc_step_resample` with the groups' next temperature searched inside the kernel (`flow.hmc_step_schedule`): schedule = P
        on an annealing init or end call makes anneal the ceiling and steps every group of P rows to where the conditional effective
        sample size of its incremental weights is cess_target * P, by at least min_step.  Returns what `hmc_step_resample` returns."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.hmc_step_schedule(self._plan(), det(z_prop), det(grad_g), det(energy_g), state, det(noise), steps, metric, temper,
                                      phase=phase, uniform=det(uniform), propose=propose, inplace=inplace, reuse_buffers=reuse_buffers,
                                      adapt=adapt, window=window, anneal=det(anneal), resample=resample, ess_threshold=ess_threshold,
                                      resample_uniform=det(resample_uniform), schedule=schedule, cess_target=cess_target,
                                      min_step=min_step)

    def reverse_hmc_step_schedule(self, eps_prop, z_saved, act_saved, grad_g=None, energy_g=None, state=None, noise=None, steps=None,
                                  metric=None, temper=None, *, phase="end", uniform=None, propose=True, inplace=False,
                                  reuse_buffers=False, adapt=None, window=None, anneal=None, resample=None, ess_threshold=0.5,
                                  resample_uniform=None, schedule=None, cess_target=0.95, min_step=0.0):
        """`reverse_hmc_step_resample` with the groups' next temperature searched inside the kernel
        (`flow.reverse_hmc_step_schedule`).  Returns what `reverse_hmc_step_resample` returns."""
        det = lambda t: t.detach().contiguous() if isinstance(t, torch.Tensor) else t
        return flow.reverse_hmc_step_schedule(self._plan(), det(eps_prop), det(z_saved), det(act_saved), det(grad_g), det(energy_g),
                                              state, det(noise), steps, metric, temper, phase=phase, uniform=det(uniform),
                                              propose=propose, inplace=inplace, reuse_buffers=reuse_buffers, adapt=adapt, window=window,
                                              anneal=det(anneal), resample=resample, ess_threshold=ess_threshold,
                                              resample_uniform=det(resample_uniform), schedule=schedule, cess_target=cess_target,
                                              min_step=min_step)

    def mle_grads(self, z, accumulate: bool = False, max_norm: Optional[float] = None, reuse_buffers: bool = False):
        """Fused flow-MLE gradients (train.py:404-411): loss_f = -mean_b ll(z_b) and d loss_f / d theta written to
        `.grad` of the 60 live tensors -- forward (ll summed in-kernel), dump backward, batch contraction, unfold:
        5 launches and no autograd graph.  max_norm: clip the global gradient norm (train.py:413-414
        `clip_grad_norm_`) on the one flat buffer the gradients are views of (3 launches instead of a foreach over
        60 tensors; only without `accumulate`).  With `deterministic_grads` the gradients are bit-reproducible.
        reuse_buffers: the gradient tensors are the same objects every call,
        overwritten in place (`flow.backward_params`): for loops that consume `.grad` before the next call.
        Returns loss_f as a 0-dim device tensor (no host sync)."""
        plan = self._plan()
        z = z.detach().contiguous()
        B = z.shape[0]
        if B == 0:
            raise LsnfError("mle_grads needs a non-empty batch")
        stats = flow.new_stats(z.device)
        fast = flow.params_fast_path()         # forward keeps the stash + writes h1 / h2 for the contraction: nothing is recomputed
        bufs = plan.__dict__.get("_mle_buffers") if reuse_buffers else None
        det = bool(self.deterministic_grads)
        bkey = (B, z.device, torch.cuda.current_stream(z.device).cuda_stream, det)
        if fast and (bufs is None or bufs[0] != bkey):
            bufs = (bkey, flow.new_act_saved(plan, B, z.device), flow.new_params_workspace(plan, B, z.device, deterministic=det))
            if reuse_buffers:
                plan.__dict__["_mle_buffers"] = bufs
        act, ws = (bufs[1], bufs[2]) if fast else (None, None)
        if fast and z.data_ptr() % 16:
            z = z.clone()        # the fast path wants 16-byte aligned rows at large B (lsnf_forward, params_workspace)
        z1, _, _, saved = flow.forward(plan, z, None, want_ll=False, save_for_backward=True, stats=stats, act_saved=act, params_ws=ws)
        params = self._param_list()
        grads, flat = flow.backward_params(plan, params, z, z1, saved, ll_scale=-1.0 / B, want_flat=True,
                                           reuse_buffers=reuse_buffers and not accumulate, act_saved=act, workspace=ws,
                                           deterministic=det)
        if max_norm is not None:
            if accumulate:
                raise LsnfError("max_norm clips the gradients of this call only: not with accumulate=True")
            flat.mul_(torch.clamp(float(max_norm) / (flat.norm() + 1e-6), max=1.0))   # torch's clip_grad_norm_ formula
        for p, g in zip(params, grads):
            if not p.requires_grad or p.grad is g:
                continue
            p.grad = g if (p.grad is None or not accumulate) else p.grad + g
        return (stats[4] * (-1.0 / B)).to(torch.float32)

    def mle_step(self, z, optimizer, reuse_buffers: bool = True):
        """One whole flow-MLE update (train.py:404-415) without stock-PyTorch launches: `mle_grads` (no clip of its own),
        `optimizer.step()` -- a `FlowAdam`, which owns the clip (its max_norm) -- and the prepared weights re-derived from the
        written values into the cached plan buffer, so the next call on the module finds its plan current.  Returns loss_f
        (of the parameters BEFORE the update) as a 0-dim device tensor; nothing synchronises."""
        from .optim import FlowAdam
        if not isinstance(optimizer, FlowAdam) or optimizer._netF is not self:
            raise LsnfError("mle_step needs this module's lsnf_amd.FlowAdam; with any other optimizer use "
                            "langevin.flow_mle_step (mle_grads + optimizer.step())")
        loss_f = self.mle_grads(z, reuse_buffers=reuse_buffers)
        optimizer.step()
        self._plan()          # lsnf_prepare into the cached plan buffer; the plan key becomes the new versions
        return loss_f

"""Restatement of the variants of the flow's optimizer step -- `clip_grad_norm_` followed by torch.optim.Adam / AdamW with amsgrad,
maximize and decoupled weight decay, a skip of steps whose gradient norm is not finite, and an exponential moving average of
the parameters -- on lists of tensors, in the dtype asked for (float64: the reference the kernels are held to; float32: an
independent fp32 leg).  Formulas as include/lsnf_flow.h states them (lsnf_adam_step_ex); no torch.optim code is used."""
import math

import torch

from adam_restated import global_norm


def clip_adam_variants(params, grad_steps, *, lr, betas, eps=1e-8, weight_decay=0.0, max_norm=None, amsgrad=False, maximize=False,
                       decoupled=False, ema_decay=None, skip_nonfinite=False, dtype=torch.float64):
    """Runs len(grad_steps) steps from a fresh state.  params: list of tensors; grad_steps: per step a list of gradients (None =
    that tensor is skipped in that step); lr: a float, or one float per step.  Returns a dict: p, m, v, vmax (None without
    amsgrad), ema (None without ema_decay) as lists of `dtype` tensors, norms (the pre-clip global norm of every step, float64),
    step (the steps that were taken) and skipped (those that were not).
    The average is taken of the parameters as this restatement holds them (in `dtype`); a kernel that stores fp32 parameters
    averages the stored values, so its average is compared with `ema_of` over the values it stored."""
    b1, b2 = betas
    p = [t.detach().to(dtype).clone() for t in params]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    vmax = [torch.zeros_like(t) for t in p] if amsgrad else None
    ema = [torch.zeros_like(t) for t in p] if ema_decay is not None else None
    norms, step, skipped = [], 0, 0
    for k, grads in enumerate(grad_steps):
        lr_k = lr[k] if isinstance(lr, (list, tuple)) else lr
        norm = float(global_norm(grads))
        norms.append(norm)
        if skip_nonfinite and not math.isfinite(norm):
            skipped += 1
            continue
        step += 1
        coef = None if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        for i, g in enumerate(grads):
            p_before = p[i]
            if g is not None:
                g = g.to(dtype)
                if maximize:
                    g = -g
                if coef is not None:
                    g = coef * g
                pk = p[i]
                if weight_decay != 0:
                    if decoupled:
                        pk = pk * (1.0 - lr_k * weight_decay)
                    else:
                        g = g + weight_decay * pk
                m[i] = m[i] + (1.0 - b1) * (g - m[i])
                v[i] = b2 * v[i] + (1.0 - b2) * g * g
                root = v[i]
                if amsgrad:
                    root = vmax[i] = torch.maximum(vmax[i], v[i])
                p[i] = pk - (lr_k / bc1) * m[i] / (root.sqrt() / math.sqrt(bc2) + eps)
            if ema is not None:
                e_prev = p_before if step == 1 else ema[i]
                ema[i] = e_prev + (1.0 - ema_decay) * (p[i] - e_prev)
    return dict(p=p, m=m, v=v, vmax=vmax, ema=ema, norms=norms, step=step, skipped=skipped)


def ema_of(snapshots, ema_decay):
    """The float64 average of a list of parameter snapshots: snapshots[0] = the parameters before the first step (where the
    average starts), snapshots[k] = the parameters as step k stored them.  Each a list of tensors."""
    e = [t.detach().double().clone() for t in snapshots[0]]
    for snap in snapshots[1:]:
        e = [a + (1.0 - ema_decay) * (t.detach().double() - a) for a, t in zip(e, snap)]
    return e

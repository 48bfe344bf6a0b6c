"""Restatement of the flow's optimizer step -- `clip_grad_norm_` followed by torch.optim.Adam (non-amsgrad, maximize=False, L2
weight decay; PyTorch's _single_tensor_adam) -- on lists of tensors, in the dtype asked for (float64: the reference the
kernels are held to; float32: an independent fp32 leg with its own operation order).  Formulas as include/lsnf_flow.h states
them; no torch.optim code is used."""
import math

import torch


def global_norm(grads, dtype=torch.float64):
    """sqrt(sum g^2) over the gradients that are not None, accumulated in `dtype`."""
    tot = torch.zeros((), dtype=dtype)
    for g in grads:
        if g is not None:
            tot = tot + (g.to(dtype) ** 2).sum()
    return tot.sqrt()


def clip_adam(params, grad_steps, *, lr, betas, eps=1e-8, weight_decay=0.0, max_norm=None, dtype=torch.float64,
              m=None, v=None, step0=0):
    """Runs len(grad_steps) steps.  params: list of tensors; grad_steps: per step a list of gradients (None = that tensor is
    skipped in that step); lr: a float, or one float per step; m / v / step0: state to continue from (default: fresh).
    Returns (p, m, v, norms): lists of `dtype` tensors and the pre-clip global norm of every step (float64)."""
    b1, b2 = betas
    p = [t.detach().to(dtype).clone() for t in params]
    m = [torch.zeros_like(t) for t in p] if m is None else [t.detach().to(dtype).clone() for t in m]
    v = [torch.zeros_like(t) for t in p] if v is None else [t.detach().to(dtype).clone() for t in v]
    norms = []
    for k, grads in enumerate(grad_steps):
        step = step0 + k + 1
        lr_k = lr[k] if isinstance(lr, (list, tuple)) else lr
        norm = float(global_norm(grads))
        norms.append(norm)
        coef = None if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = g.to(dtype)
            if coef is not None:
                g = coef * g
            if weight_decay != 0:
                g = g + weight_decay * p[i]
            m[i] = m[i] + (1.0 - b1) * (g - m[i])
            v[i] = b2 * v[i] + (1.0 - b2) * g * g
            p[i] = p[i] - (lr_k / bc1) * m[i] / (v[i].sqrt() / math.sqrt(bc2) + eps)
    return p, m, v, norms

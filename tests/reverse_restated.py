"""The backward of the flow's REVERSE pass, restated on the oracle's building blocks (shared by test_reverse_autograd_cpu.py
and test_gpu_reverse_autograd.py; not a test module).

With f the forward stack, x = f^-1(eps) and o_out = o_in - logdet_f(x), for upstream gradients g_x = dL/dx, g_o = dL/do_out:

  (1) g_eps = J_f(x)^-T (g_x - g_o grad_x logdet_f(x)) -- `reverse_backward_restated`: one pass over the blocks in FORWARD order,
      the recurrence lsnf_small3_rbwd.hip implements (T1, CB', B4, B3, B2 per block), in the dtype of its inputs;
  (2) dL/dtheta = d/dtheta [ -(f(x) . g_eps).sum() - (logdet_f(x) . g_o).sum() ] at fixed x (implicit-function theorem) --
      `params_via_forward`: what lsnf_backward_params computes for the FORWARD at x with g_z1 = -g_eps, g_logdet = -g_o.
"""
import torch

from oracle import flow_oracle as O


def live_keys(p):
    return sorted(k for k in p if O.is_live_param(k))


def reverse_loss_grads(p, eps, obj, g_x, g_o, dtype, want_params=False):
    """Autograd of O.flow_reverse in `dtype` at eps: L = (x * g_x).sum() + (o_out * g_o).sum(), o_out = -negobj.
    Returns (x, o_out, dL/deps, {key: dL/dtheta} or None)."""
    q = O.to_dtype(p, dtype)
    keys = live_keys(q) if want_params else []
    leaves = {k: q[k].clone().requires_grad_(True) for k in keys}
    q = {**q, **leaves}
    e = eps.to(dtype).clone().requires_grad_(True)
    x, negobj = O.flow_reverse(q, e, obj.to(dtype))
    loss = (x * g_x.to(dtype)).sum() + ((-negobj) * g_o.to(dtype)).sum()
    grads = torch.autograd.grad(loss, [e] + [leaves[k] for k in keys])
    return x.detach(), (-negobj).detach(), grads[0], (dict(zip(keys, grads[1:])) if want_params else None)


def forward64(p, x):
    """(f(x), logdet_f(x)) in float64."""
    xx = x.double()
    return O.flow_forward(O.to_dtype(p, torch.float64), xx, torch.zeros(xx.shape[0], dtype=torch.float64))


def reverse64(p, eps):
    ee = eps.double()
    return O.flow_reverse(O.to_dtype(p, torch.float64), ee, torch.zeros(ee.shape[0], dtype=torch.float64))[0]


def params_via_forward(p, x, g_eps, g_o, dtype):
    """Identity (2): the parameter gradients of the reverse from the FORWARD at the fixed point x."""
    q = O.to_dtype(p, dtype)
    keys = live_keys(q)
    leaves = {k: q[k].clone().requires_grad_(True) for k in keys}
    q = {**q, **leaves}
    xx = x.to(dtype)
    z1, logdet = O.flow_forward(q, xx, torch.zeros(xx.shape[0], dtype=dtype))
    loss = -(z1 * g_eps.to(dtype)).sum() - (logdet * g_o.to(dtype)).sum()
    return dict(zip(keys, torch.autograd.grad(loss, [leaves[k] for k in keys])))


def reverse_backward_restated(p, x, g_x, g_o):
    """Identity (1) as the recurrence over the blocks in forward order; every tensor in x's dtype."""
    dt = x.dtype
    q = O.to_dtype(p, dt)
    coupling = O.coupling_of(q)
    depth, nz = O.depth_of(q), x.shape[1]
    half = nz // 2
    e3 = lambda k: torch.exp(q[k] * 3.0)
    state, z = [], x
    ld = torch.zeros(x.shape[0], dtype=dt)
    for i in range(depth):              # the forward at x: per block sigma, the two ReLU masks and the output y2
        pre = O.block_prefix(i)
        v1 = torch.matmul(O.actnorm_fwd(z, q[pre + "actnorm.b"], q[pre + "actnorm.logs"]), q[pre + "invertible_1x1_conv.w"])[:, :half]
        a1 = O.actnorm_fwd(torch.matmul(v1, q[pre + "f.fc_1.w"]), q[pre + "f.fc_1.actnorm.b"], q[pre + "f.fc_1.actnorm.logs"])
        a2 = O.actnorm_fwd(torch.matmul(torch.relu(a1), q[pre + "f.fc_2.w"]), q[pre + "f.fc_2.actnorm.b"], q[pre + "f.fc_2.actnorm.logs"])
        h = O.mlp_f(q, pre, v1)
        sigma = torch.sigmoid(h[:, 1::2] + 2.0) if coupling else torch.ones_like(v1)
        z, ld = O.block_fwd(q, i, z, ld, coupling)
        state.append((sigma, a1 > 0, a2 > 0, z[:, half:]))
    g, go = g_x.to(dt), g_o.to(dt)
    for i in range(depth):
        pre = O.block_prefix(i)
        sigma, m1, m2, y2 = state[i]
        winv = torch.inverse(q[pre + "invertible_1x1_conv.w"].double()).to(dt) * torch.exp(-3.0 * q[pre + "actnorm.logs"])   # Winv'
        gv = torch.matmul(g, winv.t())                                                      # T1
        gv1, gv2 = gv[:, :half], gv[:, half:]
        gy2 = gv2 / sigma                                                                   # CB'
        gt = -gv2
        if coupling:
            gp = -(1.0 - sigma) * (gy2 * y2 + go[:, None])
            gh = torch.stack([gt, gp], dim=2).reshape(x.shape[0], nz)                       # columns 2f: shift, 2f+1: pre-sigmoid
        else:
            gh = gt
        ga2 = torch.matmul(gh * e3(pre + "f.fc_zeros.logs"), q[pre + "f.fc_zeros.w"].t()) * m2            # B4
        ga1 = torch.matmul(ga2 * e3(pre + "f.fc_2.actnorm.logs"), q[pre + "f.fc_2.w"].t()) * m1           # B3
        gy1 = gv1 + torch.matmul(ga1 * e3(pre + "f.fc_1.actnorm.logs"), q[pre + "f.fc_1.w"].t())          # B2
        g = torch.cat([gy1, gy2], 1)
    return g


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()

"""GPU: autograd through the reverse (sampling) pass -- lsnf_reverse_backward_z (lsnf_small3_rbwd.hip) and the module's
differentiable `netF(eps, obj, reverse=True)` against float64 autograd of oracle/flow_oracle.py.

Tolerances: every comparison allows max(the forward direction's gate, 3 x the oracle's OWN fp32-vs-fp64 error for that quantity on
that input, computed here on the CPU): an inverse amplifies fp32 rounding in any implementation (the factor 3 is the one
`inverse_tolerance` of test_gpu_reverse_backward.py grants the reverse).  Gates of the forward direction: dz 1e-5 rel-L2 over rows
with relu_margin > 2e-6 (the other rows within 2 %), dtheta 2e-5 per tensor on kink-free batches, 1e-4 on fixtures.  Every case
prints `measured / allowed / oracle-fp32` (run with -s to collect the table)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden
from oracle import flow_oracle as O
import reverse_restated as R

pytestmark = pytest.mark.gpu
KINK = 2e-6
ILL = ("c3_nz128_w64_B65_trained02", "c5_nz100_w128_B33_trained02", "c3_nz128_w64_B7_trained_s3")   # covered at kernel level only


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


def geometry(p):
    pre = O.block_prefix(0)
    return p[pre + "actnorm.logs"].shape[1], p[pre + "f.fc_1.w"].shape[1], O.depth_of(p), O.coupling_of(p)


def make_plan(lsnf, p, dev):
    nz, w, d, c = geometry(p)
    return lsnf.prepare(lsnf.params_from_state_dict(p, d, dev), nz, w, d, c)


def additive(p):
    """The oracle's synthetic weights with the additive coupling's fc_zeros (nz/2 outputs, model.py:385)."""
    q = dict(p)
    for k in p:
        if ".f.fc_zeros." in k:
            q[k] = p[k][:, : p[k].shape[1] // 2].contiguous()
    return q


def fwd_stash(lsnf, plan, x):
    act = lsnf.flow.new_act_saved(plan, x.shape[0], x.device)
    act.fill_(float("nan"))                 # every word the kernel reads of a live row must have been written by the forward
    z1, _, _, saved = lsnf.forward(plan, x, want_ll=False, save_for_backward=True, act_saved=act)
    return z1, saved, act


def rbwd_at(lsnf, plan, x, gx, go):
    z1, saved, act = fwd_stash(lsnf, plan, x)
    return lsnf.flow.reverse_backward_z(plan, z1, saved, act, gx, go)


def report(what, got, allowed, own):
    print(f"[reverse-autograd] {what}: measured {got:.3e} allowed {allowed:.3e} oracle-fp32 {own:.3e}")


def seeded(B, nz, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, nz, generator=gen), torch.randn(B, generator=gen), torch.randn(B, generator=gen)


# ---------------------------------------------------------------------------------------------
# 1. kernel level, the point x given
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names())
def test_kernel_at_given_x_matches_float64_oracle(lsnf, kernels, gpu_device, name):
    p, g = load_golden(name)
    x = torch.from_numpy(g["z"])
    B, nz = x.shape
    gx, go, _ = seeded(B, nz, 11)
    eps64 = R.forward64(p, x)[0]
    _, _, ref, _ = R.reverse_loss_grads(p, eps64, torch.zeros(B), gx, go, torch.float64)
    own32 = R.reverse_backward_restated(p, x, gx, go)          # the same formulation in the oracle's fp32
    ok = O.relu_margin(p, x) > KINK
    assert int((~ok).sum()) <= 2
    own = R.rel_l2(own32[ok], ref[ok])
    tol = max(1e-5, 3.0 * own)
    plan = make_plan(lsnf, p, gpu_device)
    got = rbwd_at(lsnf, plan, x.to(gpu_device), gx.to(gpu_device), go.to(gpu_device)).cpu()
    err = R.rel_l2(got[ok], ref[ok])
    report(f"kernel {name} [{kernels}] kink-rows {int((~ok).sum())}", err, tol, own)
    assert err <= tol
    assert (got.double() - ref).abs().max().item() <= 2e-2 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("name", golden_names())
def test_kernel_call_forms(lsnf, gpu_device, name):
    """NULL upstream gradients == explicit zeros (bits), linearity, the stash of lsnf_restash, g_z_in aliasing g_x, tensors at a
    4-byte offset, and the LSNF_E_ARG cases."""
    p, g = load_golden(name)
    dev = gpu_device
    x = torch.from_numpy(g["z"]).to(dev)
    B, nz = x.shape
    nzw = geometry(p)
    gx, go, _ = (t.to(dev) for t in seeded(B, nz, 12))
    plan = make_plan(lsnf, p, dev)
    f = lsnf.flow
    z1, saved, act = fwd_stash(lsnf, plan, x)
    base = f.reverse_backward_z(plan, z1, saved, act, gx, go)
    assert torch.isfinite(base).all()
    assert torch.equal(f.reverse_backward_z(plan, z1, saved, act, None, go), f.reverse_backward_z(plan, z1, saved, act, torch.zeros_like(gx), go))
    assert torch.equal(f.reverse_backward_z(plan, z1, saved, act, gx, None), f.reverse_backward_z(plan, z1, saved, act, gx, torch.zeros_like(go)))
    assert torch.count_nonzero(f.reverse_backward_z(plan, z1, saved, act, None, None)) == 0
    two = f.reverse_backward_z(plan, z1, saved, act, 2 * gx, 2 * go)
    assert (two - 2 * base).abs().max().item() <= 1e-4 * base.abs().max().item()
    # the stash rebuilt from the block outputs
    lib = lsnf.load_library()
    act2 = f.new_act_saved(plan, B, dev)
    act2.fill_(float("nan"))
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    sp = torch.cuda.current_stream(dev).cuda_stream
    assert lib.lsnf_restash(ptr(plan.buf), *nzw, B, ptr(z1), ptr(saved), ptr(act2), sp) == 0
    assert torch.equal(f.reverse_backward_z(plan, z1, saved, act2, gx, go), base)
    # in place
    buf = gx.clone()
    assert f.reverse_backward_z(plan, z1, saved, act, buf, go, out=buf) is buf and torch.equal(buf, base)
    assert torch.equal(z1, fwd_stash(lsnf, plan, x)[0])                       # (inputs are never written)

    def off4(t):                                                             # the same values 4 bytes past a 16-byte boundary
        if t is None:
            return None
        b = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
        assert b.data_ptr() % 16 == 0
        v = b[1: 1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    out = off4(torch.zeros_like(gx))
    f.reverse_backward_z(plan, off4(z1), off4(saved), act, off4(gx), off4(go), out=out)
    assert torch.equal(out, base)
    # refused before anything is launched
    call = lambda zs, a: lib.lsnf_reverse_backward_z(ptr(plan.buf), *nzw, B, ptr(z1), ptr(zs), a, ptr(gx), ptr(go), ptr(out), sp)
    assert call(saved, None) == -1
    assert call(saved, ctypes.c_void_p(act.data_ptr() + 4)) == -1
    if nzw[2] > 1:
        assert call(None, ptr(act)) == -1
    torch.cuda.synchronize()
    assert torch.equal(out, base)
    with pytest.raises(lsnf.LsnfError):
        f.reverse_backward_z(plan, z1, saved, None, gx, go)
    with pytest.raises(lsnf.LsnfError):
        f.reverse_backward_z(plan, z1, saved, act[: act.numel() // 2], gx, go)
    with pytest.raises(lsnf.LsnfError):
        f.reverse_backward_z(plan, z1, saved, act, gx.cpu(), go)


# ---------------------------------------------------------------------------------------------
# 2. geometry and size sweep, kink-free
# ---------------------------------------------------------------------------------------------
def kinkfree_case(nz, w, depth, coupling, B):
    p = O.init_params(nz, w, depth, seed=3)
    if coupling == 0:
        p = additive(p)
    x, _ = O.smooth_batch(p, B, nz, seed=B)
    eps = R.forward64(p, x)[0].float()
    return p, eps


# (nz, width, depth, coupling, B): <1,1> / <2,2> / <2,4>; 16 / 32 / 64 rows per workgroup through the batch size (<= 4 096 / <= 8 192 /
# above; width 128 has no 64-row form); ragged last tiles; B = 1, 33; nz 2 / w 1; nz 126 / w 127; depth 1 and 16; additive; 20 000
SWEEP = [(8, 4, 5, 1, 1), (8, 4, 5, 1, 33), (2, 1, 3, 1, 37), (126, 127, 2, 1, 77), (64, 32, 1, 1, 100), (20, 12, 16, 1, 50),
         (20, 12, 5, 0, 33), (100, 64, 5, 0, 300), (128, 64, 5, 1, 100), (128, 64, 5, 1, 5000), (100, 128, 5, 1, 4200),
         (100, 128, 5, 1, 9001), (64, 32, 5, 1, 4000), (64, 32, 5, 1, 6000), (64, 32, 5, 1, 9000), (128, 64, 5, 1, 20000)]


@pytest.mark.parametrize("nz,w,depth,coupling,B", SWEEP)
def test_sweep_kinkfree_vs_float64_oracle(lsnf, gpu_device, nz, w, depth, coupling, B):
    p, eps = kinkfree_case(nz, w, depth, coupling, B)
    assert (O.relu_margin(p, R.reverse64(p, eps)) > 1e-5).all()            # a kink-free input of the REVERSE: no row is set aside
    gx, go, obj = seeded(B, nz, 100 + B)
    _, _, ref, _ = R.reverse_loss_grads(p, eps, obj, gx, go, torch.float64)
    _, _, g32, _ = R.reverse_loss_grads(p, eps, obj, gx, go, torch.float32)
    own = R.rel_l2(g32, ref)
    tol = max(1e-5, 3.0 * own)
    plan = make_plan(lsnf, p, gpu_device)
    dev = gpu_device
    x, _ = lsnf.reverse(plan, eps.to(dev), obj.to(dev))
    got = rbwd_at(lsnf, plan, x, gx.to(dev), go.to(dev)).cpu()
    err = R.rel_l2(got, ref)
    report(f"sweep nz{nz} w{w} d{depth} c{coupling} B{B}", err, tol, own)
    assert err <= tol


def test_full_size_65536_properties(lsnf, gpu_device):
    """B = 65 536 (several rounds of workgroups): sampled rows against the oracle; every row bit-identical to the same row run in
    smaller batches that select the other workgroup shapes (stash by the latency forward in all of them); within 2e-6 of the
    gradient's maximum when the throughput forward wrote the stash; the adjoint identity over the whole batch."""
    nz, w, depth, B = 128, 64, 5, 65536
    dev = gpu_device
    f = lsnf.flow
    p = O.init_params(nz, w, depth, seed=3)
    plan = make_plan(lsnf, p, dev)
    idx = torch.arange(5, B, 4099)
    xs, _ = O.smooth_batch(p, len(idx), nz, seed=B)
    eps = torch.randn(B, nz, generator=torch.Generator().manual_seed(65))
    eps[idx] = R.forward64(p, xs)[0].float()                                  # the sampled rows are kink-free inputs of the reverse
    gx, go, obj = seeded(B, nz, 66)
    _, _, ref, _ = R.reverse_loss_grads(p, eps[idx], obj[idx], gx[idx], go[idx], torch.float64)
    x32, _, g32, _ = R.reverse_loss_grads(p, eps[idx], obj[idx], gx[idx], go[idx], torch.float32)
    own = R.rel_l2(g32, ref)
    gxd, god = gx.to(dev), go.to(dev)
    x, _ = lsnf.reverse(plan, eps.to(dev), obj.to(dev))
    assert f.set_math_mode(-1) == f.MATH_BF16X3
    # default dispatch: the THROUGHPUT forward writes the stash
    assert f.set_small_batch_max(-1) == 16384
    z1, saved, act = fwd_stash(lsnf, plan, x)
    g_thr = f.reverse_backward_z(plan, z1, saved, act, gxd, god)
    err = R.rel_l2(g_thr.cpu()[idx], ref)
    report("65536 sampled rows", err, max(1e-5, 3.0 * own), own)
    assert err <= max(1e-5, 3.0 * own)
    # adjoint identity: the forward's backward applied to (g_y, g_o) gives g_x back
    back = f.backward_z(plan, z1, saved, g_thr, god, act_saved=act)
    res = R.rel_l2(back, gxd)
    xx = x32.clone().requires_grad_(True)
    z1o, ldo = O.flow_forward(p, xx, torch.zeros(len(idx)))
    (back32,) = torch.autograd.grad((z1o * g32).sum() + (ldo * go[idx]).sum(), xx)
    own_res = R.rel_l2(back32, gx[idx])
    report("65536 adjoint identity", res, max(2e-5, 3.0 * own_res), own_res)
    assert res <= max(2e-5, 3.0 * own_res)
    prev = f.set_small_batch_max(1 << 30)                                     # the LATENCY forward writes every stash below
    try:
        z1l, savedl, actl = fwd_stash(lsnf, plan, x)
        g_lat = f.reverse_backward_z(plan, z1l, savedl, actl, gxd, god)
        for n in (16000, 8000, 100):                                          # 64 / 32 / 16 rows per workgroup
            sub = rbwd_at(lsnf, plan, x[:n].contiguous(), gxd[:n].contiguous(), god[:n].contiguous())
            assert torch.equal(sub, g_lat[:n]), n
    finally:
        f.set_small_batch_max(prev)
    gmax = g_lat.abs().max().item()
    d = (g_thr - g_lat).abs().max().item()
    report("65536 stash of the throughput vs the latency forward (of max)", d / gmax, 2e-6, 0.0)
    assert d <= 2e-6 * gmax


# ---------------------------------------------------------------------------------------------
# 3. module level, full autograd
# ---------------------------------------------------------------------------------------------
def hps_of(p):
    nz, w, d, c = geometry(p)
    return types.SimpleNamespace(f_n_levels=1, f_depth=d, f_flow_permutation=2, f_width=w, f_flow_coupling=c), nz


def module_of(lsnf, p, dev):
    h, nz = hps_of(p)
    net = lsnf._netF(h, nz)
    net.load_state_dict(p, strict=True)
    return net.to(dev)


def param_keys(lsnf, depth):
    return [O.block_prefix(i) + k for i in range(depth) for k in lsnf.flow.BLOCK_PARAM_KEYS]


def module_case(lsnf, dev, p, eps, fixture, label):
    B, nz = eps.shape
    depth = O.depth_of(p)
    cx, co, obj = seeded(B, nz, 200 + B)
    gx, go = cx / B, -co / B                                                  # loss = (x cx).sum()/B + (negobj co).mean(), negobj = -o_out
    _, _, ref, pref = R.reverse_loss_grads(p, eps, obj, gx, go, torch.float64, want_params=True)
    _, _, g32, p32 = R.reverse_loss_grads(p, eps, obj, gx, go, torch.float32, want_params=True)
    net = module_of(lsnf, p, dev)
    e = eps.to(dev).requires_grad_()
    o = obj.to(dev).requires_grad_()
    keep = e.detach().clone()
    x, negobj = net(e, o, reverse=True, return_obj=True)
    with torch.no_grad():
        x0, negobj0 = net(e, o, reverse=True, return_obj=True)
    assert torch.equal(x, x0) and torch.equal(negobj, negobj0) and torch.equal(e.detach(), keep)
    loss = (x * cx.to(dev)).sum() / B + (negobj * co.to(dev)).mean()
    loss.backward()
    # dL/d objective is dL/d objective_out passed through: exactly -co/B as PyTorch itself forms it for a plain tensor
    t = torch.zeros(B, device=dev, requires_grad=True)
    ((-t) * co.to(dev)).mean().backward()
    assert torch.equal(o.grad, t.grad) and (o.grad.cpu() + co / B).abs().max().item() <= 1e-7 * co.abs().max().item() / B
    own = R.rel_l2(g32, ref)
    err = R.rel_l2(e.grad.cpu(), ref)
    report(f"module {label} d eps", err, max(1e-5, 3.0 * own), own)
    assert err <= max(1e-5, 3.0 * own)
    floor = 1e-4 if fixture else 2e-5
    worst = (0.0, 0.0, 0.0, "")
    for k, prm in zip(param_keys(lsnf, depth), net._param_list()):
        own_k = R.rel_l2(p32[k], pref[k])
        err_k = R.rel_l2(prm.grad.cpu().reshape(pref[k].shape), pref[k])
        if err_k / max(floor, 3.0 * own_k) >= worst[0]:
            worst = (err_k / max(floor, 3.0 * own_k), err_k, own_k, k)
    report(f"module {label} d theta worst {worst[3]}", worst[1], max(floor, 3.0 * worst[2]), worst[2])
    assert worst[0] <= 1.0, worst


@pytest.fixture(params=["fast-path", "recomputing-fp32"])
def params_path(request, lsnf):
    prev = lsnf.flow.set_math_mode(lsnf.flow.MATH_FP32 if request.param == "recomputing-fp32" else lsnf.flow.MATH_BF16X3)
    assert lsnf.flow.params_fast_path() == (request.param == "fast-path")
    yield request.param
    lsnf.flow.set_math_mode(prev)


@pytest.mark.parametrize("B", [100, 5000, 20000])
def test_module_kinkfree(lsnf, params_path, gpu_device, B):
    p, eps = kinkfree_case(128, 64, 5, 1, B)
    module_case(lsnf, gpu_device, p, eps, False, f"kink-free B{B} [{params_path}]")


@pytest.mark.parametrize("name", [n for n in golden_names() if n not in ILL])
def test_module_golden_fixtures(lsnf, params_path, gpu_device, name):
    p, g = load_golden(name)
    eps = torch.from_numpy(g["rev_in"])
    keep = O.relu_margin(p, R.reverse64(p, eps)) >= 2e-5
    removed = 1.0 - keep.double().mean().item()
    print(f"[reverse-autograd] module {name}: {removed:.1%} of the rows within 2e-5 of a kink removed")
    assert removed <= 0.15
    module_case(lsnf, gpu_device, p, eps[keep].contiguous(), True, f"{name} [{params_path}]")


def test_module_bridge_behaviour(lsnf, gpu_device, monkeypatch):
    dev = gpu_device
    p, eps = kinkfree_case(128, 64, 5, 1, 100)
    B, nz = eps.shape
    cx, co, obj = (t.to(dev) for t in seeded(B, nz, 300))
    net = module_of(lsnf, p, dev)
    loss_of = lambda x, negobj: (x * cx).sum() / B + (negobj * co).mean()
    # d/d eps alone never runs the parameter-gradient kernels
    calls = []
    real = lsnf.flow.backward_params
    monkeypatch.setattr(lsnf.flow, "backward_params", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    e = eps.to(dev).requires_grad_()
    (ge,) = torch.autograd.grad(loss_of(*net(e, obj, reverse=True, return_obj=True)), e)
    assert not calls and all(q.grad is None for q in net.parameters())
    loss_of(*net(e, obj, reverse=True, return_obj=True)).backward()
    assert len(calls) == 1 and torch.equal(e.grad, ge)
    full = [q.grad.clone() for q in net._param_list()]
    # only the parameters require grad (eps = randn): the same parameter gradients (the contraction accumulates with atomics)
    net.zero_grad(set_to_none=True)
    x = net(eps.to(dev), obj, reverse=True)
    assert x.requires_grad
    (x * cx).sum().backward()
    net.zero_grad(set_to_none=True)
    loss_of(*net(eps.to(dev), obj, reverse=True, return_obj=True)).backward()
    for a, b in zip(net._param_list(), full):
        assert R.rel_l2(a.grad, b) <= 1e-5
    # nothing requires grad, or no_grad: today's path
    for q in net.parameters():
        q.requires_grad_(False)
    assert not net(eps.to(dev), obj, reverse=True).requires_grad
    for q in net.parameters():
        q.requires_grad_(True)
    with torch.no_grad():
        assert not net(e, obj, reverse=True).requires_grad
    # an optimizer step between forward and backward
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    net.zero_grad(set_to_none=True)
    loss = loss_of(*net(e, obj, reverse=True, return_obj=True))
    loss_of(*net(e, obj, reverse=True, return_obj=True)).backward()
    opt.step()
    with pytest.raises(lsnf.LsnfError):
        loss.backward()
    # empty batch
    e0 = torch.zeros(0, nz, device=dev, requires_grad=True)
    x0, n0 = net(e0, torch.zeros(0, device=dev), reverse=True, return_obj=True)
    assert x0.shape == (0, nz) and n0.shape == (0,)
    (x0.sum() + n0.sum()).backward()
    assert e0.grad.shape == (0, nz)
    # CPU tensors
    with pytest.raises(lsnf.LsnfError):
        net(torch.zeros(3, nz, requires_grad=True), torch.zeros(3), reverse=True)


def test_module_round_trip_through_both_bridges(lsnf, gpu_device):
    """netF(netF(z)[0], obj, reverse=True) is the identity: d/dz of (x * c).sum() is c."""
    dev = gpu_device
    nz, B = 128, 100
    p = O.init_params(nz, 64, 5, seed=3)
    z, _ = O.smooth_batch(p, B, nz, seed=B)
    c = seeded(B, nz, 400)[0]
    net = module_of(lsnf, p, dev)
    zd = z.to(dev).requires_grad_()
    z1, ld, _ = net(zd, torch.zeros(B, device=dev))
    x = net(z1, ld, reverse=True)
    (x * c.to(dev)).sum().backward()
    res = R.rel_l2(zd.grad.cpu(), c)
    zo = z.clone().requires_grad_(True)                                       # the same chain in the oracle's fp32
    z1o, ldo = O.flow_forward(p, zo, torch.zeros(B))
    xo, _ = O.flow_reverse(p, z1o, ldo)
    (go,) = torch.autograd.grad((xo * c).sum(), zo)
    own = R.rel_l2(go, c)
    report("round trip d/dz", res, max(2e-5, 3.0 * own), own)
    assert res <= max(2e-5, 3.0 * own)


# ---------------------------------------------------------------------------------------------
# 4. graph capture
# ---------------------------------------------------------------------------------------------
def test_forward_and_reverse_backward_are_graph_capturable(lsnf, gpu_device):
    dev = gpu_device
    f = lsnf.flow
    nz, w, depth, B = 100, 64, 5, 300
    p = O.init_params(nz, w, depth, seed=31)
    plan = make_plan(lsnf, p, dev)
    x = torch.randn(B, nz, generator=torch.Generator().manual_seed(1)).to(dev)
    gx, go = torch.empty(B, nz, device=dev), torch.empty(B, device=dev)
    out = (torch.empty_like(x), torch.empty(B, device=dev), None)
    saved = torch.empty(depth - 1, B, nz, device=dev)
    act = f.new_act_saved(plan, B, dev)
    res = torch.empty_like(x)

    def run():
        f.forward(plan, x, want_ll=False, out=out, z_saved_out=saved, act_saved=act)
        f.reverse_backward_z(plan, out[0], saved, act, gx, go, out=res)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up on a side stream (lazy module load etc.)
        gx.normal_(); go.normal_()
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for seed in (2, 3):                                # two replays with new upstream gradients
        a, b, _ = seeded(B, nz, seed)
        gx.copy_(a.to(dev)); go.copy_(b.to(dev))
        graph.replay()
        torch.cuda.synchronize()
        got = res.clone()
        assert torch.equal(got, rbwd_at(lsnf, plan, x, gx, go))

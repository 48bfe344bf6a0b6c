"""Timing driver for the differentiable reverse pass: `flow.reverse_backward_z` (lsnf_small3_rbwd.hip) next to its yardstick
`flow.backward_z` from the stash (the same four GEMM stages per block) MEASURED IN THE SAME RUN, and the module's full
`loss.backward()` through `netF(eps, obj, reverse=True)` next to `mle_grads`.  C3 geometry (nz=128, w=64, depth 5), default
arithmetic.  HIP events after a clock ramp; median and p10 / p90 over R regions of N back-to-back calls.  Prints one JSON line.

    python tools/run_reverse_autograd.py [N] [R]
"""
import json, os, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import lsnf_amd
from lsnf_amd import flow
n_calls = int(sys.argv[1]) if len(sys.argv) > 1 else 100
regions = int(sys.argv[2]) if len(sys.argv) > 2 else 7
dev = torch.device("cuda:0")
hps = types.SimpleNamespace(f_n_levels=1, f_depth=5, f_flow_permutation=2, f_width=64, f_flow_coupling=1)
torch.manual_seed(1); np.random.seed(1)
net = lsnf_amd._netF(hps, nz=128)
with torch.no_grad():
    for n_, p_ in net.named_parameters():
        if ".fc_zeros." in n_: p_.add_(0.05 * torch.randn_like(p_))
net = net.to(dev); plan = net._plan()


def timed(fn, n):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): fn()
        e1.record(); torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / n * 1e3)
    q = np.percentile(t, [50, 10, 90])
    return {"median_us": round(float(q[0]), 2), "p10_us": round(float(q[1]), 2), "p90_us": round(float(q[2]), 2)}


zr = torch.randn(65536, 128, device=dev)           # clock ramp: the headline forward until the clocks have settled
for _ in range(600): flow.forward(plan, zr, want_ll=False)
torch.cuda.synchronize()

out = {}
for B in (100, 8192, 16384, 65536):
    eps = torch.randn(B, 128, device=dev); obj = torch.randn(B, device=dev)
    gx = torch.randn(B, 128, device=dev); go = torch.randn(B, device=dev)
    x, _ = flow.reverse(plan, eps, obj)
    act = flow.new_act_saved(plan, B, dev)
    outb = (torch.empty_like(x), torch.empty(B, device=dev), None)
    saved = torch.empty((4, B, 128), device=dev)
    res = torch.empty_like(x)
    z1 = flow.forward(plan, x, want_ll=False, out=outb, act_saved=act, z_saved_out=saved)[0]
    n = n_calls if B > 1000 else 4 * n_calls
    r = {}
    r["reverse_backward_z"] = timed(lambda: flow.reverse_backward_z(plan, z1, saved, act, gx, go, out=res), n)
    r["backward_z_from_stash"] = timed(lambda: flow.backward_z(plan, z1, saved, gx, go, act_saved=act), n)
    r["forward_stash"] = timed(lambda: flow.forward(plan, x, want_ll=False, out=outb, act_saved=act, z_saved_out=saved), n)
    r["reverse"] = timed(lambda: flow.reverse(plan, eps, obj), n)
    if B in (100, 65536):
        cx = torch.randn(B, 128, device=dev); co = torch.randn(B, device=dev)

        def full():
            e = eps.detach().requires_grad_()
            xx, negobj = net(e, obj, reverse=True, return_obj=True)
            ((xx * cx).sum() / B + (negobj * co).mean()).backward()
            net.zero_grad(set_to_none=True)
        r["module_reverse_loss_backward"] = timed(full, max(10, n // 4))
        r["mle_grads"] = timed(lambda: net.mle_grads(x, reuse_buffers=True), max(10, n // 4))
    out[f"B={B}"] = r
print(json.dumps(out))

#!/usr/bin/env python3
"""GPU: what the fused base-space Langevin step costs against the launches it replaces, and whether lsnf_reverse_backward_z moved.

    python tools/reverse_langevin_vs_unfused.py [--parent-lib OTHER/liblsnf_flow.so] [--rounds 2] [--out profiles/FILE.txt]

Per batch size (100, 8 192, 16 384; default math mode and dispatch, bench.py's weights: nz 128 / w 64 / depth 5), in ONE job:
  reverse_backward_z      flow.reverse_backward_z(..., out=)                                          (a) this build and the parent
  fused tensor            flow.reverse_langevin_step with a noise tensor, in place, with norms        (b)
  fused philox            ... with the noise drawn in the kernel                                      (b)
  unfused tensor          reverse_backward_z + the torch update and the two norms                     (c) what (b) replaces
  unfused philox          ... and the flow.sample launch that draws the noise                         (c)
  step eager unfused      one step of sample_langevin_post_eps_with_flow (philox, tanh generator)     (d)
  step eager fused        ... fused=True                                                              (d)
  step graphed            one replay of GraphedEpsLangevinSampler                                     (d)
With --parent-lib (a build of the parent commit) `reverse_backward_z` of that build as well, in child processes that alternate
between the two libraries (LSNF_LIB_PATH), `rounds` times each.  A figure is the time per call of a window of back-to-back calls
between two device events (so it includes the launch gaps a caller sees, not only kernel time); every (library, round) takes
WINDOWS windows after a warm-up of every shape; the table gives the median with p10 / p90 over all windows (30 per build at the
default 2 rounds).  No GPU: the driver fails (there is no CPU path)."""
import json
import sys

import ab_harness
from ab_harness import pct

SIZES = (100, 8192, 16384)
WINDOWS = 15
NAMES = ("reverse_backward_z", "fused tensor", "fused philox", "unfused tensor", "unfused philox",
         "step eager unfused", "step eager fused", "step graphed")

CHILD = r'''
import json, math, os, sys, types
import torch
import bench, lsnf_amd
parent = bool(os.environ.get("RLU_PARENT"))
if parent:                                                     # (a build from before the entry point existed)
    lsnf_amd._lib._SIGNATURES.pop("lsnf_reverse_langevin_step", None)
F, L = lsnf_amd.flow, lsnf_amd.langevin
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
weights = [t.to(dev) for t in bench.synth_weights(1)]
plan = lsnf_amd.prepare(weights, bench.NZ, bench.WIDTH, bench.DEPTH)
hps = types.SimpleNamespace(f_n_levels=1, f_depth=bench.DEPTH, f_flow_permutation=2, f_width=bench.WIDTH, f_flow_coupling=1)
net = lsnf_amd._netF(hps, bench.NZ).to(dev)
with torch.no_grad():
    for q, t in zip(net._param_list(), weights):
        q.copy_(t.reshape(q.shape))
for q in net.parameters():
    q.requires_grad_(False)
gen = torch.Generator().manual_seed(5)
w1 = (torch.randn(bench.NZ, 24, generator=gen) / math.sqrt(bench.NZ)).to(dev)
w2 = (torch.randn(24, 16, generator=gen) / math.sqrt(24)).to(dev)
netG = lambda z: torch.tanh(torch.tanh(z.flatten(1) @ w1) @ w2)
sizes, nwin = json.loads(sys.argv[1]), int(sys.argv[2])
S = 0.1
res = {}
for B in sizes:
    f32 = dict(dtype=torch.float32, device=dev)
    eps, gx, noise = torch.randn(B, bench.NZ, **f32), torch.randn(B, bench.NZ, **f32), torch.randn(B, bench.NZ, **f32)
    target = torch.tanh(torch.randn(B, 16, **f32))
    act = F.new_act_saved(plan, B, dev)
    x = F.reverse(plan, eps, None)[0]
    e, _, _, saved = F.forward(plan, x, None, want_ll=False, save_for_backward=True, act_saved=act)
    g, xs, es = torch.empty_like(e), torch.empty_like(e), torch.empty_like(e)
    work, gn, en = e.clone(), torch.empty(B, **f32), torch.empty(B, **f32)
    rng = F.PhiloxNoise(1, 0, 0)

    def unfused(draw):
        F.reverse_backward_z(plan, e, saved, act, gx, None, out=g)
        a, b = g.norm(dim=1), e.norm(dim=1)
        new = e - 0.5 * S * S * (e + g)
        xi = noise if not draw else F.sample(plan, B, rng, want_eps=True, out=(xs, None, es, None))[2]
        return new + S * xi, a, b

    kw = dict(g_l_steps=1, g_l_step_size=S, g_llhd_sigma=0.3)
    fns = {"reverse_backward_z": lambda: F.reverse_backward_z(plan, e, saved, act, gx, None, out=g)}
    if not parent:
        # (in place on a copy whose rows drift with every call: the stash stays that of e, the arithmetic and the traffic are the step's)
        fns["fused tensor"] = lambda: F.reverse_langevin_step(plan, work, saved, act, gx, noise, S, inplace=True, out=(None, None, gn, en))
        fns["fused philox"] = lambda: F.reverse_langevin_step(plan, work, saved, act, gx, rng, S, inplace=True, out=(None, None, gn, en))
        fns["unfused tensor"] = lambda: unfused(False)
        fns["unfused philox"] = lambda: unfused(True)
        fns["step eager unfused"] = lambda: L.sample_langevin_post_eps_with_flow(eps, target, netG, net, philox=F.PhiloxNoise(1, 0, 0), **kw)
        fns["step eager fused"] = lambda: L.sample_langevin_post_eps_with_flow(eps, target, netG, net, philox=F.PhiloxNoise(1, 0, 0), fused=True, **kw)
        if F.reverse_keep_supported(plan, B):
            sampler = L.GraphedEpsLangevinSampler(netG, net, B, bench.NZ, target.shape, g_l_step_size=S, g_llhd_sigma=0.3, seed=1)
            sampler.eps.copy_(eps); sampler.x.copy_(target)
            fns["step graphed"] = lambda: sampler.graph.replay()
    n = 300 if B <= 8192 else 150
    for fn in fns.values():
        for _ in range(n): fn()
        work.copy_(e)
    torch.cuda.synchronize()
    for name, fn in fns.items():
        ts = []
        for _ in range(nwin):
            work.copy_(e)
            ts += windows(fn, n, 1)
        res[f"{B}/{name}"] = ts
emit(res)
'''


def main(argv=None):
    a, libs = ab_harness.parent_lib_args(__doc__, 2, "RLU_PARENT", argv)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS)], timeout=400)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/reverse_langevin_vs_unfused.py: us per call, median [p10, p90] over {a.rounds} x {WINDOWS} windows per library; "
            f"nz=128 w=64 depth=5, default math mode and dispatch", f"{'B':>7} {'what':<20} {'build':<7} {'median':>9} {'p10':>9} {'p90':>9}"]
    for B in SIZES:
        for name in NAMES:
            for tag, _, _ in libs:
                ts = acc.get((tag, f"{B}/{name}"))
                if ts:
                    rows.append(f"{B:>7} {name:<20} {tag:<7} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}")
    ab_harness.finish(rows, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

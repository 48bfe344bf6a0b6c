#!/usr/bin/env python3
"""GPU: what the fused flow-MLE update (netF.mle_step with a FlowAdam) costs against the launches it replaces, and whether
netF.mle_grads moved.

    python tools/mle_step_vs_torch_adam.py [--parent-lib OTHER/liblsnf_flow.so] [--rounds 2] [--out profiles/FILE.txt]

Per batch size (100 and 8 192; default math mode and dispatch, bench.py's weights: nz 128 / w 64 / depth 5), in ONE job:
  mle_grads               netF.mle_grads(z, reuse_buffers=True)                                       (a) this build and the parent
  mle_step                netF.mle_step(z, FlowAdam(max_norm=100))                                    (b)
  torch fused             mle_grads(max_norm=100, reuse_buffers=True) + Adam(fused=True).step()
                          + netF.invalidate_plan() + the next netF._plan()                            (c) what (b) replaces
  torch foreach           ... with Adam(foreach=True) (no invalidate_plan: it bumps the versions)     (c)
  step graphed            one replay of the captured FlowAdam.step() + plan refresh (capturable=True) (d) the update without mle_grads
With --parent-lib (a build of the parent commit) `mle_grads` of that build as well, in child processes that alternate between the
two libraries (LSNF_LIB_PATH), `rounds` times each.  torch's fused Adam writes the parameters without bumping their version counters,
so the module's plan cache does not see its step: a caller has to invalidate the plan by hand, and (c) does, or it would time an
update whose prepared weights are never re-derived.  Two figures per call, both over a window of back-to-back calls: `device` =
the time between two device events around the window (it includes the launch gaps a caller sees, not only kernel time), `host` =
the wall time the host needs to issue the window (before the synchronise).  Every (library, round) takes WINDOWS windows after a
warm-up of every variant; the table gives the median with p10 / p90 over all windows (30 per build at the default 2 rounds).
No GPU: the driver fails (there is no CPU path)."""
import json
import sys

import ab_harness
from ab_harness import pct

SIZES = (100, 8192)
WINDOWS = 15
NAMES = ("mle_grads", "mle_step", "torch fused", "torch foreach", "step graphed")

CHILD = r'''
import json, os, sys, types
import torch
import bench, lsnf_amd
parent = bool(os.environ.get("MSA_PARENT"))
if parent:                                                     # (a build from before the entry points existed)
    for name in ("lsnf_adam_state_bytes", "lsnf_adam_step"):
        lsnf_amd._lib._SIGNATURES.pop(name, None)
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
weights = [t.to(dev) for t in bench.synth_weights(1)]
hps = types.SimpleNamespace(f_n_levels=1, f_depth=bench.DEPTH, f_flow_permutation=2, f_width=bench.WIDTH, f_flow_coupling=1)

def make_net():
    net = lsnf_amd._netF(hps, bench.NZ).to(dev)
    with torch.no_grad():
        for q, t in zip(net._param_list(), weights):
            q.copy_(t.reshape(q.shape))
    return net

sizes, nwin = json.loads(sys.argv[1]), int(sys.argv[2])
HYPER = dict(lr=1e-4, betas=(0.5, 0.999))
res = {}
for B in sizes:
    z = torch.randn(B, bench.NZ, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    fns = {}
    n_a = make_net()
    fns["mle_grads"] = lambda: n_a.mle_grads(z, reuse_buffers=True)
    if not parent:
        n_b = make_net(); o_b = lsnf_amd.FlowAdam(n_b, max_norm=100.0, **HYPER)
        fns["mle_step"] = lambda: n_b.mle_step(z, o_b)
        for tag, kw in (("torch fused", dict(fused=True)), ("torch foreach", dict(foreach=True))):
            n_c = make_net(); o_c = torch.optim.Adam(n_c.parameters(), **HYPER, **kw)
            def replaced(n_c=n_c, o_c=o_c, invalidate="fused" in kw):
                n_c.mle_grads(z, max_norm=100.0, reuse_buffers=True)
                o_c.step()
                if invalidate:
                    n_c.invalidate_plan()
                n_c._plan()
            fns[tag] = replaced
        n_d = make_net(); o_d = lsnf_amd.FlowAdam(n_d, max_norm=100.0, capturable=True, **dict(HYPER, lr=1e-7))   # (frozen gradients: a rate that keeps the weights in place)
        n_d.mle_step(z, o_d)                                   # gradients in place, code objects loaded, the device lr filled
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            o_d.step()
            n_d._plan()
        fns["step graphed"] = graph.replay
    n = 200
    for fn in fns.values():
        for _ in range(n): fn()
    torch.cuda.synchronize()
    for name, fn in fns.items():
        res[f"{B}/{name}/device"], res[f"{B}/{name}/host"] = windows(fn, n, nwin, host=True)
emit(res)
'''


def main(argv=None):
    a, libs = ab_harness.parent_lib_args(__doc__, 2, "MSA_PARENT", argv)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS)], timeout=400)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/mle_step_vs_torch_adam.py: us per call, median [p10, p90] over {a.rounds} x {WINDOWS} windows per library; "
            f"nz=128 w=64 depth=5, default math mode and dispatch",
            f"{'B':>7} {'what':<16} {'build':<7} {'clock':<7} {'median':>9} {'p10':>9} {'p90':>9}"]
    for B in SIZES:
        for name in NAMES:
            for tag, _, _ in libs:
                for clock in ("device", "host"):
                    ts = acc.get((tag, f"{B}/{name}/{clock}"))
                    if ts:
                        rows.append(f"{B:>7} {name:<16} {tag:<7} {clock:<7} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}")
    ab_harness.finish(rows, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

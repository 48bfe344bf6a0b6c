#!/usr/bin/env python3
"""GPU: what the variants of the fused optimizer step cost, and whether the default `FlowAdam.step()` moved.

    python tools/flow_adam_variants_cost.py --parent-lib OTHER/liblsnf_flow.so [--rounds 2] [--out profiles/FILE.txt]

At bench.py's geometry (nz 128 / w 64 / depth 5: 60 tensors, 177 k elements), static gradients, a learning rate that keeps the
weights in place, in ONE job: child processes that alternate between this tree's library, a build of the parent commit
(LSNF_LIB_PATH) and THE SAME parent build a second time (tag `parent2`), `rounds` times each.  The parent children time what
that library has -- the default step, with and without the clip; this tree's children time those and every variant:
  default             FlowAdam(netF).step()                                        one launch
  clip                FlowAdam(netF, max_norm=100).step()                          two launches (norm, update)
  amsgrad / adamw / maximize / ema / skip                                          each option alone (skip: two launches)
  all                 FlowAdamW(amsgrad, maximize, ema_decay, skip_nonfinite, max_norm=100)
  ... graphed         one replay of a captured step() (capturable=True) of default, clip and all: the eager rows are bound by
                      the host (Python issues a step in about the time the device needs), these show the device's share
`device` = the time between two device events around a window of back-to-back calls (launch gaps included), `host` = the wall
time the host needs to issue the window.  Every (library, round) takes WINDOWS windows after a warm-up of every variant; the
table gives the median with p10 / p90 over all windows.
Bar for the default path (`default` and `clip`, device clock): the median of this tree differs from the parent's by no more than
the medians of the two parent runs differ from each other in this job.  The variants' costs are recorded, not gated.  The
children also hash the parameters and the state after three default steps on seeded values: this tree and the parent must
agree bit for bit.  Exit status 1 if the bar is missed or the bits differ.  No GPU: the driver fails (there is no CPU path)."""
import sys

import ab_harness
from ab_harness import pct

WINDOWS = 15
CALLS = 200
DEFAULT = ("default", "clip")
VARIANTS = ("amsgrad", "adamw", "maximize", "ema", "skip", "all", "default graphed", "clip graphed", "all graphed")

CHILD = r'''
import hashlib, types
import torch
import bench, lsnf_amd
parent = bool(os.environ.get("FAV_PARENT"))
if parent:                                                     # (a build from before the entry points existed)
    for name in ("lsnf_adam_state_bytes_ex", "lsnf_adam_step_ex"):
        lsnf_amd._lib._SIGNATURES.pop(name, None)
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
weights = [t.to(dev) for t in bench.synth_weights(1)]
hps = types.SimpleNamespace(f_n_levels=1, f_depth=bench.DEPTH, f_flow_permutation=2, f_width=bench.WIDTH, f_flow_coupling=1)

def make_net(seed=5):
    gen = torch.Generator(device=dev).manual_seed(seed)
    net = lsnf_amd._netF(hps, bench.NZ).to(dev)
    with torch.no_grad():
        for q, t in zip(net._param_list(), weights):
            q.copy_(t.reshape(q.shape))
    for q in net._param_list():
        q.grad = torch.randn(q.shape, device=dev, generator=gen) * 0.02
    return net

n, nwin = int(sys.argv[1]), int(sys.argv[2])
A, W = lsnf_amd.FlowAdam, getattr(lsnf_amd, "FlowAdamW", None)
KW = dict(lr=1e-7, betas=(0.5, 0.999))                          # (static gradients: a rate that keeps the weights in place)
makers = {"default": lambda net: A(net, **KW), "clip": lambda net: A(net, max_norm=100.0, **KW)}
if not parent:
    makers.update({
        "amsgrad": lambda net: A(net, amsgrad=True, **KW),
        "adamw": lambda net: W(net, **KW),
        "maximize": lambda net: A(net, maximize=True, **KW),
        "ema": lambda net: A(net, ema_decay=0.999, **KW),
        "skip": lambda net: A(net, skip_nonfinite=True, **KW),
        "all": lambda net: W(net, amsgrad=True, maximize=True, ema_decay=0.999, skip_nonfinite=True, max_norm=100.0, **KW)})
fns, keep = {}, []
for name, mk in makers.items():
    fns[name] = mk(make_net()).step
for name in ("default", "clip") + (() if parent else ("all",)):      # the device's share: one replay of the captured step
    net = make_net()
    opt = makers[name](net)
    opt.capturable = True
    opt.step()                                                 # code objects loaded, the device lr filled
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    keep.append((net, opt, graph))
    fns[name + " graphed"] = graph.replay
for fn in fns.values():
    for _ in range(n): fn()
torch.cuda.synchronize()
res = {}
for name, fn in fns.items():
    res[name + "/device"], res[name + "/host"] = windows(fn, n, nwin, host=True)
# the bits of the default path: three steps (no clip, then the clip twice) at a rate that moves the weights
net = make_net()
opt = A(net, lr=1e-3, betas=(0.5, 0.999), weight_decay=1e-2)
h = hashlib.sha256()
for k in range(3):
    opt.param_groups[0]["max_norm"] = 0.05 if k else None
    opt.step()
torch.cuda.synchronize()
for t in list(net._param_list()) + [opt._flat]:
    h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
res["_bits"] = h.hexdigest()
emit(res)
'''


def main(argv=None):
    a, libs = ab_harness.parent_lib_args(__doc__, 2, "FAV_PARENT", argv)
    if a.parent_lib:
        libs.append(("parent2", a.parent_lib, {"FAV_PARENT": "1"}))
    res = ab_harness.run(CHILD, libs, a.rounds, [str(CALLS), str(WINDOWS)], timeout=280)
    if res is None:
        return 1
    bits = {tag: sorted({p.pop("_bits") for p in payloads}) for tag, payloads in res.items()}
    acc = ab_harness.pooled(res)
    rows = [f"# tools/flow_adam_variants_cost.py: us per FlowAdam.step(), median [p10, p90] over {a.rounds} x {WINDOWS} windows of {CALLS} "
            f"calls per library; nz=128 w=64 depth=5, static gradients",
            f"{'what':<16} {'build':<8} {'clock':<7} {'median':>9} {'p10':>9} {'p90':>9}"]
    for name in DEFAULT + VARIANTS:
        for tag, _, _ in libs:
            for clock in ("device", "host"):
                ts = acc.get((tag, f"{name}/{clock}"))
                if ts:
                    rows.append(f"{name:<16} {tag:<8} {clock:<7} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}")
    bad = 0
    if a.parent_lib:
        for name in DEFAULT:
            med = {tag: pct(acc[(tag, f"{name}/device")], 0.5) for tag in ("this", "parent", "parent2")}
            moved, spread = abs(med["this"] - med["parent"]), abs(med["parent"] - med["parent2"])
            ok = moved <= spread
            bad += not ok
            rows.append(f"# bar, {name}: |this - parent| = {moved:.2f} us, |parent - parent2| = {spread:.2f} us: {'met' if ok else 'MISSED'}")
        same = len({tuple(v) for v in bits.values()}) == 1 and all(len(v) == 1 for v in bits.values())
        bad += not same
        rows.append(f"# bits of three default steps (parameters + state, sha256 {bits['this'][0][:16]}...): "
                    f"{'identical in every child of every build' if same else 'DIFFERENT: ' + repr(bits)}")
    ab_harness.finish(rows, a.out)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

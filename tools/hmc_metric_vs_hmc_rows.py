#!/usr/bin/env python3
"""GPU: what a diagonal metric per row costs a call of Hamiltonian Monte Carlo, per phase, and what folding and closing a window add.

    python tools/hmc_metric_vs_hmc_rows.py [--parent-lib OTHER/liblsnf_flow.so] [--rounds 2] [--out profiles/FILE.txt]

Per batch size (100 and 16 384; default math mode and dispatch, bench.py's weights: nz 128 / w 64 / depth 5; Philox noise, a
generator gradient and energy given, the next point written out of place so that every call sees the same rows), in ONE job, the
entry points called directly on the stash of one forward -- the launch alone, no flow pass; every measured launch has a chain
state, steps, scales and window of its own:
  hmc_rows_init / _inner / _end      lsnf_hmc_step_rows in its three phases (the end call begins the next trajectory)
  hmc_metric_init / _inner / _end    lsnf_hmc_step_metric likewise, no window: 4 nz B more read per row in every phase (twice in an end call)
  hmc_metric_fold                    an end call with LSNF_HMC_METRIC_FOLD: mean and m2 read and written, 16 nz B more per row
  hmc_metric_close                   ... and LSNF_HMC_METRIC_CLOSE: the scale written as well, a sqrtf and three divisions per column
  rhmc_...                           the same eight of lsnf_reverse_hmc_step_rows / lsnf_reverse_hmc_step_metric
With --parent-lib (a build of the parent commit) the per-row calls of that build as well, in child processes that alternate between
the two libraries (LSNF_LIB_PATH), `rounds` times each.  A figure is the time per call of a window of back-to-back calls between two
device events (so it includes the launch gaps a caller sees, not only kernel time); every (library, round) takes WINDOWS windows
after a warm-up of every shape; the table gives the median with p10 / p90 over all windows.  Below the table: each metric launch over
its per-row twin, and whether its median lies above the twin's p90.  No threshold is fixed: the file is the record.  No GPU: the
driver fails (there is no CPU path)."""
import json
import sys

import ab_harness
from ab_harness import pct

SIZES = (100, 16384)
WINDOWS = 15
FORMS = ("rows_init", "rows_inner", "rows_end", "metric_init", "metric_inner", "metric_end", "metric_fold", "metric_close")
NAMES = tuple(f"{k}_{f}" for k in ("hmc", "rhmc") for f in FORMS)
TWIN = {f"{k}_metric_{f}": f"{k}_rows_{'end' if f in ('fold', 'close') else f}" for k in ("hmc", "rhmc") for f in ("init", "inner", "end", "fold", "close")}

CHILD = r'''
import ctypes, json, os, sys
import torch
import bench, lsnf_amd
parent = bool(os.environ.get("HMM_PARENT"))
if parent:                                                     # (a build from before the entry points existed)
    lsnf_amd._lib._EXT_SIGNATURES.pop("lsnf_hmc_step_metric", None)
    lsnf_amd._lib._EXT_SIGNATURES.pop("lsnf_reverse_hmc_step_metric", None)
F = lsnf_amd.flow
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
params = [t.to(dev) for t in bench.synth_weights(1)]
plan = lsnf_amd.prepare(params, bench.NZ, bench.WIDTH, bench.DEPTH)
sizes, nwin = json.loads(sys.argv[1]), int(sys.argv[2])
S = 0.1
INIT, INNER, FOLD, CLOSE = 1, 2, 16, 32
torch.manual_seed(0)                                           # (every child times the same rows)
res = {}
head, ptr, call = F._plan_head(plan), F._ptr, F._call
for B in sizes:
    f32 = dict(dtype=torch.float32, device=dev)
    eps0, gg, energy = torch.randn(B, bench.NZ, **f32), 0.1 * torch.randn(B, bench.NZ, **f32), torch.rand(B, **f32)
    x = F.reverse(plan, eps0, None)[0]
    act = F.new_act_saved(plan, B, dev)
    eps, _, ll, saved = F.forward(plan, x, None, want_ll=True, save_for_backward=True, act_saved=act)   # (eps: the forward's own output at x)
    rows = lambda: torch.zeros(B, bench.NZ, **f32)
    rng = F.PhiloxNoise(1, 0, 0)
    def bound(space, kind, form):
        """One measured call with chain state, momentum, steps, scales and outputs of its own.  space: "z" (the chain on x, the
        point the stash belongs to) or "eps"; kind: "rows" or "metric"; form: "init", "inner", "end", "fold" or "close"."""
        point = x if space == "z" else eps
        p_acc, g_acc, u_acc, kin = point.clone(), gg.clone(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        mom, nxt, acc, la = torch.randn(B, bench.NZ, **f32), rows(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        steps = F.new_hmc_row_steps(B, dev, S)
        metric = F.new_hmc_row_metric(plan, B, dev) if kind == "metric" else None
        if space == "z":
            fixed = (B, ptr(x), ptr(eps), ptr(saved), ptr(act), ptr(ll), ptr(gg), ptr(energy))
            name = "lsnf_hmc_step_" + kind
        else:
            fixed = (B, ptr(eps), ptr(saved), ptr(act), ptr(gg), ptr(energy))
            name = "lsnf_reverse_hmc_step_" + kind
        state = (ptr(p_acc), ptr(g_acc), ptr(u_acc), ptr(mom), ptr(kin), None, None)
        inner = form == "inner"
        flags = {"init": INIT, "inner": INNER, "end": 0, "fold": FOLD, "close": FOLD | CLOSE}[form]
        keep = (p_acc, g_acc, u_acc, kin, mom, nxt, acc, la, steps, metric)
        def fn(keep=keep):
            r = None if inner else ctypes.byref(rng._c())
            extra = ()
            if metric is not None:
                extra = (ptr(metric.scale), None, None, None, None)
                if flags & FOLD:
                    reg = lsnf_amd._lib.LsnfMetricReg(metric.n0, metric.var0, metric.scale_min, metric.scale_max)
                    extra = (ptr(metric.scale), ptr(metric.mean), ptr(metric.m2), ptr(metric.count), ctypes.byref(reg))
            out = (None, None) if inner else (ptr(acc), ptr(la))
            call(name, dev, *head, *fixed, *state, r, ptr(steps.step), None, None, *extra, flags, ptr(nxt), *out)
        fn.mom, fn.metric = mom, metric
        return fn
    fns = {}
    for key, space in (("hmc", "z"), ("rhmc", "eps")):
        for form in ("init", "inner", "end"):
            fns[f"{key}_rows_{form}"] = bound(space, "rows", form)
        if not parent:
            for form in ("init", "inner", "end", "fold", "close"):
                fns[f"{key}_metric_{form}"] = bound(space, "metric", form)
    n = 300 if B <= 8192 else 150
    for fn in fns.values():
        for _ in range(n): fn()
    torch.cuda.synchronize()
    for name, fn in fns.items():
        ts = []
        for _ in range(nwin):
            fn.mom.normal_()                                   # (every call replaces mom: the same scale for every window)
            if fn.metric is not None:                          # (a closing call moves the scales: every window starts at 1, empty)
                fn.metric.scale.fill_(1.0); fn.metric.mean.zero_(); fn.metric.m2.zero_(); fn.metric.count.zero_()
            ts += windows(fn, n, 1)
        res[f"{B}/{name}"] = ts
emit(res)
'''


def main(argv=None):
    a, libs = ab_harness.parent_lib_args(__doc__, 2, "HMM_PARENT", argv)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS)], timeout=500, swap=True)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/hmc_metric_vs_hmc_rows.py: us per launch, median [p10, p90] over {a.rounds} x {WINDOWS} windows per library; "
            f"nz=128 w=64 depth=5, default math mode and dispatch, Philox noise", f"{'B':>7} {'what':<18} {'build':<7} {'median':>9} {'p10':>9} {'p90':>9}"]
    for B in SIZES:
        for name in NAMES:
            for tag, _, _ in libs:
                ts = acc.get((tag, f"{B}/{name}"))
                if ts:
                    rows.append(f"{B:>7} {name:<18} {tag:<7} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}")
    for B in SIZES:
        for name, twin in TWIN.items():
            ts = acc.get(("this", f"{B}/{name}"))
            ref = acc.get(("this", f"{B}/{twin}"))
            if ts and ref:
                m, lo, hi = pct(ts, 0.5), pct(ref, 0.1), pct(ref, 0.9)
                rows.append(f"# B={B}: {name} / {twin} = {m / pct(ref, 0.5):.3f} (medians); its median {m:.2f} us is "
                            f"{'ABOVE' if m > hi else 'NOT ABOVE'} that call's p90 [p10 {lo:.2f}, p90 {hi:.2f}]")
    ab_harness.finish(rows, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

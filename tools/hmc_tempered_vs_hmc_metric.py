#!/usr/bin/env python3
"""GPU: what a likelihood temperature per row costs an end call of Hamiltonian Monte Carlo, and what the fused anneal adds.

    python tools/hmc_tempered_vs_hmc_metric.py [--rounds 2] [--out profiles/FILE.txt]

Per batch size (100 and 16 384; default math mode and dispatch, bench.py's weights: nz 128 / w 64 / depth 5; Philox noise, a
generator gradient and energy given, the next point written out of place so that every call sees the same rows), in ONE job, the
entry points called directly on the stash of one forward -- the launch alone, no flow pass; every measured launch has a chain
state, steps, scales and temperatures of its own:
  hmc_metric_end       lsnf_hmc_step_metric, an end call that begins the next trajectory, no window
  hmc_tempered_end     lsnf_hmc_step_tempered likewise, without LSNF_HMC_ANNEAL: beta read per row, grad_g read a second time and
                       like_grad_acc / like_u_acc written on accepted rows (4 nz B read and 4 nz B written more per accepted row)
  hmc_tempered_anneal  ... with LSNF_HMC_ANNEAL: beta_next and the log_w pair read, like_grad_acc read on rejected rows, grad_acc and
                       u_acc written for every row, log_w and beta written
  rhmc_...             the same three of lsnf_reverse_hmc_step_metric / lsnf_reverse_hmc_step_tempered
A figure is the time per call of a window of back-to-back calls between two device events (so it includes the launch gaps a caller
sees, not only kernel time); every round takes WINDOWS windows after a warm-up of every shape; the table gives the median with
p10 / p90 over all windows.  Below the table: each tempered launch over the metric end call of the same job, and whether its median
lies above that call's p90.  No threshold is fixed: the file is the record.  No GPU: the driver fails (there is no CPU path)."""
import argparse
import json
import sys

import ab_harness
from ab_harness import pct

SIZES = (100, 16384)
WINDOWS = 15
FORMS = ("metric_end", "tempered_end", "tempered_anneal")
NAMES = tuple(f"{k}_{f}" for k in ("hmc", "rhmc") for f in FORMS)
TWIN = {f"{k}_{f}": f"{k}_metric_end" for k in ("hmc", "rhmc") for f in FORMS[1:]}

CHILD = r'''
import ctypes, json, os, sys
import torch
import bench, lsnf_amd
F = lsnf_amd.flow
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
params = [t.to(dev) for t in bench.synth_weights(1)]
plan = lsnf_amd.prepare(params, bench.NZ, bench.WIDTH, bench.DEPTH)
sizes, nwin = json.loads(sys.argv[1]), int(sys.argv[2])
S = 0.1
ANNEAL = 64
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
    def bound(space, form):
        """One measured end call with chain state, momentum, steps, scales, temperatures and outputs of its own.  space: "z" (the chain
        on x, the point the stash belongs to) or "eps"; form: "metric_end", "tempered_end" or "tempered_anneal"."""
        point = x if space == "z" else eps
        p_acc, g_acc, u_acc, kin = point.clone(), gg.clone(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        mom, nxt, acc, la = torch.randn(B, bench.NZ, **f32), rows(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        steps, metric = F.new_hmc_row_steps(B, dev, S), F.new_hmc_row_metric(plan, B, dev)
        tempered, anneal = form != "metric_end", form == "tempered_anneal"
        temper = F.new_hmc_row_temper(plan, B, dev, 0.5) if tempered else None
        nxt_beta = torch.full((B,), 0.5, **f32)               # (the same temperature again: every window decides the same trajectories)
        kind = "tempered" if tempered else "metric"
        if space == "z":
            fixed = (B, ptr(x), ptr(eps), ptr(saved), ptr(act), ptr(ll), ptr(gg), ptr(energy))
            name = "lsnf_hmc_step_" + kind
        else:
            fixed = (B, ptr(eps), ptr(saved), ptr(act), ptr(gg), ptr(energy))
            name = "lsnf_reverse_hmc_step_" + kind
        state = (ptr(p_acc), ptr(g_acc), ptr(u_acc), ptr(mom), ptr(kin), None, None)
        keep = (p_acc, g_acc, u_acc, kin, mom, nxt, acc, la, steps, metric, temper, nxt_beta)
        def fn(keep=keep):
            extra = (ptr(metric.scale), None, None, None, None)
            if tempered:
                extra += (ptr(temper.beta), ptr(nxt_beta) if anneal else None, ptr(temper.like_grad), ptr(temper.like_energy),
                          ptr(temper.log_w) if anneal else None)
            call(name, dev, *head, *fixed, *state, ctypes.byref(rng._c()), ptr(steps.step), None, None, *extra, ANNEAL if anneal else 0,
                 ptr(nxt), ptr(acc), ptr(la))
        fn.mom = mom
        return fn
    fns = {f"{key}_{form}": bound(space, form) for key, space in (("hmc", "z"), ("rhmc", "eps")) for form in ("metric_end", "tempered_end", "tempered_anneal")}
    n = 300 if B <= 8192 else 150
    for fn in fns.values():
        for _ in range(n): fn()
    torch.cuda.synchronize()
    for name, fn in fns.items():
        ts = []
        for _ in range(nwin):
            fn.mom.normal_()                                   # (every call replaces mom: the same scale for every window)
            ts += windows(fn, n, 1)
        res[f"{B}/{name}"] = ts
emit(res)
'''


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    libs = [("this", None, {})]                              # (the metric call of the same build, in the same job, is the yardstick)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS)], timeout=500, swap=True)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/hmc_tempered_vs_hmc_metric.py: us per launch, median [p10, p90] over {a.rounds} x {WINDOWS} windows; "
            f"nz=128 w=64 depth=5, default math mode and dispatch, Philox noise", f"{'B':>7} {'what':<20} {'median':>9} {'p10':>9} {'p90':>9}"]
    for B in SIZES:
        for name in NAMES:
            ts = acc.get(("this", f"{B}/{name}"))
            if ts:
                rows.append(f"{B:>7} {name:<20} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}")
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

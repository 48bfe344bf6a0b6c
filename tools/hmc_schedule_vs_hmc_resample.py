#!/usr/bin/env python3
"""GPU: what the scheduling entry points cost an annealing end call of Hamiltonian Monte Carlo over the resampling ones, and what the
search adds.

    python tools/hmc_schedule_vs_hmc_resample.py [--rounds 2] [--out profiles/FILE.txt]

Per batch size (128 = 8 groups of 16, and 16 384; default math mode and dispatch, bench.py's weights: nz 128 / w 64 / depth 5; Philox
noise, a generator gradient and energy given, the next point written out of place so that every call sees the same rows), in ONE job,
the entry points called directly on the stash of one forward -- the launch alone, no flow pass; every measured launch has a chain
state, steps, scales, temperatures and weights of its own (groups of 16, ess_frac 0.5, energies in U(0, 10)):
  hmc_resample_anneal    lsnf_hmc_step_resample, an end call with LSNF_HMC_ANNEAL | LSNF_HMC_RESAMPLE that begins the next trajectory
                         (beta 0.5 annealed to 0.6).  Its kernels are compiled from unchanged text (the object file is the parent
                         commit's byte for byte), so this launch IS the parent commit's SMC end call, measured in the same job
  hmc_schedule_off       lsnf_hmc_step_schedule likewise, without LSNF_HMC_SCHEDULE: the same tail in another kernel
  hmc_schedule_search    ... with LSNF_HMC_SCHEDULE, cess_frac 0.95, min_step 0, ceiling 1, beta reset to 0.2 before every window: the
                         groups search (thirteen evaluations of cess: 2 x 4 lane permutes, an expf and a division each)
  hmc_schedule_ceiling   ... beta = ceiling = 0.6: nothing moves.  (The kernel forms the halvings for every group whatever its state --
                         the groups of a wave differ and the exchanges need the whole wave -- so this figure is the search's as well.)
  rhmc_...               the same four of lsnf_reverse_hmc_step_resample / lsnf_reverse_hmc_step_schedule
A figure is the time per call of a window of back-to-back calls between two device events (so it includes the launch gaps a caller
sees, not only kernel time); every round takes WINDOWS windows after a warm-up of every shape; the table gives the median with
p10 / p90 over all windows.  Below the table: each scheduling launch over the resampling call of the same job, and whether its median
lies above that call's p90.  No threshold is fixed: the file is the record.  No GPU: the driver fails (there is no CPU path)."""
import argparse
import json
import sys

import ab_harness
from ab_harness import pct

SIZES = (128, 16384)
WINDOWS = 15
FORMS = ("resample_anneal", "schedule_off", "schedule_search", "schedule_ceiling")
NAMES = tuple(f"{k}_{f}" for k in ("hmc", "rhmc") for f in FORMS)
TWIN = {f"{k}_{f}": f"{k}_resample_anneal" for k in ("hmc", "rhmc") for f in FORMS[1:]}
GROUP = 16

CHILD = r'''
import ctypes, json, os, sys
import torch
import bench, lsnf_amd
F = lsnf_amd.flow
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
params = [t.to(dev) for t in bench.synth_weights(1)]
plan = lsnf_amd.prepare(params, bench.NZ, bench.WIDTH, bench.DEPTH)
sizes, nwin, P = json.loads(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
S = 0.1
ANNEAL, RESAMPLE, SCHEDULE = 64, 512, 1024
torch.manual_seed(0)                                           # (every child times the same rows)
res = {}
head, ptr, call = F._plan_head(plan), F._ptr, F._call
for B in sizes:
    f32 = dict(dtype=torch.float32, device=dev)
    eps0, gg, energy = torch.randn(B, bench.NZ, **f32), 0.1 * torch.randn(B, bench.NZ, **f32), 10.0 * torch.rand(B, **f32)
    x = F.reverse(plan, eps0, None)[0]
    act = F.new_act_saved(plan, B, dev)
    eps, _, ll, saved = F.forward(plan, x, None, want_ll=True, save_for_backward=True, act_saved=act)   # (eps: the forward's own output at x)
    rows = lambda: torch.zeros(B, bench.NZ, **f32)
    rng = F.PhiloxNoise(1, 0, 0)
    def bound(space, form):
        """One measured annealing end call with chain state, momentum, steps, scales, temperatures, weights and outputs of its own."""
        point = x if space == "z" else eps
        p_acc, g_acc, u_acc, kin = point.clone(), gg.clone(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        mom, nxt, acc, la = torch.randn(B, bench.NZ, **f32), rows(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        steps, metric = F.new_hmc_row_steps(B, dev, S), F.new_hmc_row_metric(plan, B, dev)
        new = form != "resample_anneal"
        start = 0.2 if form == "schedule_search" else 0.6 if form == "schedule_ceiling" else 0.5
        temper = F.new_hmc_row_temper(plan, B, dev, start)
        temper.like_energy.copy_(energy)
        temper.log_w[:, 0] = 3.0 * torch.randn(B, **f32)
        bn = torch.full((B,), 1.0 if form == "schedule_search" else 0.6, **f32)
        ancestor, ess = torch.zeros(B, **f32), torch.zeros(B, **f32)
        flags = ANNEAL | RESAMPLE | (SCHEDULE if form in ("schedule_search", "schedule_ceiling") else 0)
        kind = "schedule" if new else "resample"
        if space == "z":
            fixed = (B, ptr(x), ptr(eps), ptr(saved), ptr(act), ptr(ll), ptr(gg), ptr(energy))
            name = "lsnf_hmc_step_" + kind
        else:
            fixed = (B, ptr(eps), ptr(saved), ptr(act), ptr(gg), ptr(energy))
            name = "lsnf_reverse_hmc_step_" + kind
        state = (ptr(p_acc), ptr(g_acc), ptr(u_acc), ptr(mom), ptr(kin), None, None)
        keep = (p_acc, g_acc, u_acc, kin, mom, nxt, acc, la, steps, metric, temper, bn, ancestor, ess)
        def fn(keep=keep):
            extra = (ptr(metric.scale), None, None, None, None, ptr(temper.beta), ptr(bn), ptr(temper.like_grad), ptr(temper.like_energy),
                     ptr(temper.log_w))
            tail = (P, 0.5, None, ptr(ancestor), ptr(ess)) + ((0.95, 0.0) if new else ())
            call(name, dev, *head, *fixed, *state, ctypes.byref(rng._c()), ptr(steps.step), None, None, *extra, flags,
                 ptr(nxt), ptr(acc), ptr(la), *tail)
        fn.mom, fn.temper, fn.start = mom, temper, start
        return fn
    fns = {f"{key}_{form}": bound(space, form) for key, space in (("hmc", "z"), ("rhmc", "eps"))
           for form in ("resample_anneal", "schedule_off", "schedule_search", "schedule_ceiling")}
    n = 300 if B <= 8192 else 150
    for fn in fns.values():
        for _ in range(n): fn()
    torch.cuda.synchronize()
    for name, fn in fns.items():
        ts = []
        for _ in range(nwin):
            fn.mom.normal_()                                   # (every call replaces mom: the same scale for every window)
            fn.temper.log_w[:, 0].normal_(0.0, 3.0); fn.temper.log_w[:, 1].zero_()      # (and the weights' spread)
            fn.temper.beta.fill_(fn.start)                     # (and the temperatures: an annealing call moves them)
            ts += windows(fn, n, 1)
        res[f"{B}/{name}"] = ts
emit(res)
'''


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    libs = [("this", None, {})]                              # (the resampling call of the same build, in the same job, is the yardstick)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS), str(GROUP)], timeout=500, swap=True)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/hmc_schedule_vs_hmc_resample.py: us per launch, median [p10, p90] over {a.rounds} x {WINDOWS} windows; "
            f"nz=128 w=64 depth=5, default math mode and dispatch, Philox noise, groups of {GROUP}", f"{'B':>7} {'what':<22} {'median':>9} {'p10':>9} {'p90':>9}"]
    for B in SIZES:
        for name in NAMES:
            ts = acc.get(("this", f"{B}/{name}"))
            if ts:
                rows.append(f"{B:>7} {name:<22} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}")
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

#!/usr/bin/env python3
"""GPU: what the replica-exchange entry points cost an end call of Hamiltonian Monte Carlo over the tempered ones, and what the swap adds.

    python tools/hmc_exchange_vs_hmc_tempered.py [--rounds 2] [--out profiles/FILE.txt]

Per batch size (100 and 16 384; default math mode and dispatch, bench.py's weights: nz 128 / w 64 / depth 5; Philox noise, a
generator gradient and energy given, the next point written out of place so that every call sees the same rows), in ONE job, the
entry points called directly on the stash of one forward -- the launch alone, no flow pass; every measured launch has a chain
state, steps, scales and temperatures of its own (a geometric ladder of 4 rungs from 0.05 to 1 repeated over the rows):
  hmc_tempered_end      lsnf_hmc_step_tempered, an end call that begins the next trajectory, no anneal
  hmc_exchange_end      lsnf_hmc_step_exchange likewise, without LSNF_HMC_SWAP: the same tail in another kernel
  hmc_exchange_even     ... with LSNF_HMC_SWAP, ladder 4: like_u_acc read, like_grad_acc read on rejected rows, three scalars and six quads
                        per lane moved across lanes, the pair's uniform drawn, swapped / log_swap written; a row that swaps writes
                        z_acc, grad_acc, like_grad_acc, u_acc and like_u_acc a second time
  hmc_exchange_odd      ... with LSNF_HMC_SWAP | LSNF_HMC_SWAP_ODD: half of the rows idle
  rhmc_...              the same four of lsnf_reverse_hmc_step_tempered / lsnf_reverse_hmc_step_exchange
A figure is the time per call of a window of back-to-back calls between two device events (so it includes the launch gaps a caller
sees, not only kernel time); every round takes WINDOWS windows after a warm-up of every shape; the table gives the median with
p10 / p90 over all windows.  Below the table: each exchange launch over the tempered end call of the same job, and whether its median
lies above that call's p90.  No threshold is fixed: the file is the record.  No GPU: the driver fails (there is no CPU path)."""
import argparse
import json
import sys

import ab_harness
from ab_harness import pct

SIZES = (100, 16384)
WINDOWS = 15
FORMS = ("tempered_end", "exchange_end", "exchange_even", "exchange_odd")
NAMES = tuple(f"{k}_{f}" for k in ("hmc", "rhmc") for f in FORMS)
TWIN = {f"{k}_{f}": f"{k}_tempered_end" for k in ("hmc", "rhmc") for f in FORMS[1:]}
LADDER = 4

CHILD = r'''
import ctypes, json, os, sys
import torch
import bench, lsnf_amd
F = lsnf_amd.flow
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
params = [t.to(dev) for t in bench.synth_weights(1)]
plan = lsnf_amd.prepare(params, bench.NZ, bench.WIDTH, bench.DEPTH)
sizes, nwin, R = json.loads(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
S = 0.1
SWAP, ODD = 128, 256
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
        on x, the point the stash belongs to) or "eps"; form: "tempered_end", "exchange_end", "exchange_even" or "exchange_odd"."""
        point = x if space == "z" else eps
        p_acc, g_acc, u_acc, kin = point.clone(), gg.clone(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        mom, nxt, acc, la = torch.randn(B, bench.NZ, **f32), rows(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        steps, metric = F.new_hmc_row_steps(B, dev, S), F.new_hmc_row_metric(plan, B, dev)
        exchange, swap = form != "tempered_end", form in ("exchange_even", "exchange_odd")
        temper = F.new_hmc_row_temper(plan, B, dev, lsnf_amd.langevin.pt_ladder(R, 0.05).float().repeat(B // R))
        swapped, log_swap = torch.zeros(B, **f32), torch.zeros(B, **f32)
        flags = 0 if not swap else SWAP | (ODD if form == "exchange_odd" else 0)
        kind = "exchange" if exchange else "tempered"
        if space == "z":
            fixed = (B, ptr(x), ptr(eps), ptr(saved), ptr(act), ptr(ll), ptr(gg), ptr(energy))
            name = "lsnf_hmc_step_" + kind
        else:
            fixed = (B, ptr(eps), ptr(saved), ptr(act), ptr(gg), ptr(energy))
            name = "lsnf_reverse_hmc_step_" + kind
        state = (ptr(p_acc), ptr(g_acc), ptr(u_acc), ptr(mom), ptr(kin), None, None)
        keep = (p_acc, g_acc, u_acc, kin, mom, nxt, acc, la, steps, metric, temper, swapped, log_swap)
        def fn(keep=keep):
            extra = (ptr(metric.scale), None, None, None, None, ptr(temper.beta), None, ptr(temper.like_grad), ptr(temper.like_energy), None)
            tail = () if not exchange else (R, None, ptr(swapped), ptr(log_swap)) if swap else (0, None, None, None)
            call(name, dev, *head, *fixed, *state, ctypes.byref(rng._c()), ptr(steps.step), None, None, *extra, flags,
                 ptr(nxt), ptr(acc), ptr(la), *tail)
        fn.mom = mom
        return fn
    fns = {f"{key}_{form}": bound(space, form) for key, space in (("hmc", "z"), ("rhmc", "eps"))
           for form in ("tempered_end", "exchange_end", "exchange_even", "exchange_odd")}
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
    libs = [("this", None, {})]                              # (the tempered call of the same build, in the same job, is the yardstick)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS), str(LADDER)], timeout=500, swap=True)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/hmc_exchange_vs_hmc_tempered.py: us per launch, median [p10, p90] over {a.rounds} x {WINDOWS} windows; "
            f"nz=128 w=64 depth=5, default math mode and dispatch, Philox noise, ladder {LADDER}", f"{'B':>7} {'what':<20} {'median':>9} {'p10':>9} {'p90':>9}"]
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

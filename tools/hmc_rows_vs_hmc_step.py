#!/usr/bin/env python3
"""GPU: what reading the step per row, and adapting it, costs an end call of Hamiltonian Monte Carlo.

    python tools/hmc_rows_vs_hmc_step.py [--parent-lib OTHER/liblsnf_flow.so] [--rounds 2] [--out profiles/FILE.txt]

Per batch size (100 and 16 384; default math mode and dispatch, bench.py's weights: nz 128 / w 64 / depth 5; Philox noise, a
generator gradient and energy given, the next point written out of place so that every call sees the same rows), in ONE job, the
entry points called directly on the stash of one forward -- the launch alone, no flow pass; every measured launch has a chain
state, steps and adaptation state of its own:
  hmc_end          lsnf_hmc_step, flags 0, deciding and beginning the next trajectory                     this build and the parent
  hmc_rows_end     lsnf_hmc_step_rows, flags 0: 4 B more read per row
  hmc_rows_adapt   lsnf_hmc_step_rows, LSNF_HMC_ADAPT: 20 B more read and 20 B more written per row, the update's arithmetic
  rhmc_end / rhmc_rows_end / rhmc_rows_adapt    the same three of lsnf_reverse_hmc_step / lsnf_reverse_hmc_step_rows
With --parent-lib (a build of the parent commit) the two scalar calls of that build as well, in child processes that alternate
between the two libraries (LSNF_LIB_PATH), `rounds` times each.  A figure is the time per call of a window of back-to-back calls
between two device events (so it includes the launch gaps a caller sees, not only kernel time); every (library, round) takes
WINDOWS windows after a warm-up of every shape; the table gives the median with p10 / p90 over all windows.  Below the table: each
per-row launch over its scalar twin, and whether its median lies above the twin's p90 (the parent's where given).  No threshold is
fixed: the file is the record.  No GPU: the driver fails (there is no CPU path)."""
import json
import sys

import ab_harness
from ab_harness import pct

SIZES = (100, 16384)
WINDOWS = 15
NAMES = ("hmc_end", "hmc_rows_end", "hmc_rows_adapt", "rhmc_end", "rhmc_rows_end", "rhmc_rows_adapt")
TWIN = {"hmc_rows_end": "hmc_end", "hmc_rows_adapt": "hmc_end", "rhmc_rows_end": "rhmc_end", "rhmc_rows_adapt": "rhmc_end"}

CHILD = r'''
import ctypes, json, os, sys
import torch
import bench, lsnf_amd
parent = bool(os.environ.get("HMR_PARENT"))
if parent:                                                     # (a build from before the entry points existed)
    lsnf_amd._lib._EXT_SIGNATURES.pop("lsnf_hmc_step_rows", None)
    lsnf_amd._lib._EXT_SIGNATURES.pop("lsnf_reverse_hmc_step_rows", None)
F = lsnf_amd.flow
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
params = [t.to(dev) for t in bench.synth_weights(1)]
plan = lsnf_amd.prepare(params, bench.NZ, bench.WIDTH, bench.DEPTH)
sizes, nwin = json.loads(sys.argv[1]), int(sys.argv[2])
S = 0.1
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
        """One measured end call with chain state, momentum, steps and outputs of its own.  space: "z" (the chain on x, the point
        the stash belongs to) or "eps"; form: "scalar", "rows" or "adapt"."""
        point = x if space == "z" else eps
        p_acc, g_acc, u_acc, kin = point.clone(), gg.clone(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        mom, nxt, acc, la = torch.randn(B, bench.NZ, **f32), rows(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        steps = F.new_hmc_row_steps(B, dev, S) if not parent else None
        if space == "z":
            fixed = (B, ptr(x), ptr(eps), ptr(saved), ptr(act), ptr(ll), ptr(gg), ptr(energy))
            name = "lsnf_hmc_step"
        else:
            fixed = (B, ptr(eps), ptr(saved), ptr(act), ptr(gg), ptr(energy))
            name = "lsnf_reverse_hmc_step"
        state = (ptr(p_acc), ptr(g_acc), ptr(u_acc), ptr(mom), ptr(kin), None, None)
        keep = (p_acc, g_acc, u_acc, kin, mom, nxt, acc, la, steps)
        def fn(keep=keep):
            r = ctypes.byref(rng._c())
            if form == "scalar":
                call(name, dev, *head, *fixed, *state, r, S, 0, ptr(nxt), ptr(acc), ptr(la))
            elif form == "rows":
                call(name + "_rows", dev, *head, *fixed, *state, r, ptr(steps.step), None, None, 0, ptr(nxt), ptr(acc), ptr(la))
            else:
                da = lsnf_amd._lib.LsnfDualAvg(steps.target_accept, steps.gamma, steps.t0, steps.kappa, steps.step_min, steps.step_max)
                call(name + "_rows", dev, *head, *fixed, *state, r, ptr(steps.step), ptr(steps.adapt), ctypes.byref(da), F.HMC_ADAPT,
                     ptr(nxt), ptr(acc), ptr(la))
        fn.mom, fn.steps = mom, steps
        return fn
    fns = {"hmc_end": bound("z", "scalar"), "rhmc_end": bound("eps", "scalar")}
    if not parent:
        fns.update(hmc_rows_end=bound("z", "rows"), hmc_rows_adapt=bound("z", "adapt"),
                   rhmc_rows_end=bound("eps", "rows"), rhmc_rows_adapt=bound("eps", "adapt"))
    n = 300 if B <= 8192 else 150
    for fn in fns.values():
        for _ in range(n): fn()
    torch.cuda.synchronize()
    for name, fn in fns.items():
        ts = []
        for _ in range(nwin):
            fn.mom.normal_()                                   # (an end call replaces mom every time: the same scale for every window)
            if fn.steps is not None:                           # (an adapting call moves the steps: every window starts at S, count 0)
                fresh = F.new_hmc_row_steps(B, dev, S)
                fn.steps.step.copy_(fresh.step); fn.steps.adapt.copy_(fresh.adapt)
            ts += windows(fn, n, 1)
        res[f"{B}/{name}"] = ts
emit(res)
'''


def main(argv=None):
    a, libs = ab_harness.parent_lib_args(__doc__, 2, "HMR_PARENT", argv)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS)], timeout=500, swap=True)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/hmc_rows_vs_hmc_step.py: us per launch, median [p10, p90] over {a.rounds} x {WINDOWS} windows per library; "
            f"nz=128 w=64 depth=5, default math mode and dispatch, Philox noise", f"{'B':>7} {'what':<16} {'build':<7} {'median':>9} {'p10':>9} {'p90':>9}"]
    for B in SIZES:
        for name in NAMES:
            for tag, _, _ in libs:
                ts = acc.get((tag, f"{B}/{name}"))
                if ts:
                    rows.append(f"{B:>7} {name:<16} {tag:<7} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}")
    for B in SIZES:
        for name, twin in TWIN.items():
            ts = acc.get(("this", f"{B}/{name}"))
            ref = acc.get(("parent", f"{B}/{twin}")) or acc.get(("this", f"{B}/{twin}"))
            if ts and ref:
                which = "the parent's" if ("parent", f"{B}/{twin}") in acc else "this build's"
                m, lo, hi = pct(ts, 0.5), pct(ref, 0.1), pct(ref, 0.9)
                rows.append(f"# B={B}: {name} / {twin} = {m / pct(ref, 0.5):.3f} (medians, {which} {twin}); its median {m:.2f} us is "
                            f"{'ABOVE' if m > hi else 'NOT ABOVE'} that call's p90 [p10 {lo:.2f}, p90 {hi:.2f}]")
    ab_harness.finish(rows, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

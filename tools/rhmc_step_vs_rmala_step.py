#!/usr/bin/env python3
"""GPU: what ONE launch of the base-space Hamiltonian Monte Carlo step costs against one launch of the base-space
Metropolis-adjusted Langevin step.

    python tools/rhmc_step_vs_rmala_step.py [--parent-lib OTHER/liblsnf_flow.so] [--rounds 2] [--out profiles/FILE.txt]

Per batch size (100 and 16 384; default math mode and dispatch, bench.py's weights: nz 128 / w 64 / depth 5; Philox noise, a
generator gradient and energy given, the next point written out of place so that every call sees the same rows), in ONE job, the
entry points called directly on the stash of one forward at x = f^-1(eps) -- the launch alone, no flow pass; every measured launch
has a chain state of its own, so its cost does not depend on what else the child measures (an accepted row stores two more rows
than a rejected one):
  rmala_step      lsnf_reverse_mala_step, deciding and proposing                                         this build and the parent
  rhmc_inner      lsnf_reverse_hmc_step with LSNF_HMC_INNER: reads eps_prop, mom; writes mom, eps_next: no barrier, no sums, no draw
  rhmc_end        lsnf_reverse_hmc_step with flags 0, deciding and beginning the next trajectory: one more (B, nz) array read and
                  written than rmala_step
  rhmc_init       lsnf_reverse_hmc_step with LSNF_HMC_INIT
With --parent-lib (a build of the parent commit) `rmala_step` of that build as well, in child processes that alternate between the
two libraries (LSNF_LIB_PATH), `rounds` times each.  A figure is the time per call of a window of back-to-back calls between two
device events (so it includes the launch gaps a caller sees, not only kernel time); every (library, round) takes WINDOWS windows
after a warm-up of every shape; the table gives the median with p10 / p90 over all windows.  Below the table: each HMC launch
over this build's rmala_step, and whether rhmc_inner's median lies above the MALA launch's p90 (the parent's where given).  No
threshold is fixed: the file is the record.  No GPU: the driver fails (there is no CPU path)."""
import json
import sys

import ab_harness
from ab_harness import pct

SIZES = (100, 16384)
WINDOWS = 15
NAMES = ("rmala_step", "rhmc_inner", "rhmc_end", "rhmc_init")

CHILD = r'''
import ctypes, json, os, sys
import torch
import bench, lsnf_amd
parent = bool(os.environ.get("RHM_PARENT"))
if parent:                                                     # (a build from before the entry point existed)
    lsnf_amd._lib._EXT_SIGNATURES.pop("lsnf_reverse_hmc_step", None)
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
    eps, _, _, saved = F.forward(plan, x, None, want_ll=False, save_for_backward=True, act_saved=act)   # (eps: the forward's own output at x)
    rows = lambda: torch.zeros(B, bench.NZ, **f32)
    rng = F.PhiloxNoise(1, 0, 0)
    def bound(name, flags=0):
        """One measured launch with chain state, momentum and outputs of its own."""
        e_acc, g_acc, u_acc, kin = eps.clone(), gg.clone(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        mom, e_next, acc, la = torch.randn(B, bench.NZ, **f32), rows(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        fixed = (B, ptr(eps), ptr(saved), ptr(act), ptr(gg), ptr(energy), ptr(e_acc), ptr(g_acc), ptr(u_acc))
        keep = (e_acc, g_acc, u_acc, kin, mom, e_next, acc, la)
        def fn(keep=keep):
            if name == "lsnf_reverse_mala_step":
                call(name, dev, *head, *fixed, None, None, ctypes.byref(rng._c()), S, 0, ptr(e_next), ptr(acc), ptr(la))
            else:
                r = None if flags == 2 else ctypes.byref(rng._c())
                o = (None, None) if flags == 2 else (ptr(acc), ptr(la))
                call(name, dev, *head, *fixed, ptr(mom), ptr(kin), None, None, r, S, flags, ptr(e_next), *o)
        fn.mom = mom
        return fn
    rhmc = lambda flags: bound("lsnf_reverse_hmc_step", flags)
    fns = {"rmala_step": bound("lsnf_reverse_mala_step")}
    if not parent:
        fns.update(rhmc_inner=rhmc(2), rhmc_end=rhmc(0), rhmc_init=rhmc(1))
    n = 300 if B <= 8192 else 150
    for fn in fns.values():
        for _ in range(n): fn()
    torch.cuda.synchronize()
    for name, fn in fns.items():
        ts = []
        for _ in range(nwin):
            fn.mom.normal_()                                   # (an inner call moves mom every time: keep it finite)
            ts += windows(fn, n, 1)
        res[f"{B}/{name}"] = ts
emit(res)
'''


def main(argv=None):
    a, libs = ab_harness.parent_lib_args(__doc__, 2, "RHM_PARENT", argv)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS)], timeout=400, swap=True)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/rhmc_step_vs_rmala_step.py: us per launch, median [p10, p90] over {a.rounds} x {WINDOWS} windows per library; "
            f"nz=128 w=64 depth=5, default math mode and dispatch, Philox noise", f"{'B':>7} {'what':<16} {'build':<7} {'median':>9} {'p10':>9} {'p90':>9}"]
    for B in SIZES:
        for name in NAMES:
            for tag, _, _ in libs:
                ts = acc.get((tag, f"{B}/{name}"))
                if ts:
                    rows.append(f"{B:>7} {name:<16} {tag:<7} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}")
    for B in SIZES:
        mala = acc.get(("this", f"{B}/rmala_step"))
        ref = acc.get(("parent", f"{B}/rmala_step")) or mala
        for name in NAMES[1:]:
            ts = acc.get(("this", f"{B}/{name}"))
            if ts and mala:
                rows.append(f"# B={B}: {name} / rmala_step = {pct(ts, 0.5) / pct(mala, 0.5):.3f} (medians, this build)")
        inner = acc.get(("this", f"{B}/rhmc_inner"))
        if inner and ref:
            lo, hi, m = pct(ref, 0.1), pct(ref, 0.9), pct(inner, 0.5)
            which = "the parent's" if ("parent", f"{B}/rmala_step") in acc else "this build's"
            rows.append(f"# B={B}: rhmc_inner median {m:.2f} us is {'ABOVE' if m > hi else 'NOT ABOVE'} the p90 of {which} rmala_step "
                        f"[p10 {lo:.2f}, p90 {hi:.2f}]")
    ab_harness.finish(rows, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""GPU: what the base-space Metropolis-adjusted step costs against the plain fused base-space Langevin step, and whether the plain
step moved.

    python tools/rmala_step_vs_reverse_langevin_step.py [--parent-lib OTHER/liblsnf_flow.so] [--rounds 2] [--out profiles/FILE.txt]

Per batch size (100 and 16 384; default math mode and dispatch, bench.py's weights: nz 128 / w 64 / depth 5; Philox noise, a
generator gradient and energy given, in place), in ONE job -- the flow's two launches of a sampler step, without the generator:
  reverse_langevin_step   flow.reverse at eps + flow.reverse_langevin_step (fused update, its norms)           this build and the parent
  reverse_mala_step       flow.reverse at eps + flow.reverse_mala_step (accept / reject tail: decide + propose)  this build
The reverse keeps the stash itself where `flow.reverse_keep_supported` (B = 100); elsewhere (16 384 rows) it is the plain reverse
and the step reads a stash made once, by a forward at x, before the timing -- the same on both sides.
With --parent-lib (a build of the parent commit) `reverse_langevin_step` of that build as well, in child processes that alternate
between the two libraries (LSNF_LIB_PATH), `rounds` times each.  A figure is the time per call of a window of back-to-back calls
between two device events (so it includes the launch gaps a caller sees, not only kernel time); every (library, round) takes
WINDOWS windows after a warm-up of every shape; the table gives the median with p10 / p90 over all windows.  Below the table:
whether this build's `reverse_langevin_step` median lies inside the parent's own p10-p90 spread (its kernels are the parent's:
anything else is a finding to explain).  No ratio is fixed for the MALA tail: the file is the record.  No GPU: the driver fails
(there is no CPU path)."""
import json
import sys

import ab_harness
from ab_harness import pct

SIZES = (100, 16384)
WINDOWS = 15
NAMES = ("reverse_langevin_step", "reverse_mala_step")

CHILD = r'''
import json, os, sys
import torch
import bench, lsnf_amd
parent = bool(os.environ.get("RMS_PARENT"))
if parent:                                                     # (a build from before the entry point existed)
    lsnf_amd._lib._EXT_SIGNATURES.pop("lsnf_reverse_mala_step", None)
F = lsnf_amd.flow
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
weights = [t.to(dev) for t in bench.synth_weights(1)]
plan = lsnf_amd.prepare(weights, bench.NZ, bench.WIDTH, bench.DEPTH)
sizes, nwin = json.loads(sys.argv[1]), int(sys.argv[2])
S = 0.1
res = {}
for B in sizes:
    f32 = dict(dtype=torch.float32, device=dev)
    eps0, gg, energy = torch.randn(B, bench.NZ, **f32), 0.1 * torch.randn(B, bench.NZ, **f32), torch.rand(B, **f32)
    eps, rng = eps0.clone(), F.PhiloxNoise(1, 0, 0)
    act = F.new_act_saved(plan, B, dev)
    x, obj, gn, en = torch.empty_like(eps), torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(B, **f32)
    keeps = F.reverse_keep_supported(plan, B)
    saved = torch.empty((plan.depth - 1, B, plan.nz), **f32)
    if not keeps:                                              # (the stash of the start; the rows drift, the traffic is the step's)
        F.reverse(plan, eps, None, out=(x, obj))
        saved = F.forward(plan, x, None, want_ll=False, save_for_backward=True, act_saved=act)[3]

    def reverse():
        if keeps:
            F.reverse(plan, eps, None, out=(x, obj), act_saved=act, z_saved_out=saved)
        else:
            F.reverse(plan, eps, None, out=(x, obj))

    def plain():
        reverse()
        F.reverse_langevin_step(plan, eps, saved, act, gg, rng, S, inplace=True, out=(None, None, gn, en))

    fns = {"reverse_langevin_step": plain}
    if not parent:
        state = F.new_mala_state(plan, B, dev)
        reverse()
        F.reverse_mala_step(plan, eps, saved, act, gg, energy, state, rng, S, init=True, inplace=True, reuse_buffers=True)

        def mala():
            reverse()
            F.reverse_mala_step(plan, eps, saved, act, gg, energy, state, rng, S, inplace=True, reuse_buffers=True)
        fns["reverse_mala_step"] = mala
    n = 300 if B <= 8192 else 150
    for fn in fns.values():
        eps.copy_(eps0)
        for _ in range(n): fn()
    torch.cuda.synchronize()
    for name, fn in fns.items():
        ts = []
        for _ in range(nwin):
            eps.copy_(eps0)                                    # (every window walks the same rows)
            ts += windows(fn, n, 1)
        res[f"{B}/{name}"] = ts
emit(res)
'''


def main(argv=None):
    a, libs = ab_harness.parent_lib_args(__doc__, 2, "RMS_PARENT", argv)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS)], timeout=400, swap=True)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/rmala_step_vs_reverse_langevin_step.py: us per call (reverse + step), median [p10, p90] over {a.rounds} x {WINDOWS} "
            f"windows per library; nz=128 w=64 depth=5, default math mode and dispatch, Philox noise",
            f"{'B':>7} {'what':<24} {'build':<7} {'median':>9} {'p10':>9} {'p90':>9}"]
    for B in SIZES:
        for name in NAMES:
            for tag, _, _ in libs:
                ts = acc.get((tag, f"{B}/{name}"))
                if ts:
                    rows.append(f"{B:>7} {name:<24} {tag:<7} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}")
    for B in SIZES:
        mine, theirs = acc.get(("this", f"{B}/reverse_langevin_step")), acc.get(("parent", f"{B}/reverse_langevin_step"))
        mala = acc.get(("this", f"{B}/reverse_mala_step"))
        if mine and mala:
            rows.append(f"# B={B}: reverse_mala_step / reverse_langevin_step = {pct(mala, 0.5) / pct(mine, 0.5):.3f} (medians, this build)")
        if mine and theirs:
            lo, hi, m = pct(theirs, 0.1), pct(theirs, 0.9), pct(mine, 0.5)
            rows.append(f"# B={B}: reverse_langevin_step median {m:.2f} us is {'INSIDE' if lo <= m <= hi else 'OUTSIDE'} the parent's p10-p90 "
                        f"[{lo:.2f}, {hi:.2f}]")
    ab_harness.finish(rows, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

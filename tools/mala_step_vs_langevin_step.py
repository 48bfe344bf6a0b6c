#!/usr/bin/env python3
"""GPU: what the Metropolis-adjusted step costs against the plain fused Langevin step, and whether the plain step moved.

    python tools/mala_step_vs_langevin_step.py [--parent-lib OTHER/liblsnf_flow.so] [--rounds 2] [--out profiles/FILE.txt]

Per batch size (100 and 16 384; default math mode and dispatch, bench.py's weights: nz 128 / w 64 / depth 5; Philox noise, a
generator gradient and energy given, in place, buffers kept on the plan), in ONE job:
  langevin_step   _netF.langevin_step: the forward and the backward with the update as its output section      this build and the parent
  mala_step       _netF.mala_step: the forward and the backward with the accept / reject tail (decide + propose) this build
With --parent-lib (a build of the parent commit) `langevin_step` of that build as well, in child processes that alternate between
the two libraries (LSNF_LIB_PATH), `rounds` times each.  A figure is the time per call of a window of back-to-back calls between two
device events (so it includes the launch gaps a caller sees, not only kernel time); every (library, round) takes WINDOWS windows
after a warm-up of every shape; the table gives the median with p10 / p90 over all windows.  Below the table: whether this build's
`langevin_step` median lies inside the parent's own p10-p90 spread (its kernels are the parent's, byte for byte: anything else is
a finding to explain).  No ratio is fixed for the MALA tail: the file is the record.  No GPU: the driver fails (there is no CPU path)."""
import json
import sys

import ab_harness
from ab_harness import pct

SIZES = (100, 16384)
WINDOWS = 15
NAMES = ("langevin_step", "mala_step")

CHILD = r'''
import json, os, sys, types
import torch
import bench, lsnf_amd
parent = bool(os.environ.get("MSL_PARENT"))
if parent:                                                     # (a build from before the entry point existed)
    lsnf_amd._lib._EXT_SIGNATURES.pop("lsnf_mala_step", None)
F = lsnf_amd.flow
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
weights = [t.to(dev) for t in bench.synth_weights(1)]
hps = types.SimpleNamespace(f_n_levels=1, f_depth=bench.DEPTH, f_flow_permutation=2, f_width=bench.WIDTH, f_flow_coupling=1)
net = lsnf_amd._netF(hps, bench.NZ).to(dev)
with torch.no_grad():
    for q, t in zip(net._param_list(), weights):
        q.copy_(t.reshape(q.shape))
for q in net.parameters():
    q.requires_grad_(False)
sizes, nwin = json.loads(sys.argv[1]), int(sys.argv[2])
S = 0.1
res = {}
for B in sizes:
    f32 = dict(dtype=torch.float32, device=dev)
    z0, gg, energy = torch.randn(B, bench.NZ, **f32), 0.1 * torch.randn(B, bench.NZ, **f32), torch.rand(B, **f32)
    z, rng = z0.clone(), F.PhiloxNoise(1, 0, 0)
    fns = {"langevin_step": lambda: net.langevin_step(z, gg, rng, S, inplace=True, reuse_buffers=True)}
    if not parent:
        state = F.new_mala_state(net._plan(), B, dev)
        net.mala_step(z, gg, energy, state, rng, S, init=True, inplace=True, reuse_buffers=True)
        fns["mala_step"] = lambda: net.mala_step(z, gg, energy, state, rng, S, inplace=True, reuse_buffers=True)
    n = 300 if B <= 8192 else 150
    for fn in fns.values():
        z.copy_(z0)
        for _ in range(n): fn()
    torch.cuda.synchronize()
    for name, fn in fns.items():
        ts = []
        for _ in range(nwin):
            z.copy_(z0)                                        # (every window walks the same rows)
            ts += windows(fn, n, 1)
        res[f"{B}/{name}"] = ts
emit(res)
'''


def main(argv=None):
    a, libs = ab_harness.parent_lib_args(__doc__, 2, "MSL_PARENT", argv)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS)], timeout=400, swap=True)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/mala_step_vs_langevin_step.py: us per call, median [p10, p90] over {a.rounds} x {WINDOWS} windows per library; "
            f"nz=128 w=64 depth=5, default math mode and dispatch, Philox noise", f"{'B':>7} {'what':<16} {'build':<7} {'median':>9} {'p10':>9} {'p90':>9}"]
    for B in SIZES:
        for name in NAMES:
            for tag, _, _ in libs:
                ts = acc.get((tag, f"{B}/{name}"))
                if ts:
                    rows.append(f"{B:>7} {name:<16} {tag:<7} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}")
    for B in SIZES:
        mine, theirs = acc.get(("this", f"{B}/langevin_step")), acc.get(("parent", f"{B}/langevin_step"))
        mala = acc.get(("this", f"{B}/mala_step"))
        if mine and mala:
            rows.append(f"# B={B}: mala_step / langevin_step = {pct(mala, 0.5) / pct(mine, 0.5):.3f} (medians, this build)")
        if mine and theirs:
            lo, hi, m = pct(theirs, 0.1), pct(theirs, 0.9), pct(mine, 0.5)
            rows.append(f"# B={B}: langevin_step median {m:.2f} us is {'INSIDE' if lo <= m <= hi else 'OUTSIDE'} the parent's p10-p90 "
                        f"[{lo:.2f}, {hi:.2f}]")
    ab_harness.finish(rows, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

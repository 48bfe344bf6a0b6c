#!/usr/bin/env python3
"""GPU: what fused prior sampling costs against what it replaces, and whether lsnf_reverse moved.

    python tools/sample_vs_randn_reverse.py [--parent-lib OTHER/liblsnf_flow.so] [--rounds 3] [--out profiles/FILE.txt]

Per batch size (100, 8 192, 65 536; default math mode and dispatch, bench.py's weights), in ONE job:
  sample          flow.sample(plan, B, rng, out=...)                                   one launch
  randn+reverse   torch.randn((B, nz), out=...) + flow.reverse(plan, eps, out=...)     what a caller did before (two launches;
                  the reverse is given objective = None, so no zeros tensor is charged to it)
  reverse         flow.reverse(plan, eps, out=...) alone
and, with --parent-lib (a build of the parent commit), `reverse` and `randn+reverse` of that build as well, in child processes
that alternate between the two libraries (LSNF_LIB_PATH), `rounds` times each.  A figure is the time per call of a window of
back-to-back calls between two device events (so it includes the launch gaps a caller sees, not only kernel time); every
(library, round) takes WINDOWS windows after a warm-up of every shape; the table gives the median with p10 / p90 over all
windows.  No GPU: the driver fails (there is no CPU path)."""
import json
import sys

import ab_harness
from ab_harness import pct

SIZES = (100, 8192, 65536)
WINDOWS = 15

CHILD = r'''
import json, os, sys
import torch
import bench, lsnf_amd
if os.environ.get("SVR_NO_SAMPLE"):
    lsnf_amd._lib._SIGNATURES.pop("lsnf_sample", None)      # (a build from before the entry point existed)
F = lsnf_amd.flow
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
plan = lsnf_amd.prepare([t.to(dev) for t in bench.synth_weights(1)], bench.NZ, bench.WIDTH, bench.DEPTH)
has_sample = "lsnf_sample" in lsnf_amd._lib._SIGNATURES
sizes, nwin = json.loads(sys.argv[1]), int(sys.argv[2])
res = {}
for B in sizes:
    f32 = dict(dtype=torch.float32, device=dev)
    eps, x, obj, ll = torch.empty(B, bench.NZ, **f32), torch.empty(B, bench.NZ, **f32), torch.empty(B, **f32), torch.empty(B, **f32)
    torch.randn((B, bench.NZ), out=eps)
    ph = F.PhiloxNoise(1234, 0, 0)
    fns = {"reverse": lambda: F.reverse(plan, eps, out=(x, obj)),
           "randn+reverse": lambda: (torch.randn((B, bench.NZ), out=eps), F.reverse(plan, eps, out=(x, obj)))}
    if has_sample:
        fns["sample"] = lambda: F.sample(plan, B, ph, out=(x, obj, None, None))
        fns["sample+eps+ll"] = lambda: F.sample(plan, B, ph, out=(x, obj, eps, ll))
    n = 400 if B <= 8192 else 150
    for fn in fns.values():
        for _ in range(n): fn()
    torch.cuda.synchronize()
    for name, fn in fns.items():
        res[f"{B}/{name}"] = windows(fn, n, nwin)
emit(res)
'''


def main(argv=None):
    a, libs = ab_harness.parent_lib_args(__doc__, 3, "SVR_NO_SAMPLE", argv)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS)], timeout=500)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/sample_vs_randn_reverse.py: us per call, median [p10, p90] over {a.rounds} x {WINDOWS} windows per library; "
            f"nz={128} default math mode and dispatch", f"{'B':>7} {'what':<16} {'build':<7} {'median':>9} {'p10':>9} {'p90':>9}"]
    for B in SIZES:
        for name in ("sample", "sample+eps+ll", "randn+reverse", "reverse"):
            for tag, _, _ in libs:
                ts = acc.get((tag, f"{B}/{name}"))
                if ts:
                    rows.append(f"{B:>7} {name:<16} {tag:<7} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}")
    ab_harness.finish(rows, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

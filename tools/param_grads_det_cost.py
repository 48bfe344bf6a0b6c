#!/usr/bin/env python3
"""GPU: what the deterministic parameter gradients cost, and whether the default path moved against the parent commit.

    python tools/param_grads_det_cost.py [--parent-lib OTHER/liblsnf_flow.so] [--rounds 2] [--out profiles/param_grads_det_cost.txt]

us per call of `flow.backward_params` (nz 128 / f_width 64 / depth 5, bench.py's weights, default math mode and dispatch) at
B = 100, 8 192 and 65 536, on the fast path (from the forward's stash) and on the recomputing path:
  default   this tree, deterministic=False       -- and, with --parent-lib (a build of the parent commit), that build as well
  det       this tree, deterministic=True        (lsnf_backward_params_det: per-chunk partials + lsnf_fold_reduce_kernel)
in ONE job: child processes that alternate between the two libraries (LSNF_LIB_PATH), `rounds` times each, one alive at a time,
each under its own time limit, nothing started after a child that failed (tools/ab_harness.py).  A figure is the time per call of
a window of back-to-back calls between two device events; every (library, round) takes WINDOWS windows after a warm-up; the table
gives the median with p10 / p90 over all windows, and next to the deterministic rows the bytes of the partials (written once,
read once).  Below the table: the worst per-tensor relative L2 between five runs at 65 536 rows, default and deterministic.
No GPU: the driver fails (there is no CPU path)."""
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
parent = bool(os.environ.get("PGD_PARENT"))
if parent:      # (a build from before the entry points existed)
    for name in ("lsnf_backward_params_det", "lsnf_backward_params_det_workspace_floats"):
        lsnf_amd._lib._SIGNATURES.pop(name, None)
F = lsnf_amd.flow
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
params = [t.to(dev) for t in bench.synth_weights(1)]
plan = lsnf_amd.prepare(params, bench.NZ, bench.WIDTH, bench.DEPTH)
sizes, nwin = json.loads(sys.argv[1]), int(sys.argv[2])
res = {}
for B in sizes:
    z = torch.randn(B, bench.NZ, device=dev, generator=torch.Generator(device=dev).manual_seed(B))
    sides = ("default",) if parent else ("default", "det")
    fns = {}
    keep = []
    for side in sides:
        det = side == "det"
        kw = dict(deterministic=True) if det else {}
        act, ws = F.new_act_saved(plan, B, dev), F.new_params_workspace(plan, B, dev, **kw)
        z1, _, _, saved = F.forward(plan, z, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
        z1r, _, _, savedr = F.forward(plan, z, want_ll=False, save_for_backward=True)
        keep.append((act, ws, z1, saved, z1r, savedr))
        fns[f"{B}/fast/{side}"] = (lambda z1=z1, saved=saved, act=act, ws=ws, kw=kw:
                                   F.backward_params(plan, params, z, z1, saved, ll_scale=-1.0 / B, reuse_buffers=True, act_saved=act, workspace=ws, **kw))
        # (reuse_buffers keeps ONE set of buffers per plan, keyed by the flag and by who owns the workspace: every row below is
        #  therefore warmed up and timed on its own, never alternating with another inside a window)
        fns[f"{B}/recompute/{side}"] = (lambda z1r=z1r, savedr=savedr, kw=kw:
                                        F.backward_params(plan, params, z, z1r, savedr, ll_scale=-1.0 / B, reuse_buffers=True, **kw))
    n = 200 if B <= 100 else (100 if B <= 8192 else 30)
    for name, fn in fns.items():
        for _ in range(n): fn()
        torch.cuda.synchronize()
        res[name] = windows(fn, n, nwin)
    if B == sizes[-1]:      # run-to-run spread: worst per-tensor relative L2 between five runs of the fast path
        for side in sides:
            fn = fns[f"{B}/fast/{side}"]
            runs = [[g.double().clone() for g in fn()] for _ in range(5)]
            worst = max(((a - b).norm() / b.norm()).item() for r in runs[1:] for a, b in zip(r, runs[0]))
            res[f"spread/{B}/{side}"] = [worst]
    del keep, fns
emit(res)
'''


def partial_bytes(B, nz=128, w=64, depth=5):
    """Bytes of the partials the contraction of such a call writes (include/lsnf_flow.h): chunks x depth x fold, fast path / recomputing."""
    half = nz // 2
    fold = (nz * nz + nz + half * w + w + w * w + w + 2 * (w * half + half) + 3) // 4 * 4
    rows = 512 if B >= 16384 else 128
    fp32 = -(-B // rows)
    x3 = -(-B // ((-(-B // (256 // depth)) + 31) // 32 * 32)) if B >= 12288 else None
    return {"fast": (x3 or fp32) * depth * fold * 4, "recompute": fp32 * depth * fold * 4}


def main(argv=None):
    a, libs = ab_harness.parent_lib_args(__doc__, 2, "PGD_PARENT", argv)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS)], timeout=400, swap=True)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/param_grads_det_cost.py: flow.backward_params, us per call, median [p10, p90] over {a.rounds} x {WINDOWS} windows per "
            f"library; nz=128 f_width=64 depth=5, default math mode and dispatch",
            f"{'B':>7} {'path':<10} {'side':<8} {'build':<7} {'median':>9} {'p10':>9} {'p90':>9}  {'partials':>12}"]
    for B in SIZES:
        for path in ("fast", "recompute"):
            for side in ("default", "det"):
                for tag, _, _ in libs:
                    ts = acc.get((tag, f"{B}/{path}/{side}"))
                    if ts:
                        extra = f"{partial_bytes(B)[path]:>12,}" if side == "det" else ""
                        rows.append(f"{B:>7} {path:<10} {side:<8} {tag:<7} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}  {extra}")
    rows.append("# worst per-tensor relative L2 between five runs (fast path), per child")
    for (tag, key), vals in sorted(acc.items()):
        if key.startswith("spread/"):
            rows.append(f"{key:<24} {tag:<7} " + " ".join(f"{v:.3e}" for v in vals))
    ab_harness.finish(rows, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""GPU: what the stash-keeping reverse costs against the reverse + forward it replaces, and whether lsnf_reverse moved.

    python tools/reverse_keep_vs_forward.py [--parent-lib OTHER/liblsnf_flow.so] [--rounds 2] [--out profiles/FILE.txt]

Per batch size (100, 8 192, 16 384; default math mode and dispatch, bench.py's weights: nz 128 / w 64 / depth 5), in ONE job:
  reverse               flow.reverse(plan, eps, out=...)                                           (a) this build and the parent
  reverse_keep          the same launch with z_saved + act_saved                                   (b)
  reverse_keep+ws       ... and the parameter-gradient workspace                                   (b)
  reverse+forward       flow.reverse + flow.forward(x, z_saved, act_saved)                         (c) what the bridge does today
  reverse+forward+ws    ... the forward with the workspace too                                     (c)
  d_eps bridge          netF(eps, obj, reverse=True) and d (x . c) / d eps by autograd, `reverse_keeps_stash` False
  d_eps keeps_stash     the same with `reverse_keeps_stash` True                                   (d)
With --parent-lib (a build of the parent commit) `reverse`, `reverse+forward` and `d_eps bridge` of that build as well, in child
processes that alternate between the two libraries (LSNF_LIB_PATH), `rounds` times each.  A figure is the time per call of a window
of back-to-back calls between two device events (so it includes the launch gaps a caller sees, not only kernel time); every
(library, round) takes WINDOWS windows after a warm-up of every shape; the table gives the median with p10 / p90 over all windows
(30 per build at the default 2 rounds).  No GPU: the driver fails (there is no CPU path)."""
import json
import sys

import ab_harness
from ab_harness import pct

SIZES = (100, 8192, 16384)
WINDOWS = 15
NAMES = ("reverse", "reverse_keep", "reverse_keep+ws", "reverse+forward", "reverse+forward+ws", "d_eps bridge", "d_eps keeps_stash")

CHILD = r'''
import json, os, sys, types
import torch
import bench, lsnf_amd
parent = bool(os.environ.get("RKF_PARENT"))
if parent:                                                     # (a build from before the entry points existed)
    for name in ("lsnf_reverse_keep_covers", "lsnf_reverse_keep", "lsnf_sample_keep"):
        lsnf_amd._lib._SIGNATURES.pop(name, None)
F = lsnf_amd.flow
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
weights = [t.to(dev) for t in bench.synth_weights(1)]
plan = lsnf_amd.prepare(weights, bench.NZ, bench.WIDTH, bench.DEPTH)
hps = types.SimpleNamespace(f_n_levels=1, f_depth=bench.DEPTH, f_flow_permutation=2, f_width=bench.WIDTH, f_flow_coupling=1)
net = lsnf_amd._netF(hps, bench.NZ).to(dev)
with torch.no_grad():
    for q, t in zip(net._param_list(), weights):
        q.copy_(t.reshape(q.shape))
for q in net.parameters():
    q.requires_grad_(False)                                    # d eps alone: no parameter-gradient workspace on either path
sizes, nwin = json.loads(sys.argv[1]), int(sys.argv[2])
res = {}
for B in sizes:
    f32 = dict(dtype=torch.float32, device=dev)
    eps, x, obj, c = torch.randn(B, bench.NZ, **f32), torch.empty(B, bench.NZ, **f32), torch.empty(B, **f32), torch.randn(B, bench.NZ, **f32)
    z1, ld = torch.empty(B, bench.NZ, **f32), torch.empty(B, **f32)
    saved = torch.empty(bench.DEPTH - 1, B, bench.NZ, **f32)
    act, ws = F.new_act_saved(plan, B, dev), F.new_params_workspace(plan, B, dev)
    zero = torch.zeros(B, **f32)
    lib = lsnf_amd.load_library()
    P = lambda t: None if t is None else t.data_ptr()
    sp = torch.cuda.current_stream(dev).cuda_stream
    geo = (bench.NZ, bench.WIDTH, bench.DEPTH, 1)

    def keep(w):
        rc = lib.lsnf_reverse_keep(P(plan.buf), *geo, B, P(eps), None, P(x), P(obj), P(saved), P(act), P(w), sp)
        assert rc == 0, lib.lsnf_last_error()

    def d_eps(keeps):
        net.reverse_keeps_stash = keeps
        e = eps.detach().requires_grad_(True)
        return torch.autograd.grad((net(e, zero, reverse=True) * c).sum(), e)[0]

    fns = {"reverse": lambda: F.reverse(plan, eps, out=(x, obj)),
           "reverse+forward": lambda: (F.reverse(plan, eps, out=(x, obj)),
                                       F.forward(plan, x, want_ll=False, out=(z1, ld, None), z_saved_out=saved, act_saved=act)),
           "d_eps bridge": lambda: d_eps(False)}
    if not parent:
        fns["reverse_keep"] = lambda: keep(None)
        fns["reverse_keep+ws"] = lambda: keep(ws)
        fns["reverse+forward+ws"] = lambda: (F.reverse(plan, eps, out=(x, obj)),
                                             F.forward(plan, x, want_ll=False, out=(z1, ld, None), z_saved_out=saved, act_saved=act, params_ws=ws))
        fns["d_eps keeps_stash"] = lambda: d_eps(True)
    n = 300 if B <= 8192 else 150
    for fn in fns.values():
        for _ in range(n): fn()
    torch.cuda.synchronize()
    for name, fn in fns.items():
        res[f"{B}/{name}"] = windows(fn, n, nwin)
emit(res)
'''


def main(argv=None):
    a, libs = ab_harness.parent_lib_args(__doc__, 2, "RKF_PARENT", argv)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS)], timeout=400)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/reverse_keep_vs_forward.py: us per call, median [p10, p90] over {a.rounds} x {WINDOWS} windows per library; "
            f"nz=128 w=64 depth=5, default math mode and dispatch", f"{'B':>7} {'what':<20} {'build':<7} {'median':>9} {'p10':>9} {'p90':>9}"]
    for B in SIZES:
        for name in NAMES:
            for tag, _, _ in libs:
                ts = acc.get((tag, f"{B}/{name}"))
                if ts:
                    rows.append(f"{B:>7} {name:<20} {tag:<7} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}")
    ab_harness.finish(rows, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

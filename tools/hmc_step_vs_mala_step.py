#!/usr/bin/env python3
"""GPU: what ONE launch of the Hamiltonian Monte Carlo step costs against one launch of the Metropolis-adjusted Langevin step.

    python tools/hmc_step_vs_mala_step.py [--parent-lib OTHER/liblsnf_flow.so] [--rounds 2] [--out profiles/FILE.txt]

Per batch size (100 and 16 384; default math mode and dispatch, bench.py's weights: nz 128 / w 64 / depth 5; Philox noise, a
generator gradient and energy given, the next point written out of place so that every call sees the same rows), in ONE job, the
entry points called directly on one forward's stash -- the launch alone, no forward; every measured launch has a chain state of
its own, so its cost does not depend on what else the child measures (an accepted row stores two more rows than a rejected one):
  mala_step       lsnf_mala_step, deciding and proposing                                          this build and the parent
  hmc_inner       lsnf_hmc_step with LSNF_HMC_INNER: reads z_prop, grad_g, mom; writes mom, z_next   this build
  hmc_end         lsnf_hmc_step with flags 0, deciding and beginning the next trajectory: one more (B, nz) array read and written
                  than mala_step                                                                      this build
  hmc_init        lsnf_hmc_step with LSNF_HMC_INIT                                                    this build
With --parent-lib (a build of the parent commit) `mala_step` of that build as well, in child processes that alternate between the
two libraries (LSNF_LIB_PATH), `rounds` times each.  A figure is the time per call of a window of back-to-back calls between two
device events (so it includes the launch gaps a caller sees, not only kernel time); every (library, round) takes WINDOWS windows
after a warm-up of every shape; the table gives the median with p10 / p90 over all windows.  Below the table: each HMC launch
over this build's mala_step, and whether hmc_inner's median lies above the MALA launch's p90 (the parent's where given).  No
threshold is fixed: the file is the record.  No GPU: the driver fails (there is no CPU path)."""
import json
import sys

import ab_harness
from ab_harness import pct

SIZES = (100, 16384)
WINDOWS = 15
NAMES = ("mala_step", "hmc_inner", "hmc_end", "hmc_init")

CHILD = r'''
import json, os, sys, types
import torch
import bench, lsnf_amd
parent = bool(os.environ.get("HSM_PARENT"))
if parent:                                                     # (a build from before the entry point existed)
    lsnf_amd._lib._EXT_SIGNATURES.pop("lsnf_hmc_step", None)
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
torch.manual_seed(0)                                           # (every child times the same rows)
res = {}
plan = net._plan()
head, ptr, call = F._plan_head(plan), F._ptr, F._call
for B in sizes:
    f32 = dict(dtype=torch.float32, device=dev)
    z, gg, energy = torch.randn(B, bench.NZ, **f32), 0.1 * torch.randn(B, bench.NZ, **f32), torch.rand(B, **f32)
    act = F.new_act_saved(plan, B, dev)
    z1, _, ll, saved = F.forward(plan, z, None, want_ll=True, save_for_backward=True, act_saved=act)
    rows = lambda: torch.zeros(B, bench.NZ, **f32)
    rng = F.PhiloxNoise(1, 0, 0)
    import ctypes
    def bound(name, flags=0):
        """One measured launch with chain state, momentum and outputs of its own: what it costs does not depend on which other
        launches the child measures (an accepted row stores two more rows than a rejected one)."""
        z_acc, g_acc, u_acc, kin = z.clone(), gg.clone(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        mom, z_next, acc, la = torch.randn(B, bench.NZ, **f32), rows(), torch.zeros(B, **f32), torch.zeros(B, **f32)
        fixed = (B, ptr(z), ptr(z1), ptr(saved), ptr(act), ptr(ll), ptr(gg), ptr(energy), ptr(z_acc), ptr(g_acc), ptr(u_acc))
        keep = (z_acc, g_acc, u_acc, kin, mom, z_next, acc, la)
        def fn(keep=keep):
            if name == "lsnf_mala_step":
                call(name, dev, *head, *fixed, None, None, ctypes.byref(rng._c()), S, 0, ptr(z_next), ptr(acc), ptr(la))
            else:
                r = None if flags == 2 else ctypes.byref(rng._c())
                o = (None, None) if flags == 2 else (ptr(acc), ptr(la))
                call(name, dev, *head, *fixed, ptr(mom), ptr(kin), None, None, r, S, flags, ptr(z_next), *o)
        fn.mom = mom
        return fn
    mala, hmc = bound("lsnf_mala_step"), (lambda flags: bound("lsnf_hmc_step", flags))
    fns = {"mala_step": mala}
    if not parent:
        fns.update(hmc_inner=hmc(2), hmc_end=hmc(0), hmc_init=hmc(1))
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
    a, libs = ab_harness.parent_lib_args(__doc__, 2, "HSM_PARENT", argv)
    res = ab_harness.run(CHILD, libs, a.rounds, [json.dumps(SIZES), str(WINDOWS)], timeout=400, swap=True)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/hmc_step_vs_mala_step.py: us per launch, median [p10, p90] over {a.rounds} x {WINDOWS} windows per library; "
            f"nz=128 w=64 depth=5, default math mode and dispatch, Philox noise", f"{'B':>7} {'what':<16} {'build':<7} {'median':>9} {'p10':>9} {'p90':>9}"]
    for B in SIZES:
        for name in NAMES:
            for tag, _, _ in libs:
                ts = acc.get((tag, f"{B}/{name}"))
                if ts:
                    rows.append(f"{B:>7} {name:<16} {tag:<7} {pct(ts, 0.5):>9.2f} {pct(ts, 0.1):>9.2f} {pct(ts, 0.9):>9.2f}")
    for B in SIZES:
        mala = acc.get(("this", f"{B}/mala_step"))
        ref = acc.get(("parent", f"{B}/mala_step")) or mala
        for name in NAMES[1:]:
            ts = acc.get(("this", f"{B}/{name}"))
            if ts and mala:
                rows.append(f"# B={B}: {name} / mala_step = {pct(ts, 0.5) / pct(mala, 0.5):.3f} (medians, this build)")
        inner = acc.get(("this", f"{B}/hmc_inner"))
        if inner and ref:
            lo, hi, m = pct(ref, 0.1), pct(ref, 0.9), pct(inner, 0.5)
            which = "the parent's" if ("parent", f"{B}/mala_step") in acc else "this build's"
            rows.append(f"# B={B}: hmc_inner median {m:.2f} us is {'ABOVE' if m > hi else 'NOT ABOVE'} the p90 of {which} mala_step "
                        f"[p10 {lo:.2f}, p90 {hi:.2f}]")
    ab_harness.finish(rows, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""GPU: the twelve Hamiltonian Monte Carlo entry points of two builds of liblsnf_flow.so against each other, in one job (child
processes through tools/ab_harness.py, the library by LSNF_LIB_PATH as tools/ab_libs.py selects it): the bits, or with --time the time.

    python tools/hmc_ab_bits.py --parent-lib OTHER/liblsnf_flow.so [--out profiles/FILE.txt]            # bits
    python tools/hmc_ab_bits.py --parent-lib OTHER/liblsnf_flow.so --time [--rounds 2] [--out FILE]     # time

Bits.  Both builds make the same calls on the same inputs (seeded on the host) and every tensor a call may write is hashed (SHA-256 of
its bytes); the driver stops at the first digest that differs and returns 1.  Calls: lsnf_[reverse_]hmc_step and its _rows, _metric,
_tempered, _exchange, _resample levels; per level an INIT call, an INNER call and end calls with and without a next trajectory, the
end calls with the level's own flags (ADAPT, ADAPT | ADAPT_LAST, METRIC_FOLD | METRIC_CLOSE, ANNEAL, SWAP, SWAP | SWAP_ODD, ANNEAL |
RESAMPLE) and plain; noise and uniforms as tensors and from Philox.  Shapes: the geometry classes of tests/chain_geometries.py at
their 33 rows (and at 40 rows, five groups of 8 with a partly live workgroup, for the moves, which need B % group == 0), and one
batch size for every other <HT, WT, ST> instantiation the default dispatch reaches (tests/test_gpu_hmc.py).  The tails are fp32
without contraction: two builds of the same arithmetic agree in every bit, whatever their instruction order.

Time (--time).  bench.py's weights (nz 128 / w 64 / depth 5), 100 and 16 384 rows, Philox noise, the next point out of place: per
entry an INNER call and an end call that begins the next trajectory with the level's own flag, the launch alone on the stash of one
forward (the call construction of tools/hmc_*_vs_*.py).  A figure is the time per call of a window of back-to-back calls between two
device events; the children of the two builds alternate (the order swaps every round), every round takes 15 windows per call after a
warm-up; the table gives median [p10, p90] over all windows of a build and whether this build's median lies inside the other's own
p10..p90 (MALA section: the condition for "no slower").  The other build is measured by a second set of children as well
(`control`): how far two sets of children of ONE build lie apart in the same job.  Returns 1 if a median of this build lies above the
other's p90.  No GPU: the driver fails."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import ab_harness
import chain_geometries as G
from ab_harness import pct

LEVELS = ("scalar", "rows", "metric", "tempered", "exchange", "resample")
C3, C5, TINY = (128, 64, 5, 1), (100, 128, 5, 1), (8, 4, 5, 1)            # tests/test_gpu_reverse_keep.py's
B_MOVE = 40
# (geometry..., B): every class at its small batch; then <1, 1> at 32 and 64 rows per workgroup, <2, 2> at both, <2, 4> at 32 (its largest)
SHAPES = [c for c in G.CASES if c[4] <= 128] + [TINY + (4100,), TINY + (8200,), (66, 33, 2, 1, 4100), C3 + (8200,), C5 + (4100,)]
TIME_SIZES = (100, 16384)
WINDOWS = 15

CHILD = r'''
import ctypes, hashlib, json, sys
import torch
import lsnf_amd
from lsnf_amd._lib import LsnfDualAvg, LsnfMetricReg
F = lsnf_amd.flow
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
ptr, call = F._ptr, F._call
LEVELS = ("scalar", "rows", "metric", "tempered", "exchange", "resample")
SUFFIX = dict(zip(LEVELS, ("", "_rows", "_metric", "_tempered", "_exchange", "_resample")))
INIT, INNER, ADAPT, LAST, FOLD, CLOSE, ANNEAL, SWAP, ODD, RESAMPLE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
STEP = 0.1

class Point:
    """A batch at which the chain stands: x, eps = f(x) with the forward's stash, a generator gradient and energy."""
    def __init__(self, plan, B, seed):
        g = torch.Generator().manual_seed(seed)
        self.plan, self.B, self.nz = plan, B, plan.nz
        eps0 = torch.randn(B, plan.nz, generator=g).to(dev)
        self.gg, self.energy = (0.1 * torch.randn(B, plan.nz, generator=g)).to(dev), torch.rand(B, generator=g).to(dev)
        self.x = F.reverse(plan, eps0, None)[0]
        self.act = F.new_act_saved(plan, B, dev)
        self.eps, _, self.ll, self.saved = F.forward(plan, self.x, None, want_ll=True, save_for_backward=True, act_saved=self.act)

def bound(pt, space, level, flags, philox, propose, P, seed):
    """(fn, outs): one call of the entry with inputs of its own, and every tensor it may write by name."""
    B, nz, k = pt.B, pt.nz, LEVELS.index(level)
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    ru = lambda *s: torch.rand(*s, generator=g).to(dev)
    zeros = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    init, inner, decides = bool(flags & INIT), bool(flags & INNER), not flags & INNER
    point = pt.x if space == "z" else pt.eps
    u_prop = pt.energy - pt.ll if space == "z" else pt.energy + 0.5 * (pt.eps ** 2).sum(1)
    mom = rn(B, nz)
    o = dict(acc=point + 0.1 * rn(B, nz), grad=0.1 * rn(B, nz), u=u_prop + rn(B), mom=mom, kin=0.5 * (mom ** 2).sum(1) + rn(B),
             nxt=zeros(B, nz) if propose else None, accept=zeros(B) if decides else None, la=zeros(B) if decides else None)
    tensors = decides and not philox
    noise = rn(B, nz) if tensors and propose else None
    uniform = ru(B).clamp_min(2.0 ** -25) if tensors and not init else None
    rng = F.PhiloxNoise(1234, 40, 0) if decides and philox else None
    args = [B, ptr(pt.x), ptr(pt.eps), ptr(pt.saved), ptr(pt.act), ptr(pt.ll)] if space == "z" else [B, ptr(pt.eps), ptr(pt.saved), ptr(pt.act)]
    keep = [noise, uniform, rng]
    rc = rng._c() if rng is not None else None
    args += [ptr(pt.gg), ptr(pt.energy), ptr(o["acc"]), ptr(o["grad"]), ptr(o["u"]), ptr(o["mom"]), ptr(o["kin"]), ptr(noise), ptr(uniform),
             ctypes.byref(rc) if rc is not None else None]
    if k == 0:
        args.append(STEP)
    else:
        step = 0.05 + 0.1 * ru(B)
        o.update(step=step, adapt=torch.stack([0.1 * rn(B), 0.1 * rn(B), torch.floor(1.0 + 9.0 * ru(B)), torch.log(10.0 * step)], 1).contiguous())
        da = LsnfDualAvg(0.8, 0.05, 10.0, 0.75, 1e-4, 1e2)
        keep.append(da)
        args += [ptr(step), ptr(o["adapt"]) if flags & ADAPT else None, ctypes.byref(da) if flags & ADAPT else None]
    if k >= 2:
        o.update(scale=0.5 + ru(B, nz), mean=0.1 * rn(B, nz), m2=ru(B, nz), count=torch.floor(6.0 * ru(B)))
        reg = LsnfMetricReg(5.0, 1e-3, 1e-3, 1e3)
        keep.append(reg)
        fold = bool(flags & FOLD)
        args += [ptr(o["scale"])] + [ptr(o[n]) if fold else None for n in ("mean", "m2", "count")] + [ctypes.byref(reg) if fold else None]
    if k >= 3:
        o.update(beta=0.3 + 0.6 * ru(B), like_grad=0.1 * rn(B, nz), like_u=ru(B), log_w=torch.stack([3.0 * rn(B), zeros(B)], 1).contiguous())
        bn = o["beta"] + 0.05
        keep.append(bn)
        anneal = bool(flags & ANNEAL)
        args += [ptr(o["beta"]), ptr(bn) if anneal else None, ptr(o["like_grad"]), ptr(o["like_u"]), ptr(o["log_w"]) if anneal else None]
    args += [flags, ptr(o["nxt"]), ptr(o["accept"]), ptr(o["la"])]
    if level == "exchange":
        on = bool(flags & SWAP)
        su = ru(B).clamp_min(2.0 ** -25) if on and not philox else None
        o.update(swap=zeros(B) if on else None, log_swap=zeros(B) if on else None)
        keep.append(su)
        args += [P if on else 0, ptr(su), ptr(o["swap"]), ptr(o["log_swap"])]
    if level == "resample":
        on = bool(flags & RESAMPLE)
        rsu = ru(B) if on and not philox else None
        o.update(ancestor=zeros(B) if on else None, ess=zeros(B) if on else None)
        keep.append(rsu)
        args += [P if on else 0, 1.0 if on else 0.0, ptr(rsu), ptr(o["ancestor"]), ptr(o["ess"])]     # (ess_frac 1: some groups resample)
    name = ("lsnf_hmc_step" if space == "z" else "lsnf_reverse_hmc_step") + SUFFIX[level]
    head = F._plan_head(pt.plan)
    def fn(keep=keep, o=o):
        call(name, dev, *head, *args)
    return fn, o

def end_flags(level):
    """The end calls of a level: plain, and with its own flags."""
    return {"scalar": [0], "rows": [0, ADAPT, ADAPT | LAST], "metric": [0, FOLD | CLOSE, ADAPT | FOLD | CLOSE, ADAPT | FOLD],
            "tempered": [0, ANNEAL, ADAPT | FOLD | CLOSE | ANNEAL], "exchange": [0, ANNEAL, SWAP, SWAP | ODD],
            "resample": [0, ANNEAL, ANNEAL | RESAMPLE]}[level]

def plan_of(nz, w, depth, coupling):
    from oracle import flow_oracle as O
    p = O.init_params(nz, w, depth, seed=3)
    if coupling == 0:                                              # the additive coupling's fc_zeros: nz / 2 outputs
        p = {k: (v[:, : v.shape[1] // 2].contiguous() if ".f.fc_zeros." in k else v) for k, v in p.items()}
    return lsnf_amd.prepare(lsnf_amd.params_from_state_dict(p, depth, dev), nz, w, depth, coupling)

def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()

def bits(shapes, b_move):
    res, accepted = {}, []
    for nz, w, depth, coupling, B in shapes:
        plan = plan_of(nz, w, depth, coupling)
        for rows in ([B, b_move] if B <= 128 else [B]):
            pt = Point(plan, rows, 1000 + rows)
            P = next((p for p in (8, 16, 4, 2) if rows % p == 0), 0)
            for space in ("z", "eps"):
                for level in LEVELS:
                    moves = level in ("exchange", "resample")
                    if rows == b_move and B != b_move and not moves:
                        continue                                   # (the extra batch is for the moves alone)
                    calls = [("init", INIT, True), ("inner", INNER, True)] + [(f"end{f}", f, True) for f in end_flags(level)] + \
                            [(f"end{f}_stay", f, False) for f in end_flags(level)[-1:]]
                    if LEVELS.index(level) >= 3:
                        calls.append(("init_anneal", INIT | ANNEAL, True))
                    if rows > 128:                                 # (the instantiation is what is new here: one call per phase)
                        calls = calls[:2] + [(f"end{f}", f, True) for f in end_flags(level)[-1:]]
                    for what, flags, propose in calls:
                        if (flags & (SWAP | RESAMPLE)) and not P:
                            continue                               # (33 rows hold no whole group)
                        for philox in ((False,) if flags & INNER else (True,) if rows > 128 else (False, True)):
                            fn, o = bound(pt, space, level, flags, philox, propose, P, seed=7 + len(res))
                            fn()
                            torch.cuda.synchronize()
                            key = f"{nz}x{w}x{depth}c{coupling} B{rows} {space} {level} {what} {'philox' if philox else 'tensors'}"
                            res[key] = {n: sha(t) for n, t in o.items() if t is not None}
                            if o["accept"] is not None and not flags & INIT:
                                accepted.append(float(o["accept"].mean()))
    res["_accept_rate_min_mean_max"] = [min(accepted), sum(accepted) / len(accepted), max(accepted)]
    return res

def times(sizes, nwin):
    import bench
    plan = lsnf_amd.prepare([t.to(dev) for t in bench.synth_weights(1)], bench.NZ, bench.WIDTH, bench.DEPTH)
    own = dict(scalar=0, rows=ADAPT, metric=ADAPT | FOLD, tempered=ANNEAL, exchange=SWAP, resample=ANNEAL | RESAMPLE)
    res = {}
    for B in sizes:
        pt = Point(plan, B, 1000 + B)
        P = 16 if B % 16 == 0 else 4
        fns = {}
        for space in ("z", "eps"):
            for level in LEVELS:
                key = ("hmc_" if space == "z" else "rhmc_") + level
                fns[f"{key}_inner"] = bound(pt, space, level, INNER, False, True, P, seed=11)
                fns[f"{key}_end"] = bound(pt, space, level, own[level], True, True, P, seed=12)
        n = 300 if B <= 8192 else 150
        for fn, _ in fns.values():
            for _ in range(n): fn()
        torch.cuda.synchronize()
        for name, (fn, o) in fns.items():
            ts = []
            for _ in range(nwin):
                o["mom"].normal_()                                 # (every call replaces mom: the same scale for every window)
                if "log_w" in o:
                    o["log_w"][:, 0].normal_(0.0, 3.0); o["log_w"][:, 1].zero_()      # (and the weights' spread)
                ts += windows(fn, n, 1)
            res[f"{B}/{name}"] = ts
    return res

torch.manual_seed(0)
emit(bits(json.loads(sys.argv[2]), int(sys.argv[3])) if sys.argv[1] == "bits" else times(json.loads(sys.argv[2]), int(sys.argv[3])))
'''


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    builds = [("this", None, {}), ("parent", a.parent_lib, {})]
    if not a.time:
        res = ab_harness.run(CHILD, builds, 1, ["bits", json.dumps(SHAPES), str(B_MOVE)], timeout=900,
                             ok=lambda tag, r, p: f"{tag}: {len(p) - 1} calls, {sum(len(v) for k, v in p.items() if k[0] != '_')} tensors")
        if res is None:
            return 1
        this, parent = res["this"][0], res["parent"][0]
        rate = this.pop("_accept_rate_min_mean_max"); parent.pop("_accept_rate_min_mean_max")
        rows = [f"# tools/hmc_ab_bits.py: SHA-256 of every tensor a call may write, this build against the build of --parent-lib",
                f"# {len(this)} calls; accepted share of the end calls: min {rate[0]:.2f}, mean {rate[1]:.2f}, max {rate[2]:.2f}"]
        if this.keys() != parent.keys():
            print("the two builds made different calls")
            return 1
        per = {}
        for key in this:
            for name in this[key]:
                if this[key][name] != parent[key].get(name):
                    print(f"MISMATCH at {key}: {name}\n  this   {this[key][name]}\n  parent {parent[key].get(name)}")
                    return 1
            space, level = key.split()[2:4]
            n = per.setdefault((space, level), [0, 0])
            n[0] += 1; n[1] += len(this[key])
        rows += [f"{'space':<6} {'level':<10} {'calls':>6} {'tensors':>8}   identical"] + \
                [f"{s:<6} {l:<10} {c:>6} {t:>8}   yes" for (s, l), (c, t) in per.items()]
        ab_harness.finish(rows, a.out)
        return 0
    builds.append(("control", a.parent_lib, {}))                     # the other build a second time: what two sets of children of ONE build differ by
    res = ab_harness.run(CHILD, builds, a.rounds, ["time", json.dumps(TIME_SIZES), str(WINDOWS)], timeout=900, swap=True)
    if res is None:
        return 1
    acc = ab_harness.pooled(res)
    rows = [f"# tools/hmc_ab_bits.py --time: us per launch, median [p10, p90] over {a.rounds} x {WINDOWS} windows per build, the builds' children "
            f"alternating; nz=128 w=64 depth=5, default math mode and dispatch",
            f"{'B':>6} {'call':<22} {'this':>8} {'p10':>8} {'p90':>8} {'parent':>8} {'p10':>8} {'p90':>8}  {'this in p10..p90':<16} {'control':>8}  control in p10..p90"]
    bad = bad_control = 0
    for (tag, key), ts in acc.items():
        if tag != "this":
            continue
        ref = acc[("parent", key)]
        B, name = key.split("/")
        m, lo, hi = pct(ts, 0.5), pct(ref, 0.1), pct(ref, 0.9)
        verdict = lambda v: "yes" if lo <= v <= hi else "below (faster)" if v < lo else "ABOVE"
        c = pct(acc[("control", key)], 0.5)
        bad += (m > hi); bad_control += (c > hi)
        rows.append(f"{B:>6} {name:<22} {m:>8.2f} {pct(ts, 0.1):>8.2f} {pct(ts, 0.9):>8.2f} {pct(ref, 0.5):>8.2f} {lo:>8.2f} {hi:>8.2f}  "
                    f"{verdict(m):<16} {c:>8.2f}  {verdict(c)}")
    rows.append(f"# medians above the parent's p90: this build {bad} of {len(rows) - 2}, the parent's own second set of children {bad_control}")
    ab_harness.finish(rows, a.out)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

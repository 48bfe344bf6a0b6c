#!/usr/bin/env python3
"""GPU: host cost of a call through the library's launch layer, two builds against each other in one job.

    python tools/host_cost_launch.py parent.so new.so [rounds=6]
    python tools/host_cost_launch.py PARENT_CHECKOUT NEW_CHECKOUT [rounds=6]

An argument is a build of liblsnf_flow.so (run under this checkout's Python, LSNF_LIB_PATH) or a checkout directory: the child
then runs with that directory as its working directory -- that tree's Python layer and that tree's built library.
The builds alternate in fresh child processes, the order within a pair swapped from round to round (use an
even number of rounds: a build against a copy of itself shows the second child of a pair ~0.1-0.5 us slower).  A child times the ENQUEUE of eleven calls -- no synchronisation
inside a timed region, as tools/host_rate.py -- in REGIONS regions of CALLS calls each (queue drained between regions):
  forward(B=64), forward(B=64, stash), langevin_step(B=100), sample(B=100), BoundForward(B=8192),
  backward_z(B=100), reverse_backward_z(B=100), backward_params(B=100, reuse_buffers) -- these three from the forward's stash --,
  mala_step(B=100), reverse_mala_step(B=100) from that stash, hmc_step(B=100, phase="inner").
Per build and call: median and p10 / p90 over every region of every round, and the medians of the rounds.  The first build is
the reference: the second one's median may exceed its median by at most the reference's own p10-p90 width; exit status 1 if
a call does."""
import os
import statistics
import sys

import ab_harness

REGIONS, CALLS = 15, 300
NAMES = ("forward B=64", "forward B=64 +stash", "langevin_step B=100", "sample B=100", "BoundForward B=8192",
         "backward_z B=100", "reverse_backward_z B=100", "backward_params B=100",
         "mala_step B=100", "reverse_mala_step B=100", "hmc_step inner B=100")

CHILD = r'''
import os, sys, time, torch
import bench, lsnf_amd
F = lsnf_amd.flow
REGIONS, CALLS = int(sys.argv[1]), int(sys.argv[2])
dev = torch.device("cuda:0")
params = [t.to(dev) for t in bench.synth_weights(1)]
plan = lsnf_amd.prepare(params, bench.NZ, bench.WIDTH, bench.DEPTH)
gen = torch.Generator().manual_seed(1234)
f32 = dict(dtype=torch.float32, device=dev)
def outs(B): return (torch.empty(B, bench.NZ, **f32), torch.empty(B, **f32), torch.empty(B, **f32))
z64, z100, z8k = (torch.randn(B, bench.NZ, generator=gen).to(dev) for B in (64, 100, 8192))
o64, o8k = outs(64), outs(8192)
act64 = F.new_act_saved(plan, 64, dev)
sav64 = torch.empty((bench.DEPTH - 1, 64, bench.NZ), **f32)
rng = F.PhiloxNoise(7)
smp_out = (torch.empty(100, bench.NZ, **f32), torch.empty(100, **f32), None, None)
bound = F.BoundForward(plan, z8k, o8k)
act100, ws100 = F.new_act_saved(plan, 100, dev), F.new_params_workspace(plan, 100, dev)
z1, _, _, sav100 = F.forward(plan, z100, save_for_backward=True, act_saved=act100, params_ws=ws100)
gz, gld = torch.randn(100, bench.NZ, generator=gen).to(dev), torch.randn(100, generator=gen).to(dev)
mala, rmala, hmc = F.new_mala_state(plan, 100, dev), F.new_mala_state(plan, 100, dev), F.new_hmc_state(plan, 100, dev)
zm, zh = z100.clone(), z100.clone()
F.mala_step(plan, zm, None, None, mala, rng, 0.1, init=True, propose=False)
F.reverse_mala_step(plan, z1, sav100, act100, None, None, rmala, rng, 0.1, init=True, propose=False)
F.hmc_step(plan, zh, None, None, hmc, rng, 0.1, phase="init", inplace=True, reuse_buffers=True)
calls = (
    lambda: F.forward(plan, z64, out=o64),
    lambda: F.forward(plan, z64, out=o64, act_saved=act64, z_saved_out=sav64),
    lambda: F.langevin_step(plan, z100, None, rng, 0.1, inplace=True, reuse_buffers=True),
    lambda: F.sample(plan, 100, rng, out=smp_out),
    lambda: bound(None),
    lambda: F.backward_z(plan, z1, sav100, gz, gld, act_saved=act100),
    lambda: F.reverse_backward_z(plan, z1, sav100, act100, gz, gld),
    lambda: F.backward_params(plan, params, z100, z1, sav100, gz, gld, reuse_buffers=True, act_saved=act100, workspace=ws100),
    lambda: F.mala_step(plan, zm, None, None, mala, rng, 0.1, inplace=True, reuse_buffers=True),
    lambda: F.reverse_mala_step(plan, z1, sav100, act100, None, None, rmala, rng, 0.1, propose=False, reuse_buffers=True),
    lambda: F.hmc_step(plan, zh, None, None, hmc, None, 1e-3, phase="inner", inplace=True, reuse_buffers=True),
)
res = []
for fn in calls:
    for _ in range(CALLS): fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(REGIONS):
        t0 = time.perf_counter()
        for _ in range(CALLS): fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        us.append(1e6 * (t1 - t0) / CALLS)
    res.append(us)
emit(res)
'''


def pct(xs, q):
    xs = sorted(xs)
    k = q * (len(xs) - 1)
    lo = int(k)
    return xs[lo] + (xs[min(lo + 1, len(xs) - 1)] - xs[lo]) * (k - lo)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    libs = [os.path.abspath(p) for p in argv[:2]]
    rounds = int(argv[2]) if len(argv) > 2 else 6
    # the order within a pair is swapped from round to round: whichever child runs second in a pair measures ~0.3 us more
    res = ab_harness.run(CHILD, [(lib, lib, {}) for lib in libs], rounds, [str(REGIONS), str(CALLS)], timeout=280, swap=True,
                         ok=lambda lib, r, _: f"round {r} {lib}: done")
    if res is None:
        return 2
    # per build and call: every region of every round, and the medians of the rounds
    regions = {lib: [sum((rnd[i] for rnd in res[lib]), []) for i in range(len(NAMES))] for lib in libs}
    round_medians = {lib: [[statistics.median(rnd[i]) for rnd in res[lib]] for i in range(len(NAMES))] for lib in libs}
    print(f"\nenqueue-only host time, us per call ({rounds} rounds per build, alternating; {REGIONS} regions x {CALLS} calls per round)")
    print(f"reference: {libs[0]}\nnew:       {libs[1]}")
    print(f"{'call':<26} {'build':<10} {'median':>8} {'p10':>8} {'p90':>8}   medians of the rounds")
    bad = 0
    for i, name in enumerate(NAMES):
        stat = {}
        for tag, lib in zip(("reference", "new"), libs):
            xs = regions[lib][i]
            stat[tag] = (statistics.median(xs), pct(xs, 0.1), pct(xs, 0.9))
            print(f"{name:<26} {tag:<10} {stat[tag][0]:8.2f} {stat[tag][1]:8.2f} {stat[tag][2]:8.2f}   "
                  + " ".join("%.2f" % m for m in round_medians[lib][i]))
        width = stat["reference"][2] - stat["reference"][1]
        delta = stat["new"][0] - stat["reference"][0]
        ok = delta <= width
        bad += not ok
        print(f"{'':<26} new - reference median {delta:+.2f} us; allowed +{width:.2f} (the reference's p10-p90 width): {'ok' if ok else 'SLOWER'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

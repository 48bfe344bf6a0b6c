#!/usr/bin/env python3
"""GPU: the headline benchmark itself (`python bench.py`, default arguments) under several builds of liblsnf_flow.so in one job:
fresh child processes, the builds alternating round by round (LSNF_LIB_PATH), every child under its own time limit, nothing
started after the first child that fails.  The first round also dumps each build's outputs (`--dump-outputs`) and the driver
compares them with the first build's: z1, logdet, ll bit for bit, the sums to 1e-9.

    ab_bench_libs.py [--rounds 6] [--out FILE] [--dump-dir DIR] parent=path/liblsnf_flow.so tree= ...     (empty path: the in-tree library)

Per build: every run's ms/step, min / median / max; per build after the first: the ratio of medians to the first build, whether
EVERY run beat EVERY run of the first build, and the noise bound 1 - 2 x (first max - first min) / first median."""
import argparse
import os
import sys

import ab_harness

CHILD = r'''
import contextlib, io, runpy
sys.argv = ["bench.py"] + sys.argv[1:]
buf = io.StringIO()
with contextlib.redirect_stdout(buf):
    runpy.run_path("bench.py", run_name="__main__")
line = json.loads(buf.getvalue().strip().splitlines()[-1])
emit({"ms_per_step": line["ms_per_step"]})
'''


def same_outputs(a, b):
    """None, or what differs between two --dump-outputs directories."""
    import numpy as np
    for name in ("z1", "logdet", "ll"):
        x, y = np.load(os.path.join(a, name + ".npy")), np.load(os.path.join(b, name + ".npy"))
        if x.shape != y.shape or not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
            return f"{name}: {int((x.view(np.uint32) != y.view(np.uint32)).sum()) if x.shape == y.shape else 'shape'} differing"
    sa, sb = np.load(os.path.join(a, "sums.npy")), np.load(os.path.join(b, "sums.npy"))
    if sa.shape != sb.shape or not np.all(np.abs(sa - sb) <= 1e-9 * np.abs(sa)):
        return f"sums: {sa} vs {sb}"
    return None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump-dir", default=None, help="round 0 runs with --dump-outputs DIR/<tag>; the outputs are compared")
    ap.add_argument("builds", nargs="+", metavar="tag=lib")
    a = ap.parse_args(argv)
    builds = []
    for spec in a.builds:
        tag, _, lib = spec.partition("=")
        builds.append((tag, lib or None, {}))
    rows = []
    runs = {tag: [] for tag, _, _ in builds}

    def note(line):                        # what a child returned: printed as it comes, and part of the record
        rows.append(line)
        return line
    if a.dump_dir:
        for tag, lib, env in builds:       # (one child per build: its dump directory is an argument of the child)
            r = ab_harness.run(CHILD, [(tag, lib, env)], 1, argv=("--dump-outputs", os.path.join(a.dump_dir, tag)), timeout=240,
                               ok=lambda t, r_, p: note(f"{t} dump run: {p['ms_per_step'] * 1e3:.2f} us/step"))
            if r is None:
                ab_harness.finish(rows, a.out)
                return 1
        first = builds[0][0]
        for tag, _, _ in builds[1:]:
            why = same_outputs(os.path.join(a.dump_dir, first), os.path.join(a.dump_dir, tag))
            rows.append(f"outputs {tag} vs {first}: " + ("z1, logdet, ll bit-identical, sums equal to 1e-9" if why is None else "DIFFER -- " + why))
            if why is not None:
                ab_harness.finish(rows, a.out)
                return 1
    res = ab_harness.run(CHILD, builds, a.rounds, timeout=240, swap=True,
                         ok=lambda t, r_, p: note(f"{t} round {r_}: {p['ms_per_step'] * 1e3:.2f} us/step"))
    if res is None:
        ab_harness.finish(rows, a.out)
        return 1
    for tag in runs:
        runs[tag] = [p["ms_per_step"] * 1e3 for p in res[tag]]
    first = builds[0][0]
    f = sorted(runs[first])
    fmed = ab_harness.pct(f, 0.5)
    bound = 1.0 - 2.0 * (f[-1] - f[0]) / fmed
    rows.append(f"bench.py default arguments, us/step, {a.rounds} alternating rounds in one job")
    for tag, v in runs.items():
        s = sorted(v)
        med = ab_harness.pct(s, 0.5)
        row = f"{tag:12s} min {s[0]:.2f} median {med:.2f} max {s[-1]:.2f}   runs " + " ".join(f"{x:.2f}" for x in v)
        if tag != first:
            row += f"\n{'':12s} median / {first} median {med / fmed:.4f}; every run beats every {first} run: {s[-1] < f[0]}; below the noise bound {bound:.4f}: {med / fmed < bound}"
        rows.append(row)
    ab_harness.finish(rows, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Do two runs of one workload launch the same kernels?  From the kernel traces of `rocprofv3 --kernel-trace` (one run per
build of liblsnf_flow.so, LSNF_LIB_PATH):

    python tools/trace_same_kernels.py TRACE_DIR_A TRACE_DIR_B [--csv OUT.csv]

Every *kernel_trace.csv under a directory is read (one per traced process, in the order the processes started), its rows put
in dispatch order.  Compared: the per-kernel call counts of every kernel, and the ordered sequence of the library's kernel
names (`lsnf_*`; the framework's own kernels depend on which process ran a library's find step first).  --csv writes the
call-count table of both runs.  Exit status 1 on any difference."""
import argparse
import collections
import csv
import glob
import os
import sys


def launches(trace_dir):
    files = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows = list(csv.DictReader(open(path)))
        if rows:
            rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
            files.append((min(int(r["Start_Timestamp"]) for r in rows), [r["Kernel_Name"] for r in rows]))
    files.sort(key=lambda f: f[0])
    return [name for _, names in files for name in names]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace_a")
    ap.add_argument("trace_b")
    ap.add_argument("--csv", default=None)
    a = ap.parse_args()
    la, lb = launches(a.trace_a), launches(a.trace_b)
    ca, cb = collections.Counter(la), collections.Counter(lb)
    names = sorted(set(ca) | set(cb))
    if a.csv:
        with open(a.csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["kernel", "calls_a", "calls_b"])
            for n in names:
                w.writerow([n, ca[n], cb[n]])
    mine = [n for n in names if "lsnf_" in n]
    diff_all = [n for n in names if ca[n] != cb[n]]
    diff_mine = [n for n in diff_all if n in mine]
    sa, sb = [n for n in la if "lsnf_" in n], [n for n in lb if "lsnf_" in n]
    first = next((i for i, (x, y) in enumerate(zip(sa, sb)) if x != y), None)
    same_seq = first is None and len(sa) == len(sb)
    print(f"launches: {len(la)} / {len(lb)}; kernels: {len(names)}, the library's: {len(mine)} ({len(sa)} / {len(sb)} launches)")
    print(f"call counts: the library's kernels {'identical' if not diff_mine else 'DIFFER: ' + '; '.join(diff_mine[:5])}; "
          f"every kernel {'identical' if not diff_all else 'differ in ' + str(len(diff_all)) + ' (' + '; '.join(n[:60] for n in diff_all[:3]) + ')'}")
    print(f"ordered sequence of the library's kernel names: {'identical' if same_seq else 'DIFFERS at launch ' + str(first)}")
    return 0 if same_seq and not diff_mine and sa else 1


if __name__ == "__main__":
    sys.exit(main())

"""The one place that starts measurement children: builds of the library against each other in one job, one fresh child process
at a time, each with a time limit, and nothing more started after the first child that fails.

    res = run(BODY, [("this", None, {}), ("parent", "other/liblsnf_flow.so", {"X_PARENT": "1"})], rounds=2, timeout=400)
    if res is None: return 1                     # a child failed: run() has reported it and has started nothing since

A build is (tag, target, extra_env).  target None: the in-tree library; a file: LSNF_LIB_PATH=<its absolute path>, this checkout as
working directory; a directory: that checkout as working directory with its own built library (its Python layer too).
The child runs PRELUDE + BODY: PRELUDE is source text and no module, because a child whose working directory is another checkout
imports that tree's modules, which need not have this file.  This module never imports torch: the driver does not hold the GPU
while its children are timed."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = "AB_RESULT "

PRELUDE = r'''
import json, os, sys, time
sys.path.insert(0, os.getcwd())

def windows(fn, n, windows, host=False):
    """`windows` windows of n back-to-back calls of fn between two device events: the us per call of each window.  host=True:
    (those, the host-clock us per call the same windows took to issue).  The caller warms up."""
    import torch
    dev_us, host_us = [], []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(n): fn()
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        dev_us.append(e0.elapsed_time(e1) / n * 1e3)
        host_us.append((t1 - t0) / n * 1e6)
    return (dev_us, host_us) if host else dev_us

def emit(obj):
    """The child's result line: what run() hands back to the driver."""
    print("AB_RESULT " + json.dumps(obj), flush=True)
'''


def child_env(target, extra_env):
    """(cwd, environment) of the child that measures `target`."""
    env = dict(os.environ, **extra_env)
    if target is None:
        return ROOT, env
    target = os.path.abspath(target)
    if os.path.isdir(target):
        return target, dict(env, LSNF_LIB_PATH=os.path.join(target, "latent-space-normalizing-flow_amd", "liblsnf_flow.so"))
    return ROOT, dict(env, LSNF_LIB_PATH=target)


def run(body, builds, rounds=1, argv=(), timeout=280, swap=False, ok=lambda tag, r, payload: f"{tag} round {r}: ok"):
    """Every build once per round, in order (swap: reversed in odd rounds), one child alive at a time.  Returns {tag: [payload per
    round]}, or None as soon as a child hit its time limit, returned non-zero or printed no result line.  `ok` is the line
    printed after a child that succeeded."""
    res = {tag: [] for tag, _, _ in builds}
    assert len(res) == len(builds), "two builds with one tag"
    for r in range(rounds):
        for tag, target, extra_env in (builds[::-1] if swap and r % 2 else builds):
            cwd, env = child_env(target, extra_env)
            try:
                out = subprocess.run([sys.executable, "-c", PRELUDE + body, *argv], cwd=cwd, env=env,
                                     capture_output=True, text=True, timeout=timeout)
                line = [l for l in out.stdout.splitlines() if l.startswith(MARK)]
                why = None
                err = out.stderr
                if out.returncode:
                    why = f"exit {out.returncode}"
                elif not line:
                    why = "exit 0, no result line"
            except subprocess.TimeoutExpired as e:
                why = f"time limit {timeout} s"
                err = e.stderr or ""
                if isinstance(err, bytes):
                    err = err.decode(errors="replace")
            if why:
                print(f"{tag} round {r}: FAILED ({why})\n{err[-2000:]}", flush=True)
                return None                           # nothing more is started after a failure
            res[tag].append(json.loads(line[-1][len(MARK):]))
            print(ok(tag, r, res[tag][-1]), flush=True)
    return res


def parent_lib_args(doc, rounds, parent_env, argv=None):
    """The command line of the drivers that time this tree and, with --parent-lib, a build of the parent commit (whose children
    get `parent_env` set): (arguments, builds)."""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=rounds)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    return a, [("this", None, {})] + ([("parent", a.parent_lib, {parent_env: "1"})] if a.parent_lib else [])


def pooled(res):
    """{(tag, key): the windows of every round} from children that each emit {key: [windows]}."""
    acc = {}
    for tag, payloads in res.items():
        for payload in payloads:
            for k, ts in payload.items():
                acc.setdefault((tag, k), []).extend(ts)
    return acc


def pct(v, q):
    """Nearest-rank percentile."""
    v = sorted(v)
    return v[min(len(v) - 1, max(0, int(round(q * (len(v) - 1)))))]


def finish(rows, out=None):
    """Print the table and, with `out`, write it there (the directory is created)."""
    text = "\n".join(rows) + "\n"
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)

"""Which of the built kernel instantiations does a traced run launch?  (No GPU needed: the traces come from one.)

    python tools/kernel_coverage.py BUILD_DIR STATS.csv [STATS.csv ...] [--calls-csv OUT.csv]

BUILD_DIR: the objects of a build (csrc/_build); every `__global__` instantiation in them is listed from the code objects' metadata
by tools/kernel_resources.py, under its short names `kernel<HT, WT, ...>`.  STATS.csv: the `*_kernel_stats.csv` files that
`rocprofv3 --kernel-trace --stats --output-format csv -- COMMAND` wrote (one per traced process; columns "Name", "Calls"), or a
reduced table of this directory's `profiles/*_kernel_calls.csv` kind (columns "kernel", "calls").  The traces' demangled names are
brought to the same short form and the calls of all files are added up.  Three lists are printed:

    launched          built instantiations with their call counts
    never launched    built instantiations that no traced process ran
    unmatched         names of the library's kernels (`lsnf_*`) in a trace that are no built instantiation

The third list must be empty: an entry means that the two name forms disagree (or that the trace is of another build), and the
exit status is then 1.  --calls-csv writes `kernel,calls` for the library's kernels in the short form."""
import argparse
import collections
import csv
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources  # noqa: E402

_VALUE = re.compile(r"(?:\([^()]*\))?(-?\d+|true|false)(?:[uU]?[lL]{0,2})$")


def _template_args(s, lt):
    """The text between the `<` at s[lt] and its matching `>`."""
    depth = 0
    for i in range(lt, len(s)):
        if s[i] in "<(":
            depth += 1
        elif s[i] in ">)":
            depth -= 1
            if depth == 0:
                return s[lt + 1:i]
    return s[lt + 1:]


def _values(args):
    """Integer and boolean template arguments in order; a class argument (`Cfg<2, 4>`) contributes its own."""
    out, depth, cur = [], 0, ""
    for ch in args + ",":
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        if ch == "," and depth == 0:
            tok = cur.strip()
            m = _VALUE.match(tok)
            if m:                                      # (`(bool)1`: the form some demanglers give a boolean argument)
                out.append(("true" if m.group(1) != "0" else "false") if tok.startswith("(bool)") else m.group(1))
            elif "<" in tok:
                out.extend(_values(_template_args(tok, tok.index("<"))))
            cur = ""
        else:
            cur += ch
    return out


def short_name(demangled):
    """`void (anonymous namespace)::lsnf_rev_kernel<(anonymous namespace)::RevCfg<1, 1>, 8, true>((anonymous namespace)::RevArgs)`
    -> `lsnf_rev_kernel<1, 1, 8, true>`, the form of kernel_resources._short; a name without `lsnf_` is returned as it is."""
    s = demangled.strip()
    if s.endswith(".kd"):
        s = s[:-3]
    m = re.search(r"\blsnf_\w+", s)
    if not m:
        return s
    vals = _values(_template_args(s, m.end())) if s[m.end():m.end() + 1] == "<" else []
    return f"{m.group(0)}<{', '.join(vals)}>" if vals else m.group(0)


def read_calls(paths):
    """{short name: calls} over all files (the library's kernels in the short form, every other kernel under its own name)."""
    calls = collections.Counter()
    for path in paths:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("kernel") or row.get("Kernel_Name")
                n = row.get("Calls") or row.get("calls") or "1"
                if name:
                    calls[short_name(name)] += int(n)
    return calls


def ledger(built, calls):
    """(launched {name: calls}, never launched [names], unmatched {name: calls}) for the built short names and the calls of a trace."""
    built = set(built)
    launched = {n: calls[n] for n in sorted(built) if calls.get(n, 0) > 0}
    never = sorted(n for n in built if n not in launched)
    unmatched = {n: c for n, c in sorted(calls.items()) if "lsnf_" in n and n not in built and c > 0}
    return launched, never, unmatched


def render(launched, never, unmatched, n_files):
    lines = [f"{len(launched) + len(never)} built instantiations, {len(launched)} launched, {len(never)} never launched; "
             f"{n_files} kernel-stats file(s)", "", f"launched ({len(launched)}): calls  kernel"]
    lines += [f"{c:>10}  {n}" for n, c in launched.items()]
    lines += ["", f"never launched ({len(never)}):"] + [f"            {n}" for n in never]
    lines += ["", f"unmatched names of the traces ({len(unmatched)}; must be none):"] + [f"{c:>10}  {n}" for n, c in unmatched.items()]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("build_dir")
    ap.add_argument("stats", nargs="+", help="kernel-stats CSVs of rocprofv3 (or reduced kernel,calls tables)")
    ap.add_argument("--calls-csv", default=None, help="write kernel,calls of the library's kernels (short names) here")
    a = ap.parse_args()
    built = kernel_resources.collect(a.build_dir, "")
    if not built:
        sys.exit(f"no kernels found in the objects of {a.build_dir}")
    calls = read_calls(a.stats)
    launched, never, unmatched = ledger(built, calls)
    print(render(launched, never, unmatched, len(a.stats)))
    if a.calls_csv:
        with open(a.calls_csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["kernel", "calls"])
            for n, c in sorted(calls.items()):
                if "lsnf_" in n:
                    w.writerow([n, c])
    return 1 if unmatched else 0


if __name__ == "__main__":
    sys.exit(main())

"""Resource notes of the kernels in built objects, from the code objects' own metadata (no GPU needed).

    python tools/kernel_resources.py BUILD_DIR [--match rev] [--against OTHER_BUILD_DIR] [--sha256]

For every *.o in BUILD_DIR: the gfx950 code object is taken out of the .hip_fatbin section and its AMDGPU metadata note
is read (llvm-readelf --notes): VGPRs, AGPRs, SGPRs, static LDS and Scratch_Size (.private_segment_fixed_size) per kernel.
Kernel names are shortened to `kernel<HT, WT, ...>` (the template arguments in order).  --against compares with a second build (e.g. the
parent commit's): a kernel is matched by its name with any trailing `false` template argument removed, so that an
instantiation that gained a compile-time flag is compared with what it was; kernels only in BUILD_DIR are listed as new.
Exit status 1 if a matched kernel differs in VGPRs, AGPRs, LDS or scratch.
--sha256 adds, below the table, the SHA-256 of every object's gfx950 code object: with --against, exit status 1 as well if any
object's device code differs by a single byte (or exists on one side only) -- the check of a host-only change."""
import argparse
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"),
          ("scratch", ".private_segment_fixed_size"))


def _run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def _short(mangled):
    """`_ZN12_GLOBAL__N_115lsnf_rev_kernelINS_6RevCfgILi1ELi1EEELi8ELb1EEEv...` -> `lsnf_rev_kernel<1, 1, 8, true>`: the kernel's
    name and the integer / boolean template arguments in order (the Cfg<HT, WT> class contributes its two)."""
    m = re.search(r"(\d\d)(lsnf_\w+)", mangled)          # (kernel names have 10..99 characters)
    if not m:
        return mangled
    name = m.group(2)[: int(m.group(1))]
    rest = mangled[m.start(2) + int(m.group(1)):]
    # (`...ILi32EEv...` of a kernel outside a namespace: the split takes the last argument's own `E` with it, so it is put back)
    targs = rest.split("EEv", 1)[0] + "E" if rest.startswith("I") else ""
    vals = [v if k == "i" else ("true" if v == "1" else "false") for k, v in re.findall(r"L([ib])(\d+)E", targs)]
    return f"{name}<{', '.join(vals)}>" if vals else name


def _code_object(obj, tmp):
    """Path of the gfx950 code object of one object file, unbundled into tmp; None for an object without device code."""
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    try:
        _run(os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj)
    except subprocess.CalledProcessError:
        return None
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    _run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
         f"--input={fat}", f"--output={co}")
    return co


def device_hashes(build_dir, match):
    """{object file name: (sha256 of its gfx950 code object, its size)}."""
    res = {}
    for obj in sorted(glob.glob(os.path.join(build_dir, "*.o"))):
        if match and match not in os.path.basename(obj):
            continue
        with tempfile.TemporaryDirectory() as tmp:
            co = _code_object(obj, tmp)
            data = open(co, "rb").read() if co else b""
            res[os.path.basename(obj)] = (hashlib.sha256(data).hexdigest() if co else "(host code only)", len(data))
    return res


def print_hashes(mine, theirs):
    """The hash table; the number of objects whose device code differs from `theirs` (None: nothing to compare with)."""
    bad = 0
    print(f"\n{'object':<24} {'bytes':>9}  sha256 of the gfx950 code object")
    for n in sorted(set(mine) | set(theirs or {})):
        h, size = mine.get(n, ("-" * 64, 0))
        verdict = ""
        if theirs is not None:
            same = n in mine and n in theirs and theirs[n][0] == h
            bad += not same
            verdict = "   identical" if same else "   DIFFERENT"
        print(f"{n:<24} {size:>9}  {h}{verdict}")
    if theirs is not None:
        print(f"{len(mine)} objects, {bad} with different device code")
    return bad


def kernels_of(obj):
    """{short name: {vgpr, agpr, sgpr, lds, scratch}} of one object file."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        co = _code_object(obj, tmp)
        if co is None:
            return out
        notes = _run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
    cur = None
    for line in notes.splitlines():
        s = line.strip()
        if s.startswith("- ") and (line.startswith("  - ") or cur is None):      # a new entry of the kernels' list: not an
            # argument or a `.language_version` item, which sit deeper and would drop the fields read so far (AGPRs, LDS)
            if cur and ".name" in cur and ".vgpr_count" in cur:
                out[_short(cur[".name"])] = {k: int(cur.get(f, 0)) for k, f in FIELDS}
            cur, s = {}, s[2:].strip()
        if cur is not None and ":" in s:
            k, v = s.split(":", 1)
            if k in (".name",) or k in [f for _, f in FIELDS]:
                if k != ".name" or v.strip().startswith("_Z"):
                    cur[k] = v.strip()
    if cur and ".name" in cur and ".vgpr_count" in cur:
        out[_short(cur[".name"])] = {k: int(cur.get(f, 0)) for k, f in FIELDS}
    return out


def collect(build_dir, match):
    res = {}
    for obj in sorted(glob.glob(os.path.join(build_dir, "*.o"))):
        if match and match not in os.path.basename(obj):
            continue
        res.update(kernels_of(obj))
    return res


def _base(name):
    while name.endswith(", false>"):                                     # (a kernel may have gained several flags at once)
        name = name[: -len(", false>")] + ">"
    return re.sub(r"<false>$", "", name)                                 # (`kernel<false>` was plain `kernel`)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("build_dir")
    ap.add_argument("--match", default="", help="only objects whose file name contains this")
    ap.add_argument("--against", default=None, help="a second build directory to compare with")
    ap.add_argument("--sha256", action="store_true", help="also hash every object's gfx950 code object (byte identity)")
    a = ap.parse_args()
    mine = collect(a.build_dir, a.match)
    if a.against is None:
        print(f"{'kernel':<70} {'VGPR':>5} {'AGPR':>5} {'SGPR':>5} {'LDS':>6} {'scratch':>7}")
        for n, r in sorted(mine.items()):
            print(f"{n:<70} {r['vgpr']:>5} {r['agpr']:>5} {r['sgpr']:>5} {r['lds']:>6} {r['scratch']:>7}")
        if a.sha256:
            print_hashes(device_hashes(a.build_dir, a.match), None)
        return 0
    theirs = collect(a.against, a.match)
    bad = 0
    print(f"{'kernel':<70} {'VGPR':>9} {'AGPR':>9} {'LDS':>9} {'scratch':>9}")
    for n, r in sorted(mine.items()):
        o = theirs.get(n) or theirs.get(_base(n))
        if o is None:
            print(f"{n:<70} {r['vgpr']:>9} {r['agpr']:>9} {r['lds']:>9} {r['scratch']:>9}   new")
            continue
        same = all(r[k] == o[k] for k in ("vgpr", "agpr", "lds", "scratch"))
        bad += not same
        cell = lambda k: f"{o[k]}->{r[k]}" if o[k] != r[k] else f"{r[k]}"
        print(f"{n:<70} {cell('vgpr'):>9} {cell('agpr'):>9} {cell('lds'):>9} {cell('scratch'):>9}   {'same' if same else 'CHANGED'}")
    gone = [n for n in theirs if n not in mine and not any(_base(m) == n for m in mine)]
    for n in sorted(gone):
        print(f"{n:<70} only in {a.against}")
    if a.sha256:
        bad += print_hashes(device_hashes(a.build_dir, a.match), device_hashes(a.against, a.match))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

"""Build-time macros and environment variables of the kernels, lexically (no compiler, no GPU).  A knob stays only if every value it
accepts computes the documented result and something in the tree uses it: the environment variables are exactly those of
INTEGRATION.md's "Environment knobs" table, the preprocessor tests only macros of the allow-list below, and no tool passes a -D
macro that the sources do not test."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "latent-space-normalizing-flow_amd", "csrc")
TOOLS = os.path.join(ROOT, "tools")

# diagnostic build with correct results (the per-phase cycle tables), the Makefile's product builds, the default latency threshold
MACROS = {"LSNF_STAMPS", "LSNF_L16_PARTS", "LSNF_FWD3_ENTRY", "LSNF_REV3_ENTRY", "LSNF_BWD3_WIDE_TU", "LSNF_SMALL_MAX_DEFAULT", "__HIPCC__"}
SAME = "every value computes the same documented result"


def sources():
    return {p: open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))}


def macros_the_sources_test():
    """identifiers in the conditions of #if / #ifdef / #ifndef / #elif"""
    names = set()
    for text in sources().values():
        for cond in re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", text, re.M):
            names |= set(re.findall(r"[A-Za-z_]\w*", cond.split("//")[0])) - {"defined"}
    return names


def test_environment_knobs_are_the_documented_table():
    read = set()
    for text in sources().values():
        read |= set(re.findall(r'getenv\(\s*"(LSNF_\w+)"', text))
        assert len(re.findall(r"getenv\(", text)) == len(re.findall(r'getenv\(\s*"LSNF_\w+"\s*\)', text))      # (no computed names)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = doc.split("## 4. Environment knobs", 1)[1].split("\n## ", 1)[0]
    rows = [[c.strip() for c in l.strip().strip("|").split("|")] for l in table.splitlines() if l.startswith("| `")]
    assert all(len(r) == 3 and r[1] and r[2] == SAME for r in rows), rows
    listed = [r[0].strip("`") for r in rows]
    assert len(listed) == len(set(listed))
    assert read and set(listed) == read


def test_preprocessor_tests_only_the_allowed_macros():
    tested = macros_the_sources_test()
    assert "LSNF_STAMPS" in tested                      # (the scan finds something)
    assert tested <= MACROS, sorted(tested - MACROS)


def test_tools_define_only_macros_the_sources_test():
    tested, passed = macros_the_sources_test(), {}
    for dirpath, dirnames, files in os.walk(TOOLS):
        dirnames[:] = [d for d in dirnames if not (dirpath == TOOLS and d == "micro") and d != "__pycache__"]
        for f in files:
            try:
                text = open(os.path.join(dirpath, f)).read()
            except UnicodeDecodeError:
                continue
            for name in re.findall(r"(?<![\w-])-D([A-Za-z_]\w*)", text):
                passed.setdefault(name, f)
    assert "LSNF_STAMPS" in passed
    assert set(passed) <= tested, {n: f for n, f in passed.items() if n not in tested}

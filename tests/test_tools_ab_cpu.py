"""tools/ab_harness.py without a GPU: the children here are a few lines of plain Python that write to a log file.  The harness starts
one child at a time in the order asked for, hands each build its library / checkout / environment, stops at the first child that
fails (exit status, no result line, time limit) so that the driver exits non-zero, never imports torch, and every ported
driver's child compiles behind the prelude."""
import importlib
import os
import subprocess
import sys

import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
sys.path.insert(0, TOOLS)
import ab_harness  # noqa: E402

PARENT_LIB = ("sample_vs_randn_reverse", "reverse_keep_vs_forward", "reverse_langevin_vs_unfused", "mle_step_vs_torch_adam")
TWO_LIBS = ("host_cost_launch", "ab_libs", "ab_secondary", "ab_fwd_sizes")
NO_ARGS = ("waves_c5", "tn_probe")
DRIVERS = PARENT_LIB + TWO_LIBS + NO_ARGS

# A child: checks that no earlier child is still alive (every "start" in the log has its "done"), logs its start, misbehaves if it
# is child number AB_FAIL_AT (counting from 0), else logs "done" and emits what it was given.
BODY = r'''
log, tag = os.environ["AB_LOG"], os.environ.get("AB_TAG", "?")
lines = open(log).read().split() if os.path.exists(log) else []
assert lines.count("start") == lines.count("done"), "the previous child has not finished"
with open(log, "a") as f: f.write("start %s\n" % tag)
if str(lines.count("start")) == os.environ.get("AB_FAIL_AT"):
    kind = os.environ["AB_FAIL"]
    if kind == "exit": sys.exit(3)
    if kind == "sleep": time.sleep(60)
    if kind == "silent": sys.exit(0)
with open(log, "a") as f: f.write("done %s\n" % tag)
emit({"tag": tag, "cwd": os.getcwd(), "lib": os.environ.get("LSNF_LIB_PATH"), "knob": os.environ.get("AB_KNOB"), "argv": sys.argv[1:]})
'''


def started(log):
    return [l.split()[1] for l in open(log).read().splitlines() if l.startswith("start")]


@pytest.fixture
def log(tmp_path, monkeypatch):
    path = str(tmp_path / "log.txt")
    monkeypatch.setenv("AB_LOG", path)
    return path


@pytest.mark.parametrize("swap, order", [(False, "a b a b a b"), (True, "a b b a a b")])
def test_order_one_child_at_a_time(log, capsys, swap, order):
    res = ab_harness.run(BODY, [("a", None, {"AB_TAG": "a"}), ("b", None, {"AB_TAG": "b"})], rounds=3, argv=["x", "7"], timeout=60, swap=swap)
    assert " ".join(started(log)) == order
    assert open(log).read().split().count("done") == 6          # (each child asserted that its predecessors had finished)
    assert [[p["tag"] for p in res[t]] for t in "ab"] == [["a"] * 3, ["b"] * 3]          # payloads per tag, in round order
    assert res["a"][0]["argv"] == ["x", "7"]
    ok = [l for l in capsys.readouterr().out.splitlines() if l.endswith(": ok")]
    assert ok == [f"{t} round {r}: ok" for r in range(3) for t in (("b", "a") if swap and r % 2 else ("a", "b"))]


def test_targets(log, tmp_path, monkeypatch):
    (tmp_path / "libs").mkdir()
    (tmp_path / "libs" / "other.so").write_bytes(b"")
    checkout = tmp_path / "checkout"
    checkout.mkdir()
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("LSNF_LIB_PATH", "the-caller's")
    builds = [("none", None, {}), ("so", os.path.join("libs", "other.so"), {"AB_KNOB": "1"}), ("dir", str(checkout), {})]
    res = ab_harness.run(BODY, builds, timeout=60)
    none, so, d = (res[t][0] for t in ("none", "so", "dir"))
    assert (none["cwd"], none["lib"], none["knob"]) == (ab_harness.ROOT, "the-caller's", None)
    assert (so["cwd"], so["lib"], so["knob"]) == (ab_harness.ROOT, str(tmp_path / "libs" / "other.so"), "1")
    assert os.path.isabs(so["lib"])
    assert (d["cwd"], d["lib"]) == (str(checkout), str(checkout / "latent-space-normalizing-flow_amd" / "liblsnf_flow.so"))
    monkeypatch.delenv("LSNF_LIB_PATH")
    assert ab_harness.run(BODY, builds[:1], timeout=60)["none"][0]["lib"] is None


DRIVER = r'''
import sys
sys.path.insert(0, sys.argv[1])
import ab_harness
res = ab_harness.run(sys.argv[2], [("a", None, {"AB_TAG": "a"}), ("b", None, {"AB_TAG": "b"})], rounds=3, timeout=float(sys.argv[3]))
sys.exit(1 if res is None else 0)
'''


@pytest.mark.parametrize("at", [1, 2], ids=["first-round", "second-round"])
@pytest.mark.parametrize("kind, why", [("exit", "exit 3"), ("silent", "no result line"), ("sleep", "time limit")])
def test_stops_at_the_first_failed_child(log, monkeypatch, kind, why, at):
    monkeypatch.setenv("AB_FAIL", kind)
    monkeypatch.setenv("AB_FAIL_AT", str(at))
    limit = "1" if kind == "sleep" else "60"
    out = subprocess.run([sys.executable, "-c", DRIVER, TOOLS, BODY, limit], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1, out.stderr                       # the driver exits non-zero, and without a traceback
    assert "Traceback" not in out.stderr
    tag, r = "ab"[at % 2], at // 2
    assert f"{tag} round {r}: FAILED" in out.stdout and why in out.stdout
    assert out.stdout.count(": ok") == at
    assert started(log) == list("abab")[:at + 1]                 # the failed child is the last one that was started
    assert open(log).read().split().count("done") == at


@pytest.mark.parametrize("name", DRIVERS)
def test_every_driver_stops_at_its_first_failed_child(log, monkeypatch, capsys, name):
    driver = importlib.import_module(name)
    monkeypatch.setattr(driver, "CHILD", BODY)
    monkeypatch.setenv("AB_FAIL", "exit")
    monkeypatch.setenv("AB_FAIL_AT", "0")
    argv = ["--parent-lib", "p.so"] if name in PARENT_LIB else ["a.so", "b.so"] if name in TWO_LIBS else []
    assert driver.main(argv) in (1, 2)
    assert "FAILED (exit 3)" in capsys.readouterr().out
    assert len(started(log)) == 1


def test_no_torch_in_the_driver():
    code = "import sys; sys.path.insert(0, %r)\nimport ab_harness, %s\nassert 'torch' not in sys.modules" % (TOOLS, ", ".join(DRIVERS))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


def test_pct_is_nearest_rank():
    pct = ab_harness.pct
    assert [pct([5.0], q) for q in (0.1, 0.5, 0.9)] == [5.0, 5.0, 5.0]
    assert [pct([2, 1], q) for q in (0.1, 0.5, 0.9)] == [1, 1, 2]          # (round-half-even: rank 0.5 is the lower one)
    assert pct([3, 1, 2], 0.5) == 2
    v15, v30 = list(range(15, 0, -1)), list(range(1, 31))           # the drivers' 15 and 30 windows
    assert [pct(v15, q) for q in (0.1, 0.5, 0.9)] == [2, 8, 14]
    assert [pct(v30, q) for q in (0.1, 0.5, 0.9)] == [4, 15, 27]
    for name in PARENT_LIB:                                         # one definition: theirs is the harness's
        assert importlib.import_module(name).pct is pct


def test_prelude_and_every_body_compile():
    compile(ab_harness.PRELUDE, "PRELUDE", "exec")
    for name in DRIVERS:
        compile(ab_harness.PRELUDE + importlib.import_module(name).CHILD, name, "exec")


def test_tags_are_unique_and_pooled_takes_every_round():
    with pytest.raises(AssertionError):
        ab_harness.run(BODY, [("a", None, {}), ("a", "other.so", {})])          # (refused before any child is started)
    res = {"this": [{"x": [1, 2]}, {"x": [3], "y": [4]}], "parent": [{"x": [5]}, {"x": [6]}]}
    assert ab_harness.pooled(res) == {("this", "x"): [1, 2, 3], ("this", "y"): [4], ("parent", "x"): [5, 6]}

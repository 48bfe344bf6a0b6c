"""The pipelined bf16x3 forward (lsnf_fwd3p.hip) after its issue-slot work -- one-instruction ReLU, one statement and one 64-bit
add per weight chunk -- in its paired form
(LSNF_FWD3Q_SHAPE=242) and its 8-wave form (82):

  * against the latency forward (the default small-batch dispatch, which does not run lsnf_fwd3p.hip): z1 bit for bit -- a row's
    z1 does not depend on the kernel family the batch size selects; logdet and ll differ across the families in their last bits on
    the parent build too (test_equals_latency_forward), so they are held to the other form and to float64.  The depth-1 and depth-2
    stacks are the shortest calls: the trailing weight fetch comes right behind the prologue;
  * the same at padded geometries (nz 100 / width 40, nz 66), and every case against the float64 oracle;
  * a row of NaN and a row of +-inf in z: those rows come out non-finite, every other row bit-equal to the call without them;
  * three calls on one stats buffer: the sums are those of the arrays each call wrote, to 1e-9.

The shape knob is read once per process, so each form runs in a fresh child process under its own `timeout`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL_REL_F64 = 2e-6      # tests/test_gpu_fwd3q_pair.py: the bf16x3 forward's log-prob against float64
Z_ABS = 1e-4           # ... and z1 against the oracle
SUMS_REL = 1e-9        # the project's figure for the in-kernel sums
BAD_NAN, BAD_INF = 5, 70           # rows of the "nonfinite" case's second call

# name -> (B, nz, f_width, depth, kind): kind "" one call; "stats" objective + three calls on one stats buffer; "nonfinite" a clean
# call and the same z with row BAD_NAN all NaN and row BAD_INF alternating +-inf
CASES = {
    "a_B33": (33, 128, 64, 5, ""),
    "a_B129": (129, 128, 64, 5, ""),
    "a_B257": (257, 128, 64, 5, ""),
    "b_depth1": (129, 128, 64, 1, ""),
    "b_depth2": (129, 128, 64, 2, ""),
    "c_nz100_w40": (129, 100, 40, 5, ""),
    "c_nz66": (129, 66, 64, 5, ""),
    "d_nonfinite": (129, 128, 64, 5, "nonfinite"),
    "e_stats_x3": (257, 128, 64, 5, "stats"),
}
PLAIN = [n for n in sorted(CASES) if CASES[n][4] == ""]
FORMS = ("242", "82")


def case_inputs(name):
    """Seeded parameters and the (z, objective) of every call of the case, as CPU tensors: children and oracle build the same ones."""
    B, nz, width, depth, kind = CASES[name]
    seed = 2000 + sorted(CASES).index(name)
    p = O.init_params(nz, width, depth, seed=seed)
    calls = []
    for i in range(3 if kind == "stats" else 1):
        g = torch.Generator().manual_seed(10 * seed + i)
        z = 1.5 * torch.randn(B, nz, generator=g)
        calls.append((z, torch.randn(B, generator=g) if kind == "stats" else None))
    if kind == "nonfinite":
        z = calls[0][0].clone()
        z[BAD_NAN] = float("nan")
        z[BAD_INF] = float("inf") * (1.0 - 2.0 * (torch.arange(nz) % 2))
        calls.append((z, None))
    return p, calls


CHILD = r'''
import os, sys
root, out, small = sys.argv[1], sys.argv[2], sys.argv[3] == "small"
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np, torch
import lsnf_amd
import test_gpu_fwd3q_issue_slots as T
dev = torch.device("cuda:0")
F = lsnf_amd.flow
F.set_math_mode(F.MATH_BF16X3)
if not small:
    F.set_small_batch_max(0)
res = {}
for name, (B, nz, width, depth, kind) in T.CASES.items():
    p, calls = T.case_inputs(name)
    plan = lsnf_amd.prepare(lsnf_amd.params_from_state_dict(p, depth, dev), nz, width, depth)
    stats = F.new_stats(dev)
    for i, (z, obj) in enumerate(calls):
        z1, ld, ll, _ = lsnf_amd.forward(plan, z.to(dev), None if obj is None else obj.to(dev), stats=stats)
        torch.cuda.synchronize()
        res[f"{name}/{i}/z1"], res[f"{name}/{i}/logdet"], res[f"{name}/{i}/ll"] = z1.cpu().numpy(), ld.cpu().numpy(), ll.cpu().numpy()
        res[f"{name}/{i}/sums"] = stats[4:7].cpu().numpy()
np.savez(out, **res)
print("child ok", sys.argv[3])
'''


@pytest.fixture(scope="module")
def forms(gpu_device, tmp_path_factory):
    """{"small" | shape code: arrays of every case}, from one fresh child process each."""
    d = tmp_path_factory.mktemp("fwd3q_issue_slots")
    got = {}
    for code in ("small",) + FORMS:
        out = str(d / f"form_{code}.npz")
        env = dict(os.environ)
        env.pop("LSNF_SMALL_MAX", None)
        if code != "small":
            env["LSNF_FWD3Q_SHAPE"] = code
        r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD, ROOT, out, code], env=env, capture_output=True, text=True)
        assert r.returncode == 0, f"child {code} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        got[code] = dict(np.load(out))
    return got


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("code", FORMS)
@pytest.mark.parametrize("name", PLAIN)
def test_equals_latency_forward(forms, name, code):
    """z1 bit for bit.  logdet and ll are NOT bit-equal across the two kernel families, on the parent build of this file exactly as
    on this one (measured in one job, both builds: 17 / 71 / 149 of 33 / 129 / 257 rows differ in logdet, 85 and 59 at depth 1 and
    2, 67 and 73 at the padded geometries, the same counts for 242 and 82 -- the families sum a row's log terms in different
    orders).  So those two arrays are held bit for bit to the OTHER form of the same family here, to the latency forward within the
    reordering bound worked out below, and to the float64 oracle at the
    tolerances of tests/test_gpu_fwd3q_pair.py in test_meets_float64_oracle, every case."""
    new, ref = forms[code], forms["small"]
    a, b = new[f"{name}/0/z1"], ref[f"{name}/0/z1"]
    assert bits_equal(a, b), (name, code, "z1", int((a.view(np.uint32) != b.view(np.uint32)).sum()) if a.shape == b.shape else "shape")
    other = forms[FORMS[1 - FORMS.index(code)]]
    # Against the latency forward, a bound from the arithmetic alone: both families add the same fp32 terms, in another order.
    # logdet is a sum of N = depth x (half + 2) terms (a log-sigmoid per coupled feature, two constants per block), so two orders
    # differ by at most 2 N u x sum |terms| (u = 2^-24); the log-sigmoids are all <= 0, so sum |terms| is |logdet| but for the
    # constants: max(1, |logdet|) stands for it.  ll = -0.5 sum z1^2 + const + logdet adds the nz squares' sum (z1 is bit-equal:
    # 2 nz u x 0.5 sum z1^2) and three roundings of its own (4 u |ll|).
    B, nz, width, depth, _ = CASES[name]
    u = 2.0 ** -24
    ld = ref[f"{name}/0/logdet"].astype(np.float64)
    ss = (ref[f"{name}/0/z1"].astype(np.float64) ** 2).sum(axis=1)
    tol_ld = 2.0 * depth * (nz // 2 + 2) * u * np.maximum(1.0, np.abs(ld))
    tol = {"logdet": tol_ld, "ll": tol_ld + 2.0 * nz * u * 0.5 * ss + 4.0 * u * np.abs(ref[f"{name}/0/ll"].astype(np.float64))}
    for arr in ("logdet", "ll"):
        assert bits_equal(new[f"{name}/0/{arr}"], other[f"{name}/0/{arr}"]), (name, code, arr)
        d = np.abs(new[f"{name}/0/{arr}"].astype(np.float64) - ref[f"{name}/0/{arr}"].astype(np.float64))
        print(name, code, arr, "max abs difference to the latency forward", d.max(), "largest share of its bound", (d / tol[arr]).max())
        assert np.all(d <= tol[arr]), (name, code, arr, d.max(), (d / tol[arr]).max())


@pytest.fixture(scope="module")
def oracle64():
    """{case: [(z1, ll) in float64 per call]}, evaluated once."""
    ref = {}
    for name in CASES:
        if CASES[name][4] == "nonfinite":
            continue
        p, calls = case_inputs(name)
        p64 = O.to_dtype(p, torch.float64)
        ref[name] = []
        for z, obj in calls:
            z1r, ldr = O.flow_forward(p64, z.double(), torch.zeros(z.shape[0], dtype=torch.float64) if obj is None else obj.double())
            ref[name].append((z1r, O.log_prob(z1r, ldr)))
    return ref


@pytest.mark.parametrize("code", FORMS)
@pytest.mark.parametrize("name", [n for n in sorted(CASES) if CASES[n][4] != "nonfinite"])
def test_meets_float64_oracle(forms, oracle64, name, code):
    for i, (z1r, llr) in enumerate(oracle64[name]):
        ll, z1 = torch.from_numpy(forms[code][f"{name}/{i}/ll"]).double(), torch.from_numpy(forms[code][f"{name}/{i}/z1"]).double()
        err_ll = ((ll - llr).abs() / llr.abs().clamp_min(1.0)).max().item()
        err_z = (z1 - z1r).abs().max().item()
        print(name, code, i, "ll rel", err_ll, "z1 abs", err_z)
        assert err_ll <= LL_REL_F64, (name, code, i, err_ll)
        assert err_z <= Z_ABS * max(1.0, z1r.abs().max().item()), (name, code, i, err_z)


@pytest.mark.parametrize("code", FORMS)
def test_nonfinite_rows_stay_in_their_rows(forms, code):
    got = forms[code]
    clean = {arr: got[f"d_nonfinite/0/{arr}"] for arr in ("z1", "logdet", "ll")}
    bad = {arr: got[f"d_nonfinite/1/{arr}"] for arr in ("z1", "logdet", "ll")}
    for r in (BAD_NAN, BAD_INF):
        assert not np.isfinite(bad["z1"][r]).any(), (code, r, "z1")
        assert not np.isfinite(bad["ll"][r]), (code, r, "ll")
    keep = np.ones(CASES["d_nonfinite"][0], dtype=bool)
    keep[[BAD_NAN, BAD_INF]] = False
    for arr in ("z1", "logdet", "ll"):
        assert np.isfinite(clean[arr]).all(), (code, arr)
        assert bits_equal(bad[arr][keep], clean[arr][keep]), (code, arr)


@pytest.mark.parametrize("code", FORMS)
def test_sums_of_three_calls_on_one_stats_buffer(forms, code):
    got = forms[code]
    B = CASES["e_stats_x3"][0]
    for i in range(3):
        s = got[f"e_stats_x3/{i}/sums"]
        ll, ld = got[f"e_stats_x3/{i}/ll"].astype(np.float64).sum(), got[f"e_stats_x3/{i}/logdet"].astype(np.float64).sum()
        print(code, i, "sums", s, ll, ld)
        assert s[2] == B
        assert abs(s[0] - ll) <= SUMS_REL * abs(ll) and abs(s[1] - ld) <= SUMS_REL * abs(ld), (code, i, s, ll, ld)

"""The CU-sharing form of the pipelined bf16x3 forward (lsnf_fwd3p.hip, LSNF_FWD3Q_SHAPE=242: two 4-wave workgroups per CU, half
the weight ring, 8-step half-phases) against the 8-wave form (82), which keeps the same per-wave arithmetic: z1, logdet and ll bit
for bit, the in-kernel sums to 1e-9, and the new form against the float64 oracle.

The shape knob is read once per process, so each form runs in a fresh child process (under its own `timeout`) that makes the same
seeded calls and saves what they returned; the float64 oracle is evaluated once, here."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL_REL_F64 = 2e-6      # tests/test_gpu_forward.py::test_split_bf16_is_fp32_faithful: the bf16x3 forward's log-prob against float64
Z_ABS = 1e-4           # tests/test_gpu_forward.py: z1 against the oracle
SUMS_REL = 1e-9        # the project's figure for the in-kernel sums

# name -> (B, nz, f_width, depth, objective and three calls on one stats buffer)
CASES = {
    "a_B1": (1, 128, 64, 5, False),            # waves and sample tiles past the batch
    "a_B33": (33, 128, 64, 5, False),
    "b_B127": (127, 128, 64, 5, False),        # the workgroup boundary
    "b_B128": (128, 128, 64, 5, False),
    "b_B129": (129, 128, 64, 5, False),
    "c_B257": (257, 128, 64, 5, False),        # three workgroups, two of them co-resident
    "d_depth1": (129, 128, 64, 1, False),      # the trailing re-fetch with 4 phases
    "d_depth2": (129, 128, 64, 2, False),      # ... and with 8
    "e_nz100_w40": (129, 100, 40, 5, False),   # padded halves, vec4 path
    "f_nz66": (129, 66, 64, 5, False),         # vec2 path
    "g_stats_x3": (257, 128, 64, 5, True),     # objective and stats given, three calls on one stats buffer: the slots re-arm
}


def case_inputs(name):
    """Seeded parameters and the inputs of every call of the case (CPU tensors): the children and the oracle build the same ones."""
    B, nz, width, depth, three = CASES[name]
    seed = 1000 + sorted(CASES).index(name)
    p = O.init_params(nz, width, depth, seed=seed)
    calls = []
    for i in range(3 if three else 1):
        g = torch.Generator().manual_seed(10 * seed + i)
        z = 1.5 * torch.randn(B, nz, generator=g)
        obj = torch.randn(B, generator=g) if three else None
        calls.append((z, obj))
    return p, calls


CHILD = r'''
import os, sys
root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np, torch
import lsnf_amd
import test_gpu_fwd3q_pair as T
dev = torch.device("cuda:0")
F = lsnf_amd.flow
F.set_small_batch_max(0); F.set_math_mode(F.MATH_BF16X3)
res = {}
for name, (B, nz, width, depth, three) in T.CASES.items():
    p, calls = T.case_inputs(name)
    plan = lsnf_amd.prepare(lsnf_amd.params_from_state_dict(p, depth, dev), nz, width, depth)
    stats = F.new_stats(dev)
    for i, (z, obj) in enumerate(calls):
        z1, ld, ll, _ = lsnf_amd.forward(plan, z.to(dev), None if obj is None else obj.to(dev), stats=stats)
        torch.cuda.synchronize()
        res[f"{name}/{i}/z1"], res[f"{name}/{i}/logdet"], res[f"{name}/{i}/ll"] = z1.cpu().numpy(), ld.cpu().numpy(), ll.cpu().numpy()
        res[f"{name}/{i}/sums"] = stats[4:7].cpu().numpy()
np.savez(out, **res)
print("child ok", os.environ.get("LSNF_FWD3Q_SHAPE"))
'''


@pytest.fixture(scope="module")
def forms(gpu_device, tmp_path_factory):
    """{shape code: arrays of every case}, from one fresh child process per form."""
    d = tmp_path_factory.mktemp("fwd3q_pair")
    got = {}
    for code in ("242", "82"):
        out = str(d / f"form_{code}.npz")
        r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD, ROOT, out],
                           env=dict(os.environ, LSNF_FWD3Q_SHAPE=code), capture_output=True, text=True)
        assert r.returncode == 0, f"child for LSNF_FWD3Q_SHAPE={code} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        got[code] = dict(np.load(out))
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_pair_form_equals_eight_wave_form(forms, name):
    new, old = forms["242"], forms["82"]
    for i in range(3 if CASES[name][4] else 1):
        for arr in ("z1", "logdet", "ll"):
            a, b = new[f"{name}/{i}/{arr}"], old[f"{name}/{i}/{arr}"]
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, i, arr)
        sa, sb = new[f"{name}/{i}/sums"], old[f"{name}/{i}/sums"]
        print(name, i, "sums", sa, sb)
        assert sa[2] == sb[2] == CASES[name][0]
        assert np.all(np.abs(sa[:2] - sb[:2]) <= SUMS_REL * np.abs(sb[:2])), (name, i, sa, sb)
        # and the sums are those of the arrays the same call wrote
        ll, ld = new[f"{name}/{i}/ll"].astype(np.float64).sum(), new[f"{name}/{i}/logdet"].astype(np.float64).sum()
        assert abs(sa[0] - ll) <= SUMS_REL * abs(ll) + 1e-9 and abs(sa[1] - ld) <= SUMS_REL * abs(ld) + 1e-9, (name, i, sa, ll, ld)


@pytest.mark.parametrize("name", sorted(CASES))
def test_pair_form_meets_float64_oracle(forms, name):
    new = forms["242"]
    p, calls = case_inputs(name)
    p64 = O.to_dtype(p, torch.float64)
    for i, (z, obj) in enumerate(calls):
        o64 = torch.zeros(z.shape[0], dtype=torch.float64) if obj is None else obj.double()
        z1r, ldr = O.flow_forward(p64, z.double(), o64)
        llr = O.log_prob(z1r, ldr)
        ll, z1 = torch.from_numpy(new[f"{name}/{i}/ll"]).double(), torch.from_numpy(new[f"{name}/{i}/z1"]).double()
        err_ll = ((ll - llr).abs() / llr.abs().clamp_min(1.0)).max().item()
        err_z = (z1 - z1r).abs().max().item()
        print(name, i, "ll rel", err_ll, "z1 abs", err_z)
        assert err_ll <= LL_REL_F64, (name, i, err_ll)
        assert err_z <= Z_ABS * max(1.0, z1r.abs().max().item()), (name, i, err_z)

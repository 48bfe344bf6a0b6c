"""GPU: `bench.py` as the benchmark driver calls it -- a plain run times exactly K steps and prints the headline only;
`--dump-outputs DIR` writes what the last timed step computed, and those arrays are the flow's outputs on the seeded
inputs (checked against the oracle); `--full` adds the figures beside the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step(gpu_device, tmp_path):
    import bench
    import lsnf_amd
    d = _bench("--steps", "7", "--warmup", "2", "--ramp", "4", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 7 and d["timed_regions"] == 1 and d["ms_per_step"] > 0
    assert d["unit"] == "latent-samples/s" and d["higher_is_better"] is True and d["dtype"] == "bf16x3"
    for key in ("roofline", "cpu_baseline", "ms_per_step_single_stream"):
        assert key not in d
    out = {n: np.load(tmp_path / f"{n}.npy") for n in ("z1", "logdet", "ll", "sums")}
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert out["z1"].shape == (bench.B_GLOBAL, bench.NZ) and out["z1"].dtype == np.float32
    assert out["ll"].shape == out["logdet"].shape == (bench.B_GLOBAL,) and out["sums"].dtype == np.float64
    # the seeded inputs of bench.py, sampled rows against the oracle
    w = bench.synth_weights(1)
    p = {}
    for i in range(bench.DEPTH):
        for j, k in enumerate(lsnf_amd.flow.BLOCK_PARAM_KEYS):
            t = w[i * 12 + j]
            p[O.block_prefix(i) + k] = t.reshape(1, -1) if t.dim() == 1 else t
    z = torch.randn(bench.B_GLOBAL, bench.NZ, generator=torch.Generator().manual_seed(1234))
    idx = torch.arange(0, bench.B_GLOBAL, 331)
    z1r, ldr, llr = O.flow_log_prob(p, z[idx])
    assert (np.abs(out["ll"][idx.numpy()] - llr.numpy()) / np.abs(llr.numpy())).max() <= 1e-5
    assert np.abs(out["z1"][idx.numpy()] - z1r.numpy()).max() <= 1e-4
    # the in-kernel sums of the same step
    assert out["sums"][2] == bench.B_GLOBAL
    assert abs(out["sums"][0] - out["ll"].astype(np.float64).sum()) <= 1e-6 * abs(out["sums"][0])
    assert abs(out["sums"][1] - out["logdet"].astype(np.float64).sum()) <= 1e-6 * abs(out["sums"][1])


def test_full_run_reports_the_extra_figures(gpu_device):
    d = _bench("--steps", "5", "--warmup", "1", "--ramp", "4", "--reps", "2", "--full", "--no-cpu-baseline")
    assert d["steps"] == 5 and d["timed_regions"] == 2
    assert d["roofline"]["kernel_ms"] > 0 and d["ms_per_step_single_stream"] > 0
    assert set(d["config"]["other_math_modes"]) == {"fp32", "fp16x2"}

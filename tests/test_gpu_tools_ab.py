"""GPU: tools/ab_harness.py end to end with real children -- the prelude's `windows` and `emit` around one small forward, the in-tree
library once as it is and once named through LSNF_LIB_PATH."""
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

BODY = r'''
import torch, bench, lsnf_amd
dev = torch.device("cuda:0")
plan = lsnf_amd.prepare([t.to(dev) for t in bench.synth_weights(1)], bench.NZ, bench.WIDTH, bench.DEPTH)
z = torch.randn(16, bench.NZ, device=dev)
fn = lambda: lsnf_amd.flow.forward(plan, z)
fn()
torch.cuda.synchronize()
emit(windows(fn, n=20, windows=2))
'''


def test_two_builds_through_the_harness(gpu_device):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import ab_harness
    lib = os.path.join(ab_harness.ROOT, "latent-space-normalizing-flow_amd", "liblsnf_flow.so")
    res = ab_harness.run(BODY, [("a", None, {}), ("b", lib, {})], rounds=1, timeout=120)
    assert res is not None and sorted(res) == ["a", "b"]
    for tag in "ab":
        (ts,) = res[tag]
        assert len(ts) == 2 and all(math.isfinite(t) and t > 0 for t in ts), (tag, ts)

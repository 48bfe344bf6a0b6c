"""Cost of the data-dependent actnorm init (`flow.actnorm_init`) at nz=128, width=64, depth=5: a few calls at B = 100 and at
B = 65 536, for a `rocprofv3 --kernel-trace --stats` run (the per-kernel sums of one call are the init's cost), plus
HIP-event wall times of one call per batch size.

    rocprofv3 --kernel-trace --stats -d OUT -o init -- python3 tools/init_cost.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lsnf_amd  # noqa: E402
from oracle import flow_oracle as O  # noqa: E402

nz, width, depth, reps = 128, 64, 5, 5
dev = torch.device("cuda:0")
p = O.init_params(nz, width, depth, seed=1, fcz_std=0.1)
for B in (100, 65536):
    z = (3.0 * torch.rand(nz) + torch.randn(B, nz, generator=torch.Generator().manual_seed(B))).to(dev)
    params = lsnf_amd.params_from_state_dict(p, depth, dev)
    ws = torch.empty(lsnf_amd.flow.actnorm_init_workspace_bytes(nz, width, depth, 1, B) // 4 + 4, device=dev)
    lsnf_amd.flow.actnorm_init(params, z, nz, width, depth, 1, workspace=ws)          # warm-up (module load)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        lsnf_amd.flow.actnorm_init(params, z, nz, width, depth, 1, workspace=ws)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    print(f"B={B}: actnorm_init {min(times):.3f} ms min / {sorted(times)[reps // 2]:.3f} ms median of {reps} (HIP events)")

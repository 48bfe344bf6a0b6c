"""GPU experiment: time of the batch contraction of lsnf_params.hip at B = 65 536 by samples per workgroup and by kernel (env knobs
LSNF_TN_CHUNK / LSNF_TN_PLAIN, one subprocess each; every row computes the same gradients)."""
import sys

import ab_harness

CHILD = r'''
import os, sys, types, numpy as np, torch
import lsnf_amd
from lsnf_amd import flow
dev = torch.device("cuda:0")
hps = types.SimpleNamespace(f_n_levels=1, f_depth=5, f_flow_permutation=2, f_width=64, f_flow_coupling=1)
torch.manual_seed(1); np.random.seed(1)
net = lsnf_amd._netF(hps, nz=128).to(dev); plan = net._plan(); params = [p.detach() for p in net._param_list()]
B = 65536
z = torch.randn(B, 128, device=dev)
act = flow.new_act_saved(plan, B, dev); ws = flow.new_params_workspace(plan, B, dev)
z1, _, _, saved = flow.forward(plan, z, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
def run(): flow.backward_params(plan, params, z, z1, saved, ll_scale=-1.0 / B, reuse_buffers=True, act_saved=act, workspace=ws)
for _ in range(10): run()
torch.cuda.synchronize()
emit("%.1f us" % windows(run, 30, 1)[0])
'''
BUILDS = (("lds kernel", {}),
          ("lds, chunk 512", {"LSNF_TN_CHUNK": "512"}), ("lds, chunk 2048", {"LSNF_TN_CHUNK": "2048"}), ("lds, chunk 4096", {"LSNF_TN_CHUNK": "4096"}),
          ("plain kernel", {"LSNF_TN_PLAIN": "1"}), ("plain, chunk 512", {"LSNF_TN_PLAIN": "1", "LSNF_TN_CHUNK": "512"}))


def main(argv=None):
    res = ab_harness.run(CHILD, [(name, None, env) for name, env in BUILDS], timeout=200,
                         ok=lambda name, r, t: f"{name:36s} backward_params (fast path, total) {t}")
    return 1 if res is None else 0


if __name__ == "__main__":
    sys.exit(main())

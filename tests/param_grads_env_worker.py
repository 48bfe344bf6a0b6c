"""The child of tests/test_gpu_param_grads_oracle.py::test_library_ignores_LSNF_TN_ABL (a FRESH process: the library reads its
environment knobs once per process, at the first call).  For every batch size on the command line: the recomputing path of
`flow.backward_params` (no act_saved) on the oracle's smooth batch, at the parent's geometry and weights; the gradient tensors
go, per batch size, into the file named first."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lsnf_amd                                              # noqa: E402
from lsnf_amd import flow as F                               # noqa: E402
from oracle import flow_oracle as O                          # noqa: E402


def main(out_path, nz, width, depth, batches):
    assert os.environ.get("LSNF_TN_ABL") == "7"              # (what this process is for)
    dev = torch.device("cuda", 0)
    lsnf_amd.load_library()
    p = O.init_params(nz, width, depth, seed=3)
    params = F.params_from_state_dict(p, depth, dev)
    plan = F.prepare(params, nz, width, depth, 1)
    out = {}
    for B in batches:
        z = O.smooth_batch(p, B, nz, seed=B)[0].to(dev)
        z1, _, _, saved = F.forward(plan, z, want_ll=False, save_for_backward=True)
        grads = F.backward_params(plan, params, z, z1, saved, ll_scale=-1.0 / B)
        torch.cuda.synchronize()
        out[B] = [g.detach().cpu().clone() for g in grads]
    torch.save(out, out_path)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), [int(b) for b in sys.argv[5:]])

"""fp64 restatement of the data-dependent actnorm init (reference model.py:238-241, 253-262 with init=True, threaded through
revnet2d_step.forward :389-422 and fc.forward :324-331), built from oracle.flow_oracle's pieces.  Shared by
tests/test_actnorm_init_cpu.py (which pins it to the reference's fixtures under tests/golden/init/) and
tests/test_gpu_actnorm_init.py (which uses it at batch sizes the fixtures do not cover)."""
import os

import numpy as np
import torch

from oracle import flow_oracle as O

INIT_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init")
# tensors of one block the init writes, and their ABI slots (include/lsnf_flow.h)
WRITTEN = ("actnorm.b", "actnorm.logs", "f.fc_1.actnorm.b", "f.fc_1.actnorm.logs", "f.fc_2.actnorm.b", "f.fc_2.actnorm.logs")
WRITTEN_SLOTS = (0, 1, 4, 5, 7, 8)
LOGS_ABS = 2e-6       # |logs - ref|
B_REL_RMS = 2e-6      # |b - ref| / RMS of the column the statistic is taken over


def init_names():
    return sorted(f[:-4] for f in os.listdir(INIT_DIR) if f.endswith(".npz"))


def load_init(name):
    """(starting params keyed like the reference state_dict incl. the '.bias' aliases, post-init written tensors of the
    fp32 reference, the same of the fp64 reference, remaining arrays)."""
    raw = np.load(os.path.join(INIT_DIR, name + ".npz"), allow_pickle=False)
    p, ref32, ref64, rest = {}, {}, {}, {}
    for k in raw.files:
        if k.startswith("sd/"):             # stored as float16 (exact: make_golden_init.py draws fp16-representable values)
            p[k[3:]] = torch.from_numpy(raw[k].astype(np.float32))
        elif k.startswith("sd_init/"):
            ref32[k[8:]] = raw[k]
        elif k.startswith("sd_init_f64/"):
            ref64[k[12:]] = raw[k]
        else:
            rest[k] = raw[k]
    for k in list(p):
        if k.endswith("actnorm.b"):
            p[k + "ias"] = p[k]
    return p, ref32, ref64, rest


def _fit(x):
    """b := -mean x; logs := log(1 / (sqrt(mean (x+b)^2) + 1e-6)) / 3 (model.py:238-241, 253-262).  Also the column RMS."""
    b = -x.mean(0, keepdim=True)
    v = ((x + b) ** 2).mean(0, keepdim=True)
    logs = torch.log(1.0 / (torch.sqrt(v) + 1e-6)) / 3.0
    return b, logs, torch.sqrt((x ** 2).mean(0, keepdim=True))


def restated_init(p, z, coupling=None):
    """Returns (params after the init, float64, every key; {written key: column RMS of its statistic's input})."""
    q = {k: v.double() for k, v in p.items()}
    coupling = O.coupling_of(q) if coupling is None else coupling
    x = z.double()
    rms = {}
    for i in range(O.depth_of(q)):
        pre = O.block_prefix(i)
        q[pre + "actnorm.b"], q[pre + "actnorm.logs"], r = _fit(x)
        rms[pre + "actnorm.b"] = r
        a = O.actnorm_fwd(x, q[pre + "actnorm.b"], q[pre + "actnorm.logs"])
        z1 = torch.matmul(a, q[pre + "invertible_1x1_conv.w"])[:, : x.shape[1] // 2]
        u1 = torch.matmul(z1, q[pre + "f.fc_1.w"])
        q[pre + "f.fc_1.actnorm.b"], q[pre + "f.fc_1.actnorm.logs"], r = _fit(u1)
        rms[pre + "f.fc_1.actnorm.b"] = r
        h1 = torch.relu(O.actnorm_fwd(u1, q[pre + "f.fc_1.actnorm.b"], q[pre + "f.fc_1.actnorm.logs"]))
        u2 = torch.matmul(h1, q[pre + "f.fc_2.w"])
        q[pre + "f.fc_2.actnorm.b"], q[pre + "f.fc_2.actnorm.logs"], r = _fit(u2)
        rms[pre + "f.fc_2.actnorm.b"] = r
        for k in ("actnorm", "f.fc_1.actnorm", "f.fc_2.actnorm"):
            q[pre + k + ".bias"] = q[pre + k + ".b"]
        x, _ = O.block_fwd(q, i, x, torch.zeros(x.shape[0], dtype=torch.float64), coupling)
    return q, rms


def written_keys(depth):
    return [O.block_prefix(i) + k for i in range(depth) for k in WRITTEN]


def init_error(got, ref, rms, depth):
    """(max |logs - ref|, max |b - ref| / column RMS) over the written tensors."""
    e_logs = e_b = 0.0
    for k in written_keys(depth):
        d = np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(ref[k], dtype=np.float64))
        if k.endswith("logs"):
            e_logs = max(e_logs, float(d.max()))
        else:
            e_b = max(e_b, float((d / np.maximum(np.asarray(rms[k], dtype=np.float64), 1e-30)).max()))
    return e_logs, e_b


def bounds(ref32, ref64, rms, depth):
    """The tolerances: LOGS_ABS / B_REL_RMS, or at most twice the reference's own fp32-vs-fp64 error on the fixture."""
    e_logs, e_b = init_error(ref32, ref64, rms, depth)
    return max(LOGS_ABS, 2.0 * e_logs), max(B_REL_RMS, 2.0 * e_b)

#!/usr/bin/env python3
"""Generate tests/golden/init/*.npz: the reference's data-dependent actnorm init, `_netF.forward(z, objective, init=True)`
(model.py:238-241, 253-262, threaded through :389-422 and :324-331), run on the REFERENCE's own ``model.py`` (imported
read-only from /root/reference, CPU, fp32, plus the same call in fp64 as a tie-breaker).

Runs only where the reference is checked out; the .npz files it writes are committed.  They live in the ``init/``
subdirectory so that the parametrised tests over ``tests/golden/*.npz`` do not pick them up.

    python tests/golden/make_golden_init.py

Each file holds
    sd/*            the starting state_dict (non-zero actnorm values, perturbed fc_zeros: overwriting is visible and the
                    coupling is not the identity), drawn as the reference does and then rounded to fp16-representable
                    values, so that they are stored as float16 (exactly) -- half the bytes; every file stays below 1 MB
    z               per-column means in [-3, 3], scales in [0.1, 5]
    sd_init/*       the six written tensors of every block after the call (actnorm.b / .logs of the block, fc_1, fc_2)
    sd_init_f64/*   the same call on the same module in float64
    z1, logdet      what the init call returned;  grad_z = d(-sum ll)/dz through the init call (train.py:317-323)
"""
import os
import sys
import types

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import model as ref  # noqa: E402  (the reference's model.py)

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "init")
torch.set_num_threads(4)
WRITTEN = ("actnorm.b", "actnorm.logs", "f.fc_1.actnorm.b", "f.fc_1.actnorm.logs", "f.fc_2.actnorm.b", "f.fc_2.actnorm.logs")


def build_netF(nz, width, depth, coupling, seed, fcz_std):
    torch.manual_seed(seed)
    np.random.seed(seed)
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=depth, f_flow_permutation=2, f_width=width, f_flow_coupling=coupling)
    net = ref._netF(hps, nz=nz)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for name, prm in net.named_parameters():
            if ".fc_zeros." in name:
                prm.add_(torch.randn(prm.shape, generator=g) * fcz_std)
        for prm in net.parameters():        # fp16-representable starting values: the files store them as float16
            prm.copy_(prm.half().float())
    return net


def ll_of(z1, logdet):
    prior_ll = -0.5 * (z1 ** 2)                                     # train.py:317
    prior_ll = prior_ll.flatten(1).sum(-1) + np.log(2 * np.pi)      # train.py:318
    return prior_ll + logdet                                        # train.py:319


def written_keys(depth):
    return [f"revnet2d_s.0.revnet2d_step_s.{i}.{k}" for i in range(depth) for k in WRITTEN]


def run_case(name, nz, width, B, seed, depth=5, coupling=1, fcz_std=0.1):
    net = build_netF(nz, width, depth, coupling, seed, fcz_std)
    g = torch.Generator().manual_seed(seed + 77)
    mu = (torch.rand(nz, generator=g) * 6.0 - 3.0)
    sc = torch.exp(torch.rand(nz, generator=g) * (np.log(5.0) - np.log(0.1)) + np.log(0.1))
    z = (mu + sc * torch.randn(B, nz, generator=g)).float()

    out = {"meta_nz": np.int64(nz), "meta_width": np.int64(width), "meta_depth": np.int64(depth),
           "meta_B": np.int64(B), "meta_coupling": np.int64(coupling), "z": z.numpy().copy()}
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items() if not k.endswith(".bias")}
    for k, v in sd0.items():
        out["sd/" + k] = v.numpy().astype(np.float16)      # exact: build_netF rounded them
        assert np.array_equal(out["sd/" + k].astype(np.float32), v.numpy())

    zz = z.clone().requires_grad_(True)
    z1, logdet, eps = net(zz, objective=torch.zeros(B), init=True)
    assert eps == []
    ll = ll_of(z1, logdet)
    (gz,) = torch.autograd.grad(-ll.sum(), zz)
    out["z1"] = z1.detach().numpy().copy()
    out["logdet"] = logdet.detach().numpy().copy()
    out["grad_z"] = gz.numpy().copy()
    sd1 = net.state_dict()
    for k in written_keys(depth):
        out["sd_init/" + k] = sd1[k].detach().numpy().copy()

    # fp64 tie-breaker: the same starting module and z in double
    net64 = build_netF(nz, width, depth, coupling, seed, fcz_std).double()
    with torch.no_grad():
        net64(z.double(), objective=torch.zeros(B, dtype=torch.float64), init=True)
    sd64 = net64.state_dict()
    for k in written_keys(depth):
        out["sd_init_f64/" + k] = sd64[k].numpy().copy()

    os.makedirs(HERE, exist_ok=True)
    path = os.path.join(HERE, name + ".npz")
    np.savez(path, **out)
    e_logs = max(np.abs(out["sd_init/" + k] - out["sd_init_f64/" + k]).max() for k in written_keys(depth) if k.endswith("logs"))
    e_b = max(np.abs(out["sd_init/" + k] - out["sd_init_f64/" + k]).max() for k in written_keys(depth) if k.endswith(".b"))
    print(f"{name}: nz={nz} w={width} d={depth} c={coupling} B={B} ll[mean]={ll.mean().item():.3f} "
          f"fp32-vs-fp64 |d logs|={e_logs:.2e} |d b|={e_b:.2e} -> {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    run_case("affine_nz100_w64_B100", 100, 64, 100, seed=101)
    run_case("affine_nz128_w64_B200", 128, 64, 200, seed=102)
    run_case("affine_nz100_w128_B100", 100, 128, 100, seed=103)
    run_case("tiny_nz8_w4_B37", 8, 4, 37, seed=104)
    run_case("ragged_nz126_w127_B77", 126, 127, 77, seed=105)
    run_case("ragged_nz2_w1_B9", 2, 1, 9, seed=106)
    run_case("additive_nz20_w12_B33", 20, 12, 33, seed=107, coupling=0)
    run_case("deep_nz64_w32_B64_d10", 64, 32, 64, seed=108, depth=10)
    run_case("single_nz8_w4_B1", 8, 4, 1, seed=109)

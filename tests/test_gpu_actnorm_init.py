"""GPU: data-dependent actnorm init, `_netF.forward(z, objective, init=True)` (reference model.py:238-241, 253-262) and
`flow.actnorm_init`, against the reference's fixtures (tests/golden/init/) and, at large batch sizes, against the fp64
restatement that tests/test_actnorm_init_cpu.py pins to those fixtures."""
import types

import numpy as np
import pytest
import torch

from init_restated import (B_REL_RMS, LOGS_ABS, WRITTEN_SLOTS, bounds, init_error, init_names, load_init, restated_init,
                           written_keys)
from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu
LL_REL = 1e-5     # tests/test_gpu_forward.py
Z_ABS = 1e-4
G_REL = 1e-5      # tests/test_gpu_reverse_backward.py / test_gpu_module.py (rows off the ReLU kinks)
KINK = 2e-6


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


def make_net(lsnf, p, g, dev):
    nz, w, d = int(g["meta_nz"]), int(g["meta_width"]), int(g["meta_depth"])
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=d, f_flow_permutation=2, f_width=w,
                                f_flow_coupling=int(g.get("meta_coupling", 1)))
    net = lsnf._netF(hps, nz=nz)
    net.load_state_dict(p, strict=True)
    return net.to(dev)


def ll_of(z1, logdet):
    return (-0.5 * (z1 ** 2)).flatten(1).sum(-1) + np.log(2 * np.pi) + logdet     # train.py:317-319


def state(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def synthetic(nz, width, B, seed, depth=5):
    """Affine-coupling weights with the reference's initial distributions (fc_zeros perturbed) and z with per-column means
    in [-3, 3] and scales in [0.1, 5], as in the fixtures."""
    p = O.init_params(nz, width, depth, seed=seed, fcz_std=0.1)
    g = torch.Generator().manual_seed(seed + 7)
    mu = torch.rand(nz, generator=g) * 6.0 - 3.0
    sc = torch.exp(torch.rand(nz, generator=g) * (np.log(5.0) - np.log(0.1)) + np.log(0.1))
    z = (mu + sc * torch.randn(B, nz, generator=g)).float()
    return p, z


def params_of(lsnf, p, depth, dev):
    """The depth*12 live tensors, shaped as the reference registers them."""
    return [t.clone() for t in lsnf.params_from_state_dict(p, depth, dev)]


# ---- 1. the reference's fixtures, every kernel family / math mode ------------------------------------------------------
@pytest.mark.parametrize("name", init_names())
def test_init_call_matches_reference_fixture(lsnf, kernels, gpu_device, name):
    p, ref32, ref64, g = load_init(name)
    depth, nz = int(g["meta_depth"]), int(g["meta_nz"])
    net = make_net(lsnf, p, g, gpu_device)
    z = torch.from_numpy(g["z"]).to(gpu_device).requires_grad_(True)
    z1, logdet, eps = net(z, torch.zeros(z.shape[0], device=gpu_device), init=True)
    assert eps == []
    (gz,) = torch.autograd.grad(-ll_of(z1, logdet).sum(), z)
    sd = state(net)

    # the written tensors against the reference's
    _, rms = restated_init(p, torch.from_numpy(g["z"]), int(g["meta_coupling"]))
    tol_logs, tol_b = bounds(ref32, ref64, rms, depth)
    e_logs, e_b = init_error({k: sd[k].numpy() for k in written_keys(depth)}, ref32, rms, depth)
    assert e_logs <= tol_logs and e_b <= tol_b, (e_logs, e_b, tol_logs, tol_b)
    # the read-only ones bit for bit
    written = set(written_keys(depth))
    for k, v in p.items():
        if k.endswith(".bias"):
            continue
        if k not in written:
            assert torch.equal(sd[k], v), k

    if int(g["meta_B"]) == 1:
        # var = 0: every actnorm scale is exp(3 logs) = 1e6 and every centred input exactly 0.  The reference subtracts
        # before it scales and returns exact zeros; the forward kernels fold the scale into the weights (x*s + b*s), which
        # leaves 1e6 * ulp(x) per block -- the function itself is that ill-conditioned there.  Only the writes are compared.
        return
    # what the call returned: the plain forward under the new parameters
    z1r, ldr = g["z1"], g["logdet"]
    assert np.max(np.abs(z1.detach().cpu().numpy() - z1r)) <= Z_ABS * max(1.0, np.abs(z1r).max())
    assert np.max(np.abs(logdet.detach().cpu().numpy() - ldr) / np.maximum(np.abs(ldr), 1.0)) <= LL_REL
    p_init = dict(p)
    p_init.update({k: torch.from_numpy(ref32[k]) for k in written_keys(depth)})
    ok = (O.relu_margin(p_init, torch.from_numpy(g["z"])) > KINK).numpy()
    got, ref = gz.cpu().numpy(), g["grad_z"]
    if ok.any():
        assert np.linalg.norm(got[ok] - ref[ok]) / np.linalg.norm(ref[ok]) <= G_REL
        assert np.max(np.abs(got[ok] - ref[ok])) <= 1e-4 * max(1.0, np.abs(ref).max())


# ---- 2. large batches against the fp64 restatement -----------------------------------------------------------------------
@pytest.mark.parametrize("nz,width,B", [(128, 64, 20000), (128, 64, 65536), (128, 128, 20000)])
def test_init_large_batch_matches_fp64_restatement(lsnf, gpu_device, nz, width, B):
    depth = 5
    p, z = synthetic(nz, width, B, seed=B + width)
    params = params_of(lsnf, p, depth, gpu_device)
    lsnf.flow.actnorm_init(params, z.to(gpu_device), nz, width, depth, 1)
    torch.cuda.synchronize()
    q, rms = restated_init(p, z, 1)
    got = {}
    for i in range(depth):
        for s, k in zip(WRITTEN_SLOTS, ("actnorm.b", "actnorm.logs", "f.fc_1.actnorm.b", "f.fc_1.actnorm.logs",
                                        "f.fc_2.actnorm.b", "f.fc_2.actnorm.logs")):
            got[O.block_prefix(i) + k] = params[i * 12 + s].cpu().numpy()
    e_logs, e_b = init_error(got, {k: q[k].numpy() for k in written_keys(depth)}, rms, depth)
    assert e_logs <= LOGS_ABS and e_b <= B_REL_RMS, (e_logs, e_b)


# ---- 3. reproducibility ------------------------------------------------------------------------------------------------
def test_init_is_bitwise_reproducible(lsnf, gpu_device):
    nz, width, depth, B = 128, 64, 5, 20000
    p, z = synthetic(nz, width, B, seed=5)
    zd = z.to(gpu_device)
    ref = params_of(lsnf, p, depth, gpu_device)
    lsnf.flow.actnorm_init(ref, zd, nz, width, depth, 1)
    again = params_of(lsnf, p, depth, gpu_device)
    lsnf.flow.actnorm_init(again, zd, nz, width, depth, 1)
    assert all(torch.equal(a, b) for a, b in zip(ref, again))
    # the tuning knobs do not reach the init
    prev_small, prev_math = lsnf.flow.set_small_batch_max(lsnf.flow.SMALL_BATCH_AUTO), lsnf.flow.set_math_mode(-1)
    try:
        for small in (0, 1 << 30):
            for math in (lsnf.flow.MATH_FP32, lsnf.flow.MATH_BF16X3, lsnf.flow.MATH_BF16X3_PHASED, lsnf.flow.MATH_FP16X2):
                lsnf.flow.set_small_batch_max(small)
                lsnf.flow.set_math_mode(math)
                other = params_of(lsnf, p, depth, gpu_device)
                lsnf.flow.actnorm_init(other, zd, nz, width, depth, 1)
                assert all(torch.equal(a, b) for a, b in zip(ref, other)), (small, math)
    finally:
        lsnf.flow.set_small_batch_max(prev_small)
        lsnf.flow.set_math_mode(prev_math)
    # nor do the actnorm values it starts from
    moved = params_of(lsnf, p, depth, gpu_device)
    for i, t in enumerate(moved):
        if i % 12 in WRITTEN_SLOTS:
            t.copy_(torch.randn(t.shape, generator=torch.Generator().manual_seed(i)).to(gpu_device))
    lsnf.flow.actnorm_init(moved, zd, nz, width, depth, 1)
    assert all(torch.equal(a, b) for a, b in zip(ref, moved))


# ---- 4. everything after the init sees the new weights ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["affine_nz128_w64_B200", "additive_nz20_w12_B33"])
def test_calls_after_init_use_the_new_weights(lsnf, gpu_device, name):
    p, _, _, g = load_init(name)
    net = make_net(lsnf, p, g, gpu_device)
    z = torch.from_numpy(g["z"]).to(gpu_device)
    obj = torch.zeros(z.shape[0], device=gpu_device)
    with torch.no_grad():
        z1_before, _, _ = net(z, obj)
        z1_init, ld_init, _ = net(z, obj, init=True)
        z1, ld, _ = net(z, obj)
    assert not torch.equal(z1_before, z1_init)
    assert torch.equal(z1, z1_init) and torch.equal(ld, ld_init)
    ll = ll_of(z1, ld)
    _, _, ll_lp = net.log_prob(z)
    assert ((ll_lp - ll).abs() / ll.abs().clamp_min(1.0)).max().item() <= LL_REL
    _, ll_lv, _, _ = net.langevin_step(z, step_size=0.1)
    assert ((ll_lv - ll).abs() / ll.abs().clamp_min(1.0)).max().item() <= LL_REL
    loss = net.mle_grads(z)
    assert abs(loss.item() + ll.mean().item()) <= LL_REL * max(1.0, abs(ll.mean().item()))
    with torch.no_grad():
        zr = net(z1, obj, reverse=True)
    assert (zr - z).abs().max().item() <= 1e-3 * max(1.0, z.abs().max().item())


# ---- 5. a graph recorded before the init is refused after it ------------------------------------------------------------
def test_backward_across_init_raises(lsnf, gpu_device):
    p, _, _, g = load_init("affine_nz100_w64_B100")
    net = make_net(lsnf, p, g, gpu_device)
    z = torch.from_numpy(g["z"]).to(gpu_device)
    obj = torch.zeros(z.shape[0], device=gpu_device)
    z1, ld, _ = net(z, obj)                               # parameters require grad: a graph is recorded
    with torch.no_grad():
        net(z, obj, init=True)
    with pytest.raises(lsnf.LsnfError, match="modified between forward and backward"):
        (-ll_of(z1, ld).mean()).backward()


# ---- 6. the other cases and argument checks -----------------------------------------------------------------------------
def test_init_edge_cases(lsnf, gpu_device):
    p, _, _, g = load_init("tiny_nz8_w4_B37")
    net = make_net(lsnf, p, g, gpu_device)
    z = torch.from_numpy(g["z"]).to(gpu_device)
    obj = torch.zeros(z.shape[0], device=gpu_device)
    before = state(net)
    with torch.no_grad():
        x_plain = net(z, obj, reverse=True)
        x_init = net(z, obj, init=True, reverse=True)    # init is ignored on the reverse branch (model.py:484-498)
    assert torch.equal(x_plain, x_init)
    assert all(torch.equal(v, before[k]) for k, v in state(net).items())
    with pytest.raises(lsnf.LsnfError):
        net(z[:0], obj[:0], init=True)
    assert all(torch.equal(v, before[k]) for k, v in state(net).items())
    with torch.no_grad():                                # no graph, same parameters as with one
        net(z, obj, init=True)
    after_no_grad = state(net)
    net2 = make_net(lsnf, p, g, gpu_device)
    net2(z.clone().requires_grad_(True), obj, init=True)
    assert all(torch.equal(v, after_no_grad[k]) for k, v in state(net2).items())


def test_actnorm_init_rejects_bad_arguments_without_launching(lsnf, gpu_device):
    nz, width, depth, B = 8, 4, 2, 37
    p, z = synthetic(nz, width, B, seed=3, depth=depth)
    params = params_of(lsnf, p, depth, gpu_device)
    snapshot = [t.clone() for t in params]
    zd = z.to(gpu_device)
    init = lsnf.flow.actnorm_init
    need = lsnf.flow.actnorm_init_workspace_bytes(nz, width, depth, 1, B)
    bad_calls = [
        lambda: init(params, zd[:, :6].contiguous(), nz, width, depth, 1),                     # z shape
        lambda: init(params, zd.double(), nz, width, depth, 1),                                # z dtype
        lambda: init(params, zd.t().contiguous().t(), nz, width, depth, 1),                    # z not contiguous
        lambda: init(params, zd.cpu(), nz, width, depth, 1),                                   # z on the CPU
        lambda: init(params[:-1], zd, nz, width, depth, 1),                                    # tensor count
        lambda: init(params[:1] + [params[1].view(-1)] + params[2:], zd, nz, width, depth, 1),  # vector shape
        lambda: init(params[:2] + [params[2].t()] + params[3:], zd, nz, width, depth, 1),      # not contiguous
        lambda: init(params[:3] + [params[3].double()] + params[4:], zd, nz, width, depth, 1),  # dtype
        lambda: init(params[:4] + [params[4].cpu()] + params[5:], zd, nz, width, depth, 1),    # device
        lambda: init(params, zd, nz, width, depth, 1,
                     workspace=torch.empty(need // 4 - 1, dtype=torch.float32, device=gpu_device)),   # workspace too small
        lambda: init(params, zd, nz + 1, width, depth, 1),                                     # geometry
    ]
    for call in bad_calls:
        with pytest.raises(lsnf.LsnfError):
            call()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(params, snapshot))
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=gpu_device)     # exactly enough
    init(params, zd, nz, width, depth, 1, workspace=ws)
    torch.cuda.synchronize()
    assert not torch.equal(params[0], snapshot[0])

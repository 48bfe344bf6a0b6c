"""CPU: the fused optimizer step without a GPU -- `lsnf_adam_state_bytes` / `lsnf_adam_step` are declared, exported and bound,
the state size follows the geometry, the entry point validates before any HIP call, the float64 restatement the GPU tests use
(tests/adam_restated.py) IS torch.optim.Adam + clip_grad_norm_, and `FlowAdam` has no CPU path.  None of this holds without the
feature."""
import ctypes
import os
import re
import types

import pytest
import torch

from conftest import ROOT

import lsnf_amd
from adam_restated import clip_adam

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2
HEADER = 4160


def numel_sum(nz, w, depth, coupling=1):
    half, n_out = nz // 2, (nz if coupling == 1 else nz // 2)
    return depth * (2 * nz + nz * nz + half * w + 4 * w + w * w + w * n_out + 2 * n_out)


def test_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    assert re.search(r"\bsize_t\s+lsnf_adam_state_bytes\s*\(", hdr) and re.search(r"\bint\s+lsnf_adam_step\s*\(", hdr)
    for name in ("lsnf_adam_state_bytes", "lsnf_adam_step"):
        assert hasattr(lib, name)
        assert name in lsnf_amd._lib._SIGNATURES and name in lsnf_amd.exported_symbols()
    assert len(lsnf_amd._lib._SIGNATURES["lsnf_adam_step"][1]) == 16
    assert lib.lsnf_abi_version() == 5                          # symbols were added, nothing else changed
    assert int(re.search(r"#define\s+LSNF_ADAM_HEADER_BYTES\s+(\d+)", hdr).group(1)) == HEADER == lsnf_amd.flow.ADAM_HEADER_BYTES


def test_state_bytes_follow_the_geometry():
    lib = lsnf_amd.load_library()
    sb = lib.lsnf_adam_state_bytes
    for bad in ((130, 64, 5, 1), (7, 4, 5, 1), (128, 64, 17, 1), (128, 64, 5, 2), (128, 200, 5, 1), (128, 64, 0, 1)):
        assert lib.lsnf_plan_floats(*bad) == 0 and sb(*bad) == 0
    for geo in ((128, 64, 5, 1), (128, 64, 5, 0), (2, 1, 1, 1), (126, 127, 2, 1)):
        assert sb(*geo) >= HEADER + 2 * 4 * numel_sum(*geo)
        assert sb(*geo) % 16 == 0
        assert lsnf_amd.flow.adam_state_bytes(*geo) == sb(*geo)
    assert sb(128, 64, 5, 0) < sb(128, 64, 5, 1)
    sizes = [sb(128, 64, d, 1) for d in range(1, 17)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))


def test_validates_before_any_hip_call():
    lib = lsnf_amd.load_library()
    n = 5 * 12
    tab = (ctypes.c_void_p * n)(*[0x10000 * (i + 1) for i in range(n)])      # addresses that are never dereferenced on the host
    gtab = (ctypes.c_void_p * n)(*[0x2000000 + 0x10000 * i for i in range(n)])
    state = ctypes.c_void_p(0x40000000)
    base = dict(p=tab, g=gtab, nz=128, w=64, d=5, c=1, state=state, lr=1e-3, lr_dev=None, b1=0.5, b2=0.999, eps=1e-8, wd=0.0,
                mn=0.0, out=None)

    def call(**kw):
        a = dict(base, **kw)
        return lib.lsnf_adam_step(a["p"], a["g"], a["nz"], a["w"], a["d"], a["c"], a["state"], a["lr"], a["lr_dev"], a["b1"],
                                  a["b2"], a["eps"], a["wd"], a["mn"], a["out"], None)

    def refused(**kw):
        return call(**kw) == LSNF_E_ARG and b"lsnf_adam_step" in lib.lsnf_last_error()

    for geo in (dict(nz=130), dict(d=17), dict(nz=7, w=4), dict(c=2), dict(w=200)):
        assert call(**geo) == LSNF_E_GEOMETRY
    for name in ("p", "g", "state"):
        assert refused(**{name: None}) and b"NULL" in lib.lsnf_last_error()
    assert refused(state=ctypes.c_void_p(0x40000004)) and b"16-byte" in lib.lsnf_last_error()
    for bad in (-1e-3, float("nan"), float("inf")):
        assert refused(lr=bad) and b"lr" in lib.lsnf_last_error()
        assert refused(eps=bad) and b"eps" in lib.lsnf_last_error()
        assert refused(wd=bad) and b"weight_decay" in lib.lsnf_last_error()
    for bad in (1.0, -0.1, 1.5, float("nan")):
        assert refused(b1=bad) and refused(b2=bad) and b"betas" in lib.lsnf_last_error()
    assert refused(mn=float("nan"))
    hole = (ctypes.c_void_p * n)(*[0 if i == 17 else 0x10000 * (i + 1) for i in range(n)])
    assert refused(p=hole) and b"parameter pointer 17" in lib.lsnf_last_error()
    odd = (ctypes.c_void_p * n)(*[0x2000002 if i == 3 else 0 for i in range(n)])
    assert refused(g=odd) and b"gradient pointer 3" in lib.lsnf_last_error()
    assert refused(out=ctypes.c_void_p(0x50000002)) and refused(lr_dev=ctypes.c_void_p(0x50000001))


CONFIGS = [(0.0, None), (1e-2, None), (0.0, "below"), (1e-2, "above"), (0.0, "above"), (1e-2, "below")]


@pytest.mark.parametrize("weight_decay,clip", CONFIGS)
def test_float64_restatement_is_torch_adam_with_clip(weight_decay, clip):
    """20 steps, float64 on both sides: only the order of a handful of operations differs."""
    gen = torch.Generator().manual_seed(11)
    shapes = [(1, 6), (6, 6), (3, 5), (1, 5), (5, 5), (5, 6), (1, 1)]
    params = [torch.randn(*s, generator=gen, dtype=torch.float64) * 0.3 for s in shapes]
    steps = [[torch.randn(*s, generator=gen, dtype=torch.float64) * (0.1 + 0.05 * k) for s in shapes] for k in range(20)]
    for k in range(20):
        steps[k][2] = None if k % 3 == 0 else steps[k][2]          # a tensor without a gradient in some steps only
        steps[k][6] = None                                          # ... and one that never has one
    norms = [float(torch.sqrt(sum((g ** 2).sum() for g in gs if g is not None))) for gs in steps]
    max_norm = None if clip is None else (0.5 * min(norms) if clip == "below" else 2.0 * max(norms))
    hyper = dict(lr=3e-3, betas=(0.5, 0.999), eps=1e-8, weight_decay=weight_decay)
    live = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.Adam(live, foreach=False, **hyper)
    for gs in steps:
        for p, g in zip(live, gs):
            p.grad = None if g is None else g.clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(live, max_norm)
        opt.step()
    # torch starts a tensor's step count at its first gradient; tensor 2 misses step 1, so restate it on its own count
    p, m, v, got_norms = clip_adam(params, steps, max_norm=max_norm, **hyper)
    assert max(abs(a - b) for a, b in zip(got_norms, norms)) <= 1e-12
    for i, q in enumerate(live):
        if i == 2:
            continue
        assert (p[i] - q.detach()).abs().max().item() <= 1e-12
        if q in opt.state:
            assert (m[i] - opt.state[q]["exp_avg"]).abs().max().item() <= 1e-12
            assert (v[i] - opt.state[q]["exp_avg_sq"]).abs().max().item() <= 1e-12
    assert live[6] not in opt.state and torch.equal(p[6], params[6]) and not m[6].any() and not v[6].any()


def test_float32_leg_of_the_restatement_tracks_float64():
    gen = torch.Generator().manual_seed(5)
    params = [torch.randn(40, 7, generator=gen) * 0.2, torch.randn(1, 9, generator=gen)]
    steps = [[torch.randn_like(t) * 0.1 for t in params] for _ in range(5)]
    hyper = dict(lr=1e-3, betas=(0.5, 0.999), weight_decay=1e-2, max_norm=0.5)
    p64, m64, v64, _ = clip_adam(params, steps, **hyper)
    p32, m32, v32, _ = clip_adam(params, steps, dtype=torch.float32, **hyper)
    for a, b in zip(p64 + m64 + v64, p32 + m32 + v32):
        assert b.dtype == torch.float32 and (a - b.double()).abs().max().item() <= 2e-6 * a.abs().max().item()


def test_flow_adam_has_no_cpu_path():
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    with pytest.raises(lsnf_amd.LsnfError):
        lsnf_amd.FlowAdam(net)
    with pytest.raises(lsnf_amd.LsnfError):
        lsnf_amd.FlowAdam(list(net.parameters()))
    with pytest.raises(lsnf_amd.LsnfError, match="flow_mle_step"):
        net.mle_step(torch.zeros(3, 8), torch.optim.Adam(net.parameters()))
    params = [torch.zeros(s) for s in lsnf_amd.flow._param_shapes(8, 4, 1) * 2]
    with pytest.raises(lsnf_amd.LsnfError):
        lsnf_amd.flow.adam_step(params, [None] * 24, torch.zeros(4096), 8, 4, 2, 1)

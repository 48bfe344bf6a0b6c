"""CPU: the variants of the fused optimizer step without a GPU -- `lsnf_adam_state_bytes_ex` / `lsnf_adam_step_ex` and their
flags are declared, exported and bound, the state grows by one array per sizing flag, the entry point validates before any HIP
call, the float64 restatement the GPU tests use (tests/adam_variants_restated.py) IS torch.optim.Adam / AdamW + clip_grad_norm_
for all eight combinations of amsgrad x decoupled x maximize, and `FlowAdam` speaks torch's state format for every variant (its
state lives in views of one flat buffer, so the format and the round trips can be exercised on CPU tensors; only `step()` needs
the device).  None of this holds without the feature."""
import ctypes
import itertools
import os
import re
import types

import pytest
import torch

from conftest import ROOT

import lsnf_amd
from adam_variants_restated import clip_adam_variants, ema_of
from counting_lib import QUERIES, install

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2
HEADER = 4160
FLAGS = dict(LSNF_ADAM_AMSGRAD=1, LSNF_ADAM_DECOUPLED=2, LSNF_ADAM_MAXIMIZE=4, LSNF_ADAM_EMA=8, LSNF_ADAM_SKIP_NONFINITE=16)
F = lsnf_amd.flow
Options = lsnf_amd._lib.LsnfAdamOptions


def numel_sum(nz, w, depth, coupling=1):
    half, n_out = nz // 2, (nz if coupling == 1 else nz // 2)
    return depth * (2 * nz + nz * nz + half * w + 4 * w + w * w + w * n_out + 2 * n_out)


def test_symbols_and_flags_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "lsnf_flow.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = lsnf_amd.load_library()
    assert re.search(r"\bsize_t\s+lsnf_adam_state_bytes_ex\s*\(", hdr) and re.search(r"\bint\s+lsnf_adam_step_ex\s*\(", hdr)
    for name in ("lsnf_adam_state_bytes_ex", "lsnf_adam_step_ex"):
        assert hasattr(lib, name)
        assert name in lsnf_amd._lib._SIGNATURES and name in lsnf_amd.exported_symbols()
    assert lib.lsnf_abi_version() == 5                          # symbols were added, nothing else changed
    for name, value in FLAGS.items():
        assert int(re.search(rf"#define\s+{name}\s+(\d+)u?\b", hdr).group(1)) == value == getattr(F, name[5:])
    skipped = int(re.search(r"#define\s+LSNF_ADAM_SKIPPED_OFFSET\s+(\d+)", hdr).group(1))
    norm = int(re.search(r"#define\s+LSNF_ADAM_NORM_OFFSET\s+(\d+)", hdr).group(1))
    assert skipped == F.ADAM_SKIPPED_OFFSET and skipped % 8 == 0 and norm + 4 <= skipped and skipped + 8 <= HEADER
    # the struct of the header, field by field, is the ctypes one
    body = re.search(r"typedef\s+struct\s+LsnfAdamOptions\s*\{(.*?)\}\s*LsnfAdamOptions\s*;", hdr, flags=re.S).group(1)
    declared = [n.strip(" *") for decl in body.split(";") if decl.strip()
                for n in re.sub(r"^\s*(const\s+)?(unsigned|double|float)\s*\*?", "", decl.strip()).split(",")]
    assert declared == [n for n, _ in Options._fields_]
    assert ctypes.sizeof(Options) == 80 and Options.lr.offset == 8 and Options.grad_norm_out.offset == 72
    for word in ("vmax", "ema_decay", "SKIP_NONFINITE", "step == 1"):          # the formulas are documented
        assert word in text


def test_state_bytes_ex_adds_one_array_per_sizing_flag():
    lib = lsnf_amd.load_library()
    sb, sbx = lib.lsnf_adam_state_bytes, lib.lsnf_adam_state_bytes_ex
    A, D, M, E, S = FLAGS.values()
    for bad in ((130, 64, 5, 1), (128, 64, 17, 1), (128, 64, 5, 2)):
        assert sbx(*bad, A | E) == 0
    for geo in ((128, 64, 5, 1), (128, 64, 5, 0), (2, 1, 1, 1), (126, 127, 2, 1), (8, 4, 16, 1)):
        base = sb(*geo)
        array = (base - HEADER) // 2                                # m today: N floats, N rounded up to 4
        assert array == 4 * ((numel_sum(*geo) + 3) // 4 * 4)
        assert sbx(*geo, 0) == base == sbx(*geo, D | M | S)         # flags that do not size the state
        assert sbx(*geo, A) == base + array == sbx(*geo, E) == sbx(*geo, A | D | M | S)
        assert sbx(*geo, A | E) == base + 2 * array
        assert sbx(*geo, 32) == 0 and sbx(*geo, A | 1 << 31) == 0   # an unknown bit
        assert F.adam_state_bytes(*geo) == base
        assert F.adam_state_bytes(*geo, amsgrad=True) == F.adam_state_bytes(*geo, ema=True) == base + array
        assert F.adam_state_bytes(*geo, amsgrad=True, ema=True) == base + 2 * array


def test_extra_views_sit_behind_v():
    geo = (126, 127, 2, 1)
    for amsgrad, ema in itertools.product((False, True), repeat=2):
        state = F.new_adam_state(*geo, "cpu", amsgrad=amsgrad, ema=ema)
        assert state.numel() * 4 == F.adam_state_bytes(*geo, amsgrad, ema)
        steps, norm, m, v = F.adam_state_views(state, *geo)           # the four-tuple is what it was
        vmax, avg, skipped = F.adam_state_extra_views(state, *geo, amsgrad, ema)
        assert (vmax is None) == (not amsgrad) and (avg is None) == (not ema)
        assert skipped.dtype == torch.int64 and skipped.dim() == 0
        assert skipped.data_ptr() == state.data_ptr() + F.ADAM_SKIPPED_OFFSET
        n4 = (numel_sum(*geo) + 3) // 4 * 4
        arrays = [m, v] + ([vmax] if amsgrad else []) + ([avg] if ema else [])
        for k, arr in enumerate(arrays):
            assert [tuple(t.shape) for t in arr] == [tuple(t.shape) for t in m]
            assert arr[0].data_ptr() == state.data_ptr() + HEADER + 4 * k * n4
            assert arr[-1].data_ptr() + 4 * arr[-1].numel() <= state.data_ptr() + 4 * state.numel()
    with pytest.raises(lsnf_amd.LsnfError):                           # a plain state has no room for vmax
        F.adam_state_extra_views(F.new_adam_state(*geo, "cpu"), *geo, True, False)


def test_ex_validates_before_any_hip_call():
    lib = lsnf_amd.load_library()
    n = 5 * 12
    tab = (ctypes.c_void_p * n)(*[0x10000 * (i + 1) for i in range(n)])      # addresses that are never dereferenced on the host
    gtab = (ctypes.c_void_p * n)(*[0x2000000 + 0x10000 * i for i in range(n)])
    base = dict(p=tab, g=gtab, nz=128, w=64, d=5, c=1, state=ctypes.c_void_p(0x40000000), size=ctypes.sizeof(Options), flags=0,
                lr=1e-3, lr_dev=None, b1=0.5, b2=0.999, eps=1e-8, wd=0.0, mn=0.0, ema=0.0, out=None)

    def call(**kw):
        a = dict(base, **kw)
        o = Options(a["size"], a["flags"], a["lr"], a["lr_dev"], a["b1"], a["b2"], a["eps"], a["wd"], a["mn"], a["ema"], a["out"])
        return lib.lsnf_adam_step_ex(a["p"], a["g"], a["nz"], a["w"], a["d"], a["c"], a["state"], ctypes.byref(o), None)

    def refused(**kw):
        return call(**kw) == LSNF_E_ARG and b"lsnf_adam_step_ex" in lib.lsnf_last_error()

    A, D, M, E, S = FLAGS.values()
    assert lib.lsnf_adam_step_ex(tab, gtab, 128, 64, 5, 1, base["state"], None, None) == LSNF_E_ARG and b"options" in lib.lsnf_last_error()
    for size in (0, 72, 84, 96):
        assert refused(size=size) and b"struct_bytes" in lib.lsnf_last_error()
    for flags in (32, 64, A | 128, 1 << 31):
        assert refused(flags=flags) and b"flag" in lib.lsnf_last_error()
    for bad in (1.0, -0.1, 1.5, float("nan"), float("inf")):
        assert refused(flags=E, ema=bad) and b"ema_decay" in lib.lsnf_last_error()
        assert refused(flags=A | D | M | E | S, ema=bad)
    # ... and everything lsnf_adam_step refuses, with every flag set
    for flags in (0, A | D | M | E | S):
        kw = dict(flags=flags, ema=0.99)
        for geo in (dict(nz=130), dict(d=17), dict(nz=7, w=4), dict(c=2), dict(w=200)):
            assert call(**geo, **kw) == LSNF_E_GEOMETRY
        for name in ("p", "g", "state"):
            assert refused(**{name: None}, **kw) and b"NULL" in lib.lsnf_last_error()
        assert refused(state=ctypes.c_void_p(0x40000004), **kw) and b"16-byte" in lib.lsnf_last_error()
        for bad in (-1e-3, float("nan"), float("inf")):
            assert refused(lr=bad, **kw) and b"lr" in lib.lsnf_last_error()
            assert refused(eps=bad, **kw) and b"eps" in lib.lsnf_last_error()
            assert refused(wd=bad, **kw) and b"weight_decay" in lib.lsnf_last_error()
        for bad in (1.0, -0.1, 1.5, float("nan")):
            assert refused(b1=bad, **kw) and refused(b2=bad, **kw) and b"betas" in lib.lsnf_last_error()
        assert refused(mn=float("nan"), **kw)
        hole = (ctypes.c_void_p * n)(*[0 if i == 17 else 0x10000 * (i + 1) for i in range(n)])
        assert refused(p=hole, **kw) and b"parameter pointer 17" in lib.lsnf_last_error()
        odd = (ctypes.c_void_p * n)(*[0x2000002 if i == 3 else 0 for i in range(n)])
        assert refused(g=odd, **kw) and b"gradient pointer 3" in lib.lsnf_last_error()
        assert refused(out=ctypes.c_void_p(0x50000002), **kw) and refused(lr_dev=ctypes.c_void_p(0x50000001), **kw)


@pytest.mark.parametrize("kw", [dict(amsgrad=True), dict(ema_decay=0.9), dict(maximize=True), dict(decoupled_weight_decay=True),
                                dict(skip_nonfinite=True), dict(ema_decay=1.0), dict(ema_decay=float("nan")), dict(ema_decay=-0.5)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_wrapper_refuses_cpu_tensors_and_bad_decays_before_any_launch(kw, monkeypatch):
    """The variants go through the one argument-checking path of flow.adam_step: nothing that may launch is entered."""
    stand = install(monkeypatch, lsnf_amd)
    geo = (8, 4, 2, 1)
    params = [torch.zeros(s) for s in F._param_shapes(8, 4, 1) * 2]
    state = torch.zeros(F.adam_state_bytes(*geo, amsgrad=True, ema=True) // 4)
    with pytest.raises(lsnf_amd.LsnfError):
        F.adam_step(params, [torch.zeros_like(p) for p in params], state, *geo, **kw)
    assert [n for n in stand.launching() if n not in QUERIES | {"lsnf_adam_state_bytes_ex"}] == []


COMBOS = list(itertools.product((False, True), repeat=3))


@pytest.mark.parametrize("amsgrad,decoupled,maximize", COMBOS)
def test_float64_restatement_is_torch_adam_and_adamw(amsgrad, decoupled, maximize):
    """20 steps with weight decay and an active clip, float64 on both sides: only the order of a handful of operations differs.
    Gate: 1e-12 relative to the largest entry of each tensor."""
    gen = torch.Generator().manual_seed(11)
    shapes = [(1, 6), (6, 6), (3, 5), (1, 5), (5, 5), (5, 6), (1, 1)]
    params = [torch.randn(*s, generator=gen, dtype=torch.float64) * 0.3 for s in shapes]
    # scales that fall after the third step, so that amsgrad's maximum differs from v for most of the run
    steps = [[torch.randn(*s, generator=gen, dtype=torch.float64) * (0.3 if k < 3 else 0.03) for s in shapes] for k in range(20)]
    for k in range(20):
        steps[k][6] = None                                          # a tensor that never has a gradient
    norms = [float(torch.sqrt(sum((g ** 2).sum() for g in gs if g is not None))) for gs in steps]
    max_norm = 0.5 * min(norms)                                     # the clip is active in every step
    hyper = dict(lr=3e-3, betas=(0.5, 0.9), eps=1e-8, weight_decay=1e-2)
    live = [torch.nn.Parameter(p.clone()) for p in params]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(live, foreach=False, amsgrad=amsgrad, maximize=maximize, **hyper)
    for gs in steps:
        for p, g in zip(live, gs):
            p.grad = None if g is None else g.clone()
        torch.nn.utils.clip_grad_norm_(live, max_norm)
        opt.step()
    r = clip_adam_variants(params, steps, max_norm=max_norm, amsgrad=amsgrad, decoupled=decoupled, maximize=maximize, **hyper)
    assert r["step"] == 20 and r["skipped"] == 0
    assert max(abs(a - b) for a, b in zip(r["norms"], norms)) <= 1e-12 * max(norms)

    def close(a, b):
        return (a - b).abs().max().item() <= 1e-12 * b.abs().max().item()

    for i, q in enumerate(live[:6]):
        st = opt.state[q]
        assert close(r["p"][i], q.detach()) and close(r["m"][i], st["exp_avg"]) and close(r["v"][i], st["exp_avg_sq"])
        if amsgrad:
            assert close(r["vmax"][i], st["max_exp_avg_sq"])
            assert (r["vmax"][i] > r["v"][i]).double().mean().item() >= 0.5         # the maximum was not idle
    assert live[6] not in opt.state and torch.equal(r["p"][6], params[6]) and not r["m"][6].any()
    # the three options each change the result (a restatement that ignored one would still agree with itself)
    plain = clip_adam_variants(params, steps, max_norm=max_norm, **hyper)
    if amsgrad or decoupled or maximize:
        assert not close(r["p"][1], plain["p"][1])


def test_restated_skip_and_average():
    gen = torch.Generator().manual_seed(3)
    params = [torch.randn(4, 5, generator=gen, dtype=torch.float64), torch.randn(1, 3, generator=gen, dtype=torch.float64)]
    good = [[torch.randn_like(t) * 0.1 for t in params] for _ in range(3)]
    bad = [g.clone() for g in good[1]]
    bad[0][2, 1] = float("inf")
    hyper = dict(lr=1e-2, betas=(0.5, 0.9), amsgrad=True, ema_decay=0.75)
    r3 = clip_adam_variants(params, [good[0], bad, good[2]], skip_nonfinite=True, **hyper)
    r2 = clip_adam_variants(params, [good[0], good[2]], **hyper)
    assert r3["step"] == 2 and r3["skipped"] == 1 and not torch.isfinite(torch.tensor(r3["norms"][1]))
    for key in ("p", "m", "v", "vmax", "ema"):
        assert all(torch.equal(a, b) for a, b in zip(r3[key], r2[key]))
    poisoned = clip_adam_variants(params, [good[0], bad, good[2]], **hyper)       # without the skip the inf gets through
    assert not torch.isfinite(poisoned["p"][0]).all()
    # the average is the recursion over the stored parameters, started from the parameters before the first step
    r1 = clip_adam_variants(params, good[:1], **hyper)
    snaps = [params, r1["p"], r2["p"]]
    for a, b in zip(ema_of(snaps, 0.75), r2["ema"]):
        assert (a - b).abs().max().item() <= 1e-15
    assert all(torch.equal(a, b) for a, b in zip(ema_of(snaps[:2], 0.75), r1["ema"]))
    # a tensor without gradients: its average is the tensor
    r = clip_adam_variants(params, [[g[0], None] for g in good], **hyper)
    assert torch.equal(r["ema"][1], params[1]) and torch.equal(r["p"][1], params[1])


def test_restated_decoupled_decay_with_an_average_and_without_amsgrad():
    """The combination lsnf_adam_kernel<false, true, true> serves (tests/test_gpu_flow_adam_variants.py's "decoupled-ema"): the
    restatement's p, m and v are torch.optim.AdamW's whatever the average does, no maximum is kept, the average is the recursion
    over the parameters as stored, and both options bite."""
    gen = torch.Generator().manual_seed(13)
    params = [torch.randn(4, 5, generator=gen, dtype=torch.float64), torch.randn(1, 3, generator=gen, dtype=torch.float64)]
    steps = [[torch.randn_like(t) * 0.1 for t in params] for _ in range(5)]
    hyper = dict(lr=1e-2, betas=(0.5, 0.9), eps=1e-8, weight_decay=1e-2)
    r = clip_adam_variants(params, steps, decoupled=True, ema_decay=0.9, **hyper)
    live = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.AdamW(live, foreach=False, **hyper)
    snaps = [params]
    for k, gs in enumerate(steps):
        for p, g in zip(live, gs):
            p.grad = g.clone()
        opt.step()
        snaps.append(clip_adam_variants(params, steps[: k + 1], decoupled=True, ema_decay=0.9, **hyper)["p"])
    for i, q in enumerate(live):
        for got, ref in ((r["p"][i], q.detach()), (r["m"][i], opt.state[q]["exp_avg"]), (r["v"][i], opt.state[q]["exp_avg_sq"])):
            assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    assert r["vmax"] is None and r["step"] == 5
    for a, b in zip(ema_of(snaps, 0.9), r["ema"]):
        assert (a - b).abs().max().item() <= 1e-15
    coupled = clip_adam_variants(params, steps, ema_decay=0.9, **hyper)
    assert not torch.equal(coupled["p"][0], r["p"][0]) and not torch.equal(coupled["ema"][0], r["ema"][0])
    assert not torch.equal(r["ema"][0], r["p"][0])
    import test_gpu_flow_adam_variants as GV                     # (importing the GPU module needs no device)
    assert GV.VARIANTS["decoupled-ema"] == (dict(decoupled=True, ema_decay=0.9), GV.WD, None) and GV.WD > 0.0


# ---- FlowAdam's state format, on CPU tensors --------------------------------------------------------------------------------
HPS = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
NZ = 8


def make_net(seed=0):
    net = lsnf_amd._netF(HPS, nz=NZ)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net._param_list():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.1)
    return net


def set_grads(net, k):
    gen = torch.Generator().manual_seed(100 + k)
    for p in net._param_list():
        p.grad = torch.randn(p.shape, generator=gen) * (0.3 if k < 2 else 0.03)


@pytest.fixture
def on_cpu(monkeypatch):
    """FlowAdam keeps its state in views of one flat buffer: with the constructor's GPU check out of the way its state format
    can be exercised on CPU tensors (`step()` still has no CPU path)."""
    monkeypatch.setattr(lsnf_amd._netF, "_require_gpu", staticmethod(lambda params: None))


TORCH = {"adam": (torch.optim.Adam, {}), "amsgrad": (torch.optim.Adam, dict(amsgrad=True)), "adamw": (torch.optim.AdamW, {}),
         "adamw-amsgrad-maximize": (torch.optim.AdamW, dict(amsgrad=True, maximize=True))}


@pytest.mark.parametrize("variant", list(TORCH))
@pytest.mark.parametrize("ema_decay", [None, 0.9])
def test_state_dict_round_trips_with_torch_optimizers(on_cpu, variant, ema_decay):
    cls, kw = TORCH[variant]
    hyper = dict(lr=1e-3, betas=(0.5, 0.9), weight_decay=1e-2)
    net = make_net()
    topt = cls(net.parameters(), foreach=False, **hyper, **kw)
    for k in range(3):
        set_grads(net, k)
        topt.step()
    sd = topt.state_dict()
    decoupled, amsgrad = cls is torch.optim.AdamW, bool(kw.get("amsgrad"))
    # torch -> FlowAdam: built plain (Adam's decay), the checkpoint turns the decay decoupled and sets maximize
    opt = lsnf_amd.FlowAdam(net, amsgrad=amsgrad, ema_decay=ema_decay, **hyper)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert g["decoupled_weight_decay"] == decoupled and g["maximize"] == bool(kw.get("maximize")) and g["amsgrad"] == amsgrad
    assert g["ema_decay"] == ema_decay and opt._steps[0].item() == 3 and (opt._steps == 3).all()
    out = opt.state_dict()
    assert sorted(out["state"]) == sorted(sd["state"]) and len(out["state"]) == 24        # the dead fc_*.b carry no state
    want = {"step", "exp_avg", "exp_avg_sq"} | ({"max_exp_avg_sq"} if amsgrad else set()) | ({"ema"} if ema_decay else set())
    live = {id(p): p for p in net._param_list()}
    for pos, st in out["state"].items():
        assert set(st) == want and float(st["step"]) == 3.0
        for key in want - {"step", "ema"}:
            assert torch.equal(st[key], sd["state"][pos][key])
        if ema_decay:                        # no average in a torch checkpoint: it starts from the parameters as they are
            assert torch.equal(st["ema"], live[id(opt.param_groups[0]["params"][pos])].detach())
    og = out["param_groups"][0]
    assert og["amsgrad"] == amsgrad and og["decoupled_weight_decay"] == decoupled and og["maximize"] == bool(kw.get("maximize"))
    assert ("ema_decay" in og) == (ema_decay is not None) and "skip_nonfinite" not in og
    # FlowAdam -> torch: a fresh torch optimizer takes the dict and continues exactly as the one that made the state
    net2 = make_net()
    net2.load_state_dict(net.state_dict())
    topt2 = cls(net2.parameters(), foreach=False, lr=7.0)
    topt2.load_state_dict(out)
    assert topt2.param_groups[0]["lr"] == 1e-3 and topt2.param_groups[0]["amsgrad"] == amsgrad
    for n, o in ((net, topt), (net2, topt2)):
        set_grads(n, 3)
        o.step()
    assert all(torch.equal(a, b) for a, b in zip(net._param_list(), net2._param_list()))
    # copies, not aliases of the flat state
    out["state"][0]["exp_avg"].add_(1.0)
    assert not torch.equal(out["state"][0]["exp_avg"], opt.state_dict()["state"][0]["exp_avg"])


def test_plain_state_dict_is_what_it_was(on_cpu):
    net = make_net()
    opt = lsnf_amd.FlowAdam(net, lr=2e-3, betas=(0.5, 0.999), weight_decay=1e-2, max_norm=0.5)
    assert opt.state_dict() == {"state": {}, "param_groups": [dict(
        lr=2e-3, betas=(0.5, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=0.5, amsgrad=False, maximize=False, foreach=None,
        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False, params=list(range(28)))]}
    assert opt._flat.numel() * 4 == F.adam_state_bytes(NZ, 4, 2, 1)
    w = lsnf_amd.FlowAdamW(net, skip_nonfinite=True, ema_decay=0.999)
    g = w.state_dict()["param_groups"][0]
    assert g["decoupled_weight_decay"] is True and g["weight_decay"] == 1e-2 and g["skip_nonfinite"] is True and g["ema_decay"] == 0.999
    assert isinstance(w, lsnf_amd.FlowAdam) and w._flat.numel() * 4 == F.adam_state_bytes(NZ, 4, 2, 1, ema=True)
    assert w.skipped_steps.dtype == torch.int64 and w.skipped_steps.item() == 0 and len(w.ema_parameters()) == 24


def test_load_refuses_another_state_size(on_cpu):
    net = make_net()
    plain, ams, avg = lsnf_amd.FlowAdam(net), lsnf_amd.FlowAdam(net, amsgrad=True), lsnf_amd.FlowAdam(net, ema_decay=0.9)
    topt = torch.optim.Adam(net.parameters(), amsgrad=True, foreach=False)
    set_grads(net, 0)
    topt.step()
    with pytest.raises(lsnf_amd.LsnfError, match="amsgrad"):
        plain.load_state_dict(topt.state_dict())
    with pytest.raises(lsnf_amd.LsnfError, match="amsgrad"):
        ams.load_state_dict(torch.optim.Adam(net.parameters()).state_dict())
    with pytest.raises(lsnf_amd.LsnfError, match="average|ema"):
        plain.load_state_dict(avg.state_dict())
    ams.load_state_dict(topt.state_dict())
    avg.load_state_dict(plain.state_dict())                  # no word on an average: the decay is kept
    assert avg.param_groups[0]["ema_decay"] == 0.9
    for bad in (dict(ema_decay=1.0), dict(ema_decay=-0.1)):
        with pytest.raises(lsnf_amd.LsnfError):
            lsnf_amd.FlowAdam(net, **bad)
    with pytest.raises(lsnf_amd.LsnfError):
        plain.ema_parameters()


def test_ema_state_dict_and_copy(on_cpu):
    net, other = make_net(1), make_net(2)
    opt = lsnf_amd.FlowAdam(net, ema_decay=0.9)
    sd = opt.ema_state_dict()                                # before any step: the parameters themselves
    assert list(sd) == list(net.state_dict()) and len(sd) == len(net.state_dict())
    assert all(torch.equal(sd[k], v) for k, v in net.state_dict().items())
    # a loaded state with an average
    topt = torch.optim.Adam(net.parameters(), foreach=False)
    set_grads(net, 0)
    topt.step()
    st = topt.state_dict()
    for pos in st["state"]:
        st["state"][pos]["ema"] = torch.full_like(st["state"][pos]["exp_avg"], 0.25)
    opt.load_state_dict(st)
    sd = opt.ema_state_dict()
    live = {p.data_ptr() for p in net._param_list()}
    for k, v in net.state_dict().items():
        assert bool((sd[k] == 0.25).all()) if v.data_ptr() in live else torch.equal(sd[k], v)
    assert sum(v.data_ptr() in live for v in net.state_dict().values()) >= 24        # (some live tensors have two names)
    versions = [p._version for p in other._param_list()]
    opt.copy_ema_to(other)
    assert all(bool((p == 0.25).all()) for p in other._param_list())
    assert all(p._version > v for p, v in zip(other._param_list(), versions))
    other.load_state_dict(sd)                                # the form loads as a module state
    with pytest.raises(lsnf_amd.LsnfError):
        opt.copy_ema_to(net)


def test_cost_driver_child_compiles_and_the_driver_holds_no_gpu():
    """tools/flow_adam_variants_cost.py is a driver on tools/ab_harness.py like the others: its child's source is valid, and the
    driver itself never imports torch (it must not hold the GPU while its children are timed)."""
    import subprocess
    import sys
    tools = os.path.join(ROOT, "tools")
    code = ("import sys; sys.path.insert(0, %r)\nimport ab_harness, flow_adam_variants_cost as t\n"
            "compile(ab_harness.PRELUDE + t.CHILD, 'child', 'exec')\nassert 'torch' not in sys.modules\n"
            "assert set(t.DEFAULT) <= {'default', 'clip'}" % tools)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr

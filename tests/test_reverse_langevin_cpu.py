"""CPU: the fused base-space Langevin step without a GPU -- `lsnf_reverse_langevin_step` is declared / exported / bound, the Python
layers exist, and the entry point validates its arguments before any HIP call (every rejection is LSNF_E_ARG / LSNF_E_GEOMETRY
and names the entry point in lsnf_last_error()).  None of this holds without the feature."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT

import lsnf_amd

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2
NAME = "lsnf_reverse_langevin_step"
FAKE = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(10)]     # 16-byte aligned addresses that are never dereferenced on the host


def test_symbol_is_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, hdr)
    assert hasattr(lib, NAME)
    assert NAME in lsnf_amd._lib._SIGNATURES and NAME in lsnf_amd.exported_symbols()
    assert len(lsnf_amd._lib._SIGNATURES[NAME][1]) == 18
    assert lib.lsnf_abi_version() == 5                          # a symbol was added, nothing else changed


def test_python_layers_exist():
    assert callable(lsnf_amd.flow.reverse_langevin_step)
    sig = inspect.signature(lsnf_amd.flow.reverse_langevin_step)
    assert list(sig.parameters)[:7] == ["plan", "eps", "z_saved", "act_saved", "grad_g", "noise", "step_size"]
    for kw, default in (("inplace", False), ("out", None), ("want_g", False), ("want_norms", True)):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default == default
    assert inspect.isclass(lsnf_amd.langevin.GraphedEpsLangevinSampler)
    fused = inspect.signature(lsnf_amd.langevin.sample_langevin_post_eps_with_flow).parameters["fused"]
    assert fused.default is False                               # the default path stays what it was


def _named(lib):
    return NAME.encode() in lib.lsnf_last_error()


def test_validates_before_any_hip_call():
    lib = lsnf_amd.load_library()
    Rng = lsnf_amd._lib.LsnfRng
    plan, z_out, saved, act, grad_g, noise, eps_new, g_out, g_norm, e_norm = FAKE
    base = dict(nz=128, w=64, d=5, c=1, B=4, plan=plan, z_out=z_out, saved=saved, act=act, grad_g=grad_g, noise=None, rng=None,
                step=0.1, eps_new=eps_new, g_out=None, g_norm=None, e_norm=None)

    def call(**kw):
        a = dict(base, **kw)
        return lib.lsnf_reverse_langevin_step(a["plan"], a["nz"], a["w"], a["d"], a["c"], a["B"], a["z_out"], a["saved"], a["act"],
                                              a["grad_g"], a["noise"], None if a["rng"] is None else ctypes.byref(a["rng"]),
                                              a["step"], a["eps_new"], a["g_out"], a["g_norm"], a["e_norm"], None)

    def refused(**kw):
        return call(**kw) == LSNF_E_ARG and _named(lib)

    for geo in (dict(nz=130), dict(d=17), dict(nz=7, w=4), dict(c=2), dict(w=200)):
        assert call(**geo) == LSNF_E_GEOMETRY
    assert refused(B=-1)
    nulls = dict(plan=None, z_out=None, saved=None, act=None, grad_g=None, eps_new=None)
    assert call(B=0, **nulls) == LSNF_OK                        # empty batch: nothing to launch, NULL pointers allowed
    for name in ("plan", "z_out", "eps_new"):
        assert refused(**{name: None}) and b"NULL" in lib.lsnf_last_error()
    assert refused(act=None) and b"act_saved" in lib.lsnf_last_error()
    assert refused(saved=None) and b"NULL" in lib.lsnf_last_error()          # depth > 1 needs the block outputs
    assert refused(act=ctypes.c_void_p(0x40004)) and b"act_saved" in lib.lsnf_last_error()
    assert refused(plan=ctypes.c_void_p(0x10004)) and b"plan" in lib.lsnf_last_error()
    assert refused(z_out=ctypes.c_void_p(0x20002)) and b"4-byte" in lib.lsnf_last_error()
    assert refused(e_norm=ctypes.c_void_p(0xa0001)) and b"4-byte" in lib.lsnf_last_error()
    # the noise rules of lsnf_langevin_step; they hold for an empty batch too
    for B in (0, 4):
        assert refused(B=B, noise=noise, rng=Rng(1, 0, None, 0)) and b"not both" in lib.lsnf_last_error()
        assert refused(B=B, rng=Rng(1, 0, None, -1)) and b"row0" in lib.lsnf_last_error()
        assert refused(B=B, rng=Rng(1, 0, 0x30004, 0)) and b"offset_dev" in lib.lsnf_last_error()
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert refused(B=B, step=bad) and b"step_size" in lib.lsnf_last_error()
    # forbidden aliases of eps_new
    for kw in (dict(eps_new=grad_g), dict(eps_new=noise, noise=noise), dict(eps_new=saved), dict(eps_new=g_out, g_out=g_out)):
        for B in (0, 4):
            assert refused(B=B, **kw) and b"alias" in lib.lsnf_last_error()
    # ... of g_eps_out (the kernel stores it before it loads the noise, and reads z_out / z_saved on its way) and of the norms
    for kw in (dict(g_out=noise, noise=noise), dict(g_out=z_out), dict(g_out=saved)):
        for B in (0, 4):
            assert refused(B=B, **kw) and b"g_eps_out" in lib.lsnf_last_error()
    for kw in (dict(g_norm=z_out), dict(e_norm=grad_g), dict(g_norm=eps_new), dict(e_norm=noise, noise=noise), dict(g_norm=g_out, g_out=g_out),
               dict(g_norm=g_norm, e_norm=g_norm), dict(e_norm=saved)):
        for B in (0, 4):
            assert refused(B=B, **kw) and b"g_norm / eps_norm" in lib.lsnf_last_error()
    # allowed aliases: the in-place step, and g_eps_out over grad_g
    assert call(B=0, eps_new=z_out) == LSNF_OK
    assert call(B=0, g_out=grad_g) == LSNF_OK
    assert call(B=0, eps_new=z_out, g_out=grad_g, noise=noise, g_norm=g_norm, e_norm=e_norm) == LSNF_OK


def test_depth_one_needs_no_block_outputs_to_pass_the_null_check():
    lib = lsnf_amd.load_library()
    plan, z_out, _, act, _, _, eps_new = FAKE[:7]
    # (depth 1: z_saved may be NULL; the next rule -- a misaligned act_saved here -- is what refuses the call, still before any HIP call)
    rc = lib.lsnf_reverse_langevin_step(plan, 64, 32, 1, 1, 4, z_out, None, ctypes.c_void_p(0x40008), None, None, None, 0.1,
                                        eps_new, None, None, None, None)
    assert rc == LSNF_E_ARG and b"act_saved must be 16-byte aligned" in lib.lsnf_last_error()


def test_python_wrappers_have_no_cpu_path():
    import torch
    import types
    F = lsnf_amd.flow
    plan = F.FlowPlan(8, 4, 2, 1, torch.zeros(1), torch.zeros(1, dtype=torch.float64))
    eps, saved, act = torch.zeros(3, 8), torch.zeros(1, 3, 8), torch.zeros(64)
    with pytest.raises(lsnf_amd.LsnfError):
        F.reverse_langevin_step(plan, eps, saved, act, None, None, 0.1)
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    with pytest.raises(lsnf_amd.LsnfError):
        lsnf_amd.langevin.GraphedEpsLangevinSampler(torch.nn.Identity(), net, 3, 8, (3, 8, 1, 1), g_l_step_size=0.1, g_llhd_sigma=0.3)

"""CPU: the stash-keeping reverse without a GPU -- `lsnf_reverse_keep_covers`, `lsnf_reverse_keep` and `lsnf_sample_keep` are
declared / exported / bound, the coverage query needs no device, and both entry points validate their arguments before any HIP
call (every rejection is LSNF_E_ARG and names the entry point in lsnf_last_error()).  None of this holds without the feature."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

import lsnf_amd

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2
SYMBOLS = ("lsnf_reverse_keep_covers", "lsnf_reverse_keep", "lsnf_sample_keep")
FAKE = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]      # 16-byte aligned addresses that are never dereferenced on the host


def test_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name)
        assert name in lsnf_amd._lib._SIGNATURES and name in lsnf_amd.exported_symbols()
    assert lib.lsnf_abi_version() == 5                          # symbols were added, nothing else changed
    assert callable(lsnf_amd.flow.reverse_keep_supported)
    assert callable(lsnf_amd.langevin.sample_langevin_post_eps_with_flow)


def test_coverage_query_needs_no_device():
    lib = lsnf_amd.load_library()
    for bad in ((130, 64, 5, 1), (128, 64, 17, 1), (7, 4, 5, 1), (128, 64, 5, 2), (128, 200, 5, 1)):
        assert lib.lsnf_reverse_keep_covers(*bad, 100) == 0
    assert lib.lsnf_reverse_keep_covers(128, 64, 5, 1, -1) == 0
    F = lsnf_amd.flow
    prev_math = F.set_math_mode(F.MATH_BF16X3)
    prev_max = F.set_small_batch_max(F.SMALL_BATCH_AUTO)
    try:
        top = F.set_small_batch_max(-1)
        assert lib.lsnf_reverse_keep_covers(128, 64, 5, 1, 100) == 1
        assert lib.lsnf_reverse_keep_covers(128, 64, 5, 1, top) == 1 and lib.lsnf_reverse_keep_covers(128, 64, 5, 1, top + 1) == 0
        assert lib.lsnf_reverse_keep_covers(100, 128, 5, 1, 33) == 1 and lib.lsnf_reverse_keep_covers(2, 1, 1, 0, 1) == 1
        F.set_small_batch_max(64)
        assert lib.lsnf_reverse_keep_covers(128, 64, 5, 1, 64) == 1 and lib.lsnf_reverse_keep_covers(128, 64, 5, 1, 65) == 0
        F.set_small_batch_max(F.SMALL_BATCH_AUTO)
        F.set_math_mode(F.MATH_FP32)
        assert lib.lsnf_reverse_keep_covers(128, 64, 5, 1, 100) == 0
        F.set_math_mode(F.MATH_FP16X2)
        assert lib.lsnf_reverse_keep_covers(128, 64, 5, 1, 100) == 1
    finally:
        F.set_small_batch_max(prev_max)
        F.set_math_mode(prev_math)


def _named(lib, name):
    return name.encode() in lib.lsnf_last_error()


def test_reverse_keep_validates_before_any_hip_call():
    lib = lsnf_amd.load_library()
    plan, z_in, z_out, saved, act, ws = FAKE[:6]

    def call(nz=128, w=64, d=5, c=1, B=4, plan=plan, z_in=z_in, z_out=z_out, saved=None, act=None, ws=None):
        return lib.lsnf_reverse_keep(plan, nz, w, d, c, B, z_in, None, z_out, None, saved, act, ws, None)

    assert call(nz=130) == LSNF_E_GEOMETRY and call(d=17) == LSNF_E_GEOMETRY
    assert call(B=-1) == LSNF_E_ARG and _named(lib, "lsnf_reverse_keep")
    assert call(B=0, plan=None, z_in=None, z_out=None) == LSNF_OK          # empty batch: nothing to launch, NULL pointers allowed
    for kw in (dict(plan=None), dict(z_out=None), dict(z_in=None)):
        assert call(**kw) == LSNF_E_ARG and _named(lib, "lsnf_reverse_keep") and b"NULL" in lib.lsnf_last_error()
    assert call(z_out=ctypes.c_void_p(0x20002)) == LSNF_E_ARG and _named(lib, "lsnf_reverse_keep")
    assert call(saved=saved, act=ctypes.c_void_p(0x50004)) == LSNF_E_ARG and b"act_saved" in lib.lsnf_last_error()
    # params_workspace goes with act_saved (and, for depth > 1, z_saved)
    assert call(ws=ws) == LSNF_E_ARG and _named(lib, "lsnf_reverse_keep") and b"params_workspace" in lib.lsnf_last_error()
    assert call(ws=ws, saved=saved) == LSNF_E_ARG and b"params_workspace" in lib.lsnf_last_error()
    assert call(ws=ws, act=act) == LSNF_E_ARG and b"params_workspace" in lib.lsnf_last_error()
    assert call(saved=z_out, act=act) == LSNF_E_ARG and b"alias" in lib.lsnf_last_error()
    # an in-place call with a stash would overwrite the last block's output, which the backward reads
    assert call(z_out=z_in, saved=saved, act=act) == LSNF_E_ARG and b"z_in" in lib.lsnf_last_error()
    assert call(z_out=z_in, act=act) == LSNF_E_ARG and _named(lib, "lsnf_reverse_keep")
    # outside the coverage rule: refused, whatever is kept
    F = lsnf_amd.flow
    prev = F.set_math_mode(F.MATH_FP32)
    try:
        assert call(saved=saved, act=act) == LSNF_E_ARG and _named(lib, "lsnf_reverse_keep")
        assert call() == LSNF_E_ARG and _named(lib, "lsnf_reverse_keep")
    finally:
        F.set_math_mode(prev)


def test_sample_keep_validates_before_any_hip_call():
    lib = lsnf_amd.load_library()
    Rng = lsnf_amd._lib.LsnfRng
    plan, z_out, eps, saved, act, ws = FAKE[:6]

    def call(nz=128, w=64, d=5, c=1, B=4, rng=Rng(1, 0, None, 0), T=1.0, plan=plan, z_out=z_out, eps=None, saved=None, act=None, ws=None):
        return lib.lsnf_sample_keep(plan, nz, w, d, c, B, None if rng is None else ctypes.byref(rng), T, z_out, None, eps, None,
                                    saved, act, ws, None)

    assert call(nz=130) == LSNF_E_GEOMETRY
    assert call(B=-1) == LSNF_E_ARG and _named(lib, "lsnf_sample_keep")
    assert call(B=0, plan=None, z_out=None) == LSNF_OK
    for B in (0, 4):                                            # the generator's rules hold for an empty batch too, as lsnf_sample's
        assert call(B=B, rng=None) == LSNF_E_ARG and b"rng" in lib.lsnf_last_error()
        assert call(B=B, rng=Rng(1, 0, None, -1)) == LSNF_E_ARG and b"row0" in lib.lsnf_last_error()
        assert call(B=B, T=float("nan")) == LSNF_E_ARG and b"temperature" in lib.lsnf_last_error()
    for kw in (dict(plan=None), dict(z_out=None)):
        assert call(**kw) == LSNF_E_ARG and _named(lib, "lsnf_sample_keep") and b"NULL" in lib.lsnf_last_error()
    assert call(eps=z_out) == LSNF_E_ARG and b"alias" in lib.lsnf_last_error()
    # a stash without eps_out: the backward would lack the last block's output
    for kw in (dict(act=act), dict(saved=saved), dict(act=act, saved=saved)):
        assert call(**kw) == LSNF_E_ARG and _named(lib, "lsnf_sample_keep") and b"eps_out" in lib.lsnf_last_error()
    assert call(eps=eps, ws=ws) == LSNF_E_ARG and _named(lib, "lsnf_sample_keep") and b"params_workspace" in lib.lsnf_last_error()
    assert call(eps=eps, ws=ws, saved=saved) == LSNF_E_ARG and b"params_workspace" in lib.lsnf_last_error()
    F = lsnf_amd.flow
    prev = F.set_math_mode(F.MATH_FP32)
    try:
        assert call(eps=eps, saved=saved, act=act) == LSNF_E_ARG and _named(lib, "lsnf_sample_keep")
    finally:
        F.set_math_mode(prev)


def test_python_wrappers_have_no_cpu_path():
    import torch
    import types
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=8, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    assert net.reverse_keeps_stash is False
    net.reverse_keeps_stash = True
    with pytest.raises(lsnf_amd.LsnfError):
        net(torch.zeros(3, 8, requires_grad=True), torch.zeros(3), reverse=True)

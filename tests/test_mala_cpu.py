"""CPU: the Metropolis-adjusted Langevin step without a GPU -- `lsnf_mala_step` is declared in include/lsnf_flow_mcmc.h, exported and
bound from the extension table (outside the core ABI's symbol set), the Python layers exist and have no CPU path, the entry point
validates its arguments before any HIP call (every refusal is LSNF_E_ARG / LSNF_E_GEOMETRY, names the entry point and the
offending argument in lsnf_last_error()), and the float64 restatement the GPU tests compare with (tests/mala_restated.py) leaves
its target invariant.  None of this holds without the feature."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import flow_oracle as O
import mala_restated as M

import lsnf_amd

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2
NAME = "lsnf_mala_step"
FAKE = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(16)]     # 16-byte aligned addresses that are never dereferenced on the host


def test_symbol_is_declared_exported_and_bound_outside_the_core_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow_mcmc.h")).read(), flags=re.S)
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, hdr) and re.search(r"#define\s+LSNF_MALA_INIT\s+1u", hdr)
    assert '#include "lsnf_flow.h"' in hdr and NAME not in core
    assert hasattr(lib, NAME)
    ext = lsnf_amd._lib._EXT_SIGNATURES
    assert NAME in ext and len(ext[NAME][1]) == 25 and lsnf_amd._lib.extension_symbols() == sorted(ext)
    assert NAME not in lsnf_amd.exported_symbols() and NAME not in lsnf_amd._lib._SIGNATURES
    assert lib.lsnf_mala_step.argtypes == ext[NAME][1]              # attached in load()
    assert lib.lsnf_abi_version() == 5 and lsnf_amd._lib.ABI_VERSION == 5
    assert lsnf_amd.flow.MALA_INIT == 1


def test_a_library_without_the_symbol_does_not_load(monkeypatch):
    L = lsnf_amd._lib
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setitem(L._EXT_SIGNATURES, "lsnf_no_such_extension", (ctypes.c_int, []))
    with pytest.raises(AttributeError):
        L.load()


def test_python_layers_exist():
    F, L = lsnf_amd.flow, lsnf_amd.langevin
    sig = inspect.signature(F.mala_step)
    assert list(sig.parameters)[:7] == ["plan", "z_prop", "grad_g", "energy_g", "state", "noise", "step_size"]
    for kw, default in (("init", False), ("uniform", None), ("propose", True), ("inplace", False), ("reuse_buffers", False)):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default == default
    assert [f for f in F.MalaState.__dataclass_fields__] == ["z", "grad", "energy"] and callable(F.new_mala_state)
    assert callable(lsnf_amd._netF.mala_step)
    sig = inspect.signature(L.sample_mala_post_z_with_flow)
    assert list(sig.parameters)[:4] == ["z", "x", "netG", "netF"]
    for kw in ("g_l_steps", "g_l_step_size", "g_llhd_sigma", "philox"):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
    # the existing samplers keep their defaults
    old = inspect.signature(L.sample_langevin_post_z_with_flow).parameters
    assert old["g_l_with_noise"].default is True and old["philox"].default is None


ARGS = ("plan", "z_prop", "z_out", "saved", "act", "ll", "grad_g", "energy", "z_acc", "g_acc", "u_acc", "noise", "uniform")


def _caller(lib):
    Rng = lsnf_amd._lib.LsnfRng
    ptrs = dict(zip(ARGS + ("z_next", "accept", "la"), FAKE))
    base = dict(ptrs, nz=128, w=64, d=5, c=1, B=4, rng=None, step=0.9, flags=0, accept=None, la=None)

    def call(**kw):
        a = dict(base, **kw)
        return lib.lsnf_mala_step(a["plan"], a["nz"], a["w"], a["d"], a["c"], a["B"], a["z_prop"], a["z_out"], a["saved"], a["act"],
                                  a["ll"], a["grad_g"], a["energy"], a["z_acc"], a["g_acc"], a["u_acc"], a["noise"], a["uniform"],
                                  None if a["rng"] is None else ctypes.byref(a["rng"]), a["step"], a["flags"], a["z_next"],
                                  a["accept"], a["la"], None)

    def refused(word, **kw):
        err = lib.lsnf_last_error
        return call(**kw) == LSNF_E_ARG and NAME.encode() in err() and word.encode() in err()
    return call, refused, ptrs, Rng


def test_validates_before_any_hip_call():
    lib = lsnf_amd.load_library()
    call, refused, P, Rng = _caller(lib)
    for geo in (dict(nz=130), dict(d=17), dict(nz=7, w=4), dict(c=2), dict(w=200)):
        assert call(**geo) == LSNF_E_GEOMETRY and b"unsupported geometry" in lib.lsnf_last_error()      # (the shared rule's wording)
        assert call(B=0, **geo) == LSNF_E_GEOMETRY
    assert refused("B=-1", B=-1)
    nulls = {k: None for k in ARGS + ("z_next",)}
    assert call(B=0, **nulls) == LSNF_OK                        # empty batch: nothing to launch, NULL pointers allowed
    # rules that precede the empty-batch return: the same answer for B = 0
    tensors = dict(noise=None, uniform=None)
    for B in (0, 4):
        assert refused("not both", B=B, uniform=None, rng=Rng(1, 0, None, 0)) and b"noise" in lib.lsnf_last_error()
        assert refused("not both", B=B, noise=None, rng=Rng(1, 0, None, 0)) and b"uniform" in lib.lsnf_last_error()
        assert refused("row0", B=B, rng=Rng(1, 0, None, -1), **tensors)
        assert refused("offset_dev", B=B, rng=Rng(1, 0, 0x30004, 0), **tensors)
        for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -0.0):
            assert refused("step_size", B=B, step=bad)
        for bad in (2, 3, 0x80000000):
            assert refused("flag", B=B, flags=bad)
        # aliases: no output may be a tensor the call reads, or another output; the message names both
        for out in ("z_acc", "g_acc", "u_acc", "z_next", "accept", "la"):
            wording = {"g_acc": "grad_acc", "accept": "accept_out", "la": "log_alpha_out"}.get(out, out)
            for src in ARGS:
                if src in ("z_acc", "g_acc", "u_acc") or (out, src) == ("z_next", "z_prop"):
                    continue
                assert refused("alias", B=B, **{out: P[src]}) and wording.encode() in lib.lsnf_last_error()
            for other in ("z_acc", "g_acc", "u_acc", "z_next"):
                if other != out:
                    assert refused("alias", B=B, **{out: P[other]}) and wording.encode() in lib.lsnf_last_error()
        assert refused("alias", B=B, accept=P["la"], la=P["la"])
    # the allowed alias: the next proposal over the proposal
    assert call(B=0, z_next=P["z_prop"]) == LSNF_OK
    assert call(B=0, z_next=P["z_prop"], accept=P["accept"], la=P["la"]) == LSNF_OK
    # required pointers, each named
    for arg, word in (("plan", "plan"), ("z_prop", "z_prop"), ("z_out", "z_out"), ("act", "act_saved"), ("ll", "ll_prop"),
                      ("z_acc", "z_acc"), ("g_acc", "grad_acc"), ("u_acc", "u_acc"), ("saved", "z_saved")):
        assert refused(word, **{arg: None}) and b"NULL" in lib.lsnf_last_error()
    # without an rng: the uniform unless INIT, the noise iff a proposal is asked for
    assert refused("uniform", uniform=None)
    assert refused("noise", noise=None)
    assert refused("noise", z_next=None)
    # alignment: 16 bytes for plan and act_saved, 4 bytes for every tensor, each named
    assert refused("plan must be 16-byte", plan=ctypes.c_void_p(0x10004))
    assert refused("act_saved must be 16-byte", act=ctypes.c_void_p(0x50008))
    for arg, word in (("z_prop", "z_prop"), ("z_out", "z_out"), ("saved", "z_saved"), ("ll", "ll_prop"), ("grad_g", "grad_g"),
                      ("energy", "energy_g"), ("z_acc", "z_acc"), ("g_acc", "grad_acc"), ("u_acc", "u_acc"), ("noise", "noise"),
                      ("uniform", "uniform"), ("z_next", "z_next"), ("accept", "accept_out"), ("la", "log_alpha_out")):
        assert refused(word + " must be 4-byte", **{arg: ctypes.c_void_p(0xF00002)})


def test_depth_one_and_init_pass_the_pointer_rules():
    lib = lsnf_amd.load_library()
    call, refused, P, Rng = _caller(lib)
    # (the next rule -- a misaligned act_saved here -- is what refuses these calls, still before any HIP call)
    bad_act = ctypes.c_void_p(0x50008)
    assert refused("act_saved must be 16-byte", nz=64, w=32, d=1, saved=None, act=bad_act)           # depth 1: no block outputs
    assert refused("act_saved must be 16-byte", flags=1, uniform=None, act=bad_act)                  # INIT: no uniform
    assert refused("act_saved must be 16-byte", noise=None, z_next=None, act=bad_act)                # deciding only: no noise
    assert refused("act_saved must be 16-byte", noise=None, uniform=None, rng=Rng(1, 0, None, 0), act=bad_act)
    assert refused("act_saved must be 16-byte", grad_g=None, energy=None, act=bad_act)               # the prior alone


def test_every_rule_speaks_word_for_word():
    """One call per rule: the first violated rule speaks, and lsnf_last_error() is this text to the letter."""
    lib = lsnf_amd.load_library()
    call, _, P, Rng = _caller(lib)
    table = (
        (dict(B=-1), 'lsnf_mala_step: B=-1 out of range'),
        (dict(B=0, noise=None, rng=Rng(1, 0, None, 0)), 'lsnf_mala_step: pass either a uniform tensor or an rng, not both'),
        (dict(uniform=None, rng=Rng(1, 0, None, 0)), 'lsnf_mala_step: pass either a noise tensor or an rng, not both'),
        (dict(B=0, noise=None, uniform=None, rng=Rng(1, 0, None, -1)), 'lsnf_mala_step: rng->row0 must be >= 0'),
        (dict(noise=None, uniform=None, rng=Rng(1, 0, 0x30004, 0)), 'lsnf_mala_step: rng->offset_dev must be 8-byte aligned'),
        (dict(step=float('nan')), 'lsnf_mala_step: step_size must be finite and non-zero (got nan)'),
        (dict(B=0, step=0.0), 'lsnf_mala_step: step_size must be finite and non-zero (got 0)'),
        (dict(flags=2), 'lsnf_mala_step: unknown flag bits 0x2'),
        (dict(B=0, flags=0x80000003), 'lsnf_mala_step: unknown flag bits 0x80000002'),
        (dict(z_acc=P['grad_g']), 'lsnf_mala_step: z_acc must not alias grad_g'),
        (dict(B=0, z_next=P['z_out']), 'lsnf_mala_step: z_next must not alias z_out'),
        (dict(u_acc=P['uniform']), 'lsnf_mala_step: u_acc must not alias uniform'),
        (dict(g_acc=P['z_next']), 'lsnf_mala_step: grad_acc must not alias z_next'),
        (dict(accept=P['la'], la=P['la']), 'lsnf_mala_step: accept_out must not alias log_alpha_out'),
        (dict(la=P['z_acc']), 'lsnf_mala_step: z_acc must not alias log_alpha_out'),
        (dict(plan=None), 'lsnf_mala_step: plan is required (NULL)'),
        (dict(ll=None), 'lsnf_mala_step: ll_prop is required (NULL)'),
        (dict(u_acc=None), 'lsnf_mala_step: u_acc is required (NULL)'),
        (dict(saved=None), 'lsnf_mala_step: z_saved is required (NULL) for depth > 1'),
        (dict(uniform=None), 'lsnf_mala_step: uniform is required without an rng (unless LSNF_MALA_INIT)'),
        (dict(noise=None), 'lsnf_mala_step: noise is required with z_next when no rng is given'),
        (dict(z_next=None), 'lsnf_mala_step: noise goes with z_next: nothing is proposed without it'),
        (dict(plan=ctypes.c_void_p(0x10004)), 'lsnf_mala_step: plan must be 16-byte aligned'),
        (dict(act=ctypes.c_void_p(0x50008)), 'lsnf_mala_step: act_saved must be 16-byte aligned'),
        (dict(grad_g=ctypes.c_void_p(0xF00002)), 'lsnf_mala_step: grad_g must be 4-byte aligned'),
        (dict(la=ctypes.c_void_p(0xF00002)), 'lsnf_mala_step: log_alpha_out must be 4-byte aligned'),
    )
    for kw, message in table:
        assert call(**kw) == LSNF_E_ARG and lib.lsnf_last_error().decode() == message, (kw, lib.lsnf_last_error())


def test_python_wrappers_have_no_cpu_path():
    F = lsnf_amd.flow
    plan = F.FlowPlan(8, 4, 2, 1, torch.zeros(1), torch.zeros(1, dtype=torch.float64))
    z = torch.zeros(3, 8)
    state = F.MalaState(torch.zeros(3, 8), torch.zeros(3, 8), torch.zeros(3))
    with pytest.raises(lsnf_amd.LsnfError):
        F.mala_step(plan, z, None, None, state, F.PhiloxNoise(1), 0.5, init=True)
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    with pytest.raises(lsnf_amd.LsnfError):
        net.mala_step(z, None, None, state, F.PhiloxNoise(1), 0.5, init=True)
    with pytest.raises(lsnf_amd.LsnfError):
        lsnf_amd.langevin.sample_mala_post_z_with_flow(z.view(3, 8, 1, 1), torch.zeros(3, 8), torch.nn.Flatten(), net, g_l_steps=2,
                                                       g_l_step_size=0.5, g_llhd_sigma=0.3, philox=F.PhiloxNoise(1))


def test_cpu_tensors_are_refused_before_any_launch(monkeypatch):
    """tests/test_flow_checks_cpu.py's rule for the wrappers of flow.py, for the ones of mcmc.py (re-exported as flow.mala_step ...)."""
    from counting_lib import install
    F = lsnf_amd.flow
    assert F.mala_step is lsnf_amd.mcmc.mala_step and F.MalaState is lsnf_amd.mcmc.MalaState and F.new_mala_state is lsnf_amd.mcmc.new_mala_state
    lib = lsnf_amd.load_library()
    plan = F.FlowPlan(8, 4, 2, 1, torch.zeros(lib.lsnf_plan_floats(8, 4, 2, 1)), torch.zeros(lib.lsnf_prepare_scratch_bytes(8, 4, 2) // 8, dtype=torch.float64))
    stand = install(monkeypatch, lsnf_amd)
    z, v = torch.zeros(5, 8), torch.zeros(5)
    for kw in (dict(init=True), dict(uniform=v), dict(propose=False, inplace=True)):
        with pytest.raises(lsnf_amd.LsnfError):
            F.mala_step(plan, z, z.clone(), v, F.new_mala_state(plan, 5, "cpu"), F.PhiloxNoise(3), 0.5, **kw)
    with pytest.raises(lsnf_amd.LsnfError):
        F.mala_step(plan, z, None, None, (z, z, v), F.PhiloxNoise(3), 0.5)                  # the state is a MalaState
    assert stand.launching() == [], dict(stand.entered)


def test_restated_uniform_is_its_own_stream_in_fp32():
    u = M.uniform_draws(4096, seed=1234, offset=40, row0=0)
    assert u.dtype == np.float32 and (u > 0).all() and (u < 1).all() and abs(float(u.mean()) - 0.5) < 4 / np.sqrt(12 * 4096)
    assert np.array_equal(M.uniform_draws(100, 1234, 40, row0=60), u[60:160])                # a function of the global row
    assert not np.array_equal(M.uniform_draws(100, 1234, 41), u[:100]) and not np.array_equal(M.uniform_draws(100, 1235, 40), u[:100])
    from oracle.philox_oracle import philox4x32_10
    x0 = philox4x32_10(2 << 16, np.arange(8), 40, 0, 1234, 0)[0]
    exact = ((x0 >> 8).astype(np.float64) + 0.5) * 2.0 ** -24
    assert np.abs(u[:8].astype(np.float64) - exact).max() <= 2.0 ** -25                     # (x + 0.5 has 25 bits: one fp32 rounding)
    assert np.array_equal(u[:8], (((x0 >> 8).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)))


def test_restated_chain_leaves_its_target_invariant():
    """20 000 float64 rows started from exact prior samples, 5 Metropolis-adjusted steps, the prior alone: the mean of ll must not
    drift beyond 4 standard errors (the standard error of a difference of two means, without credit for their correlation)."""
    nz, B, K, s = 2, 20000, 5, 1.0
    p = O.init_params(nz, 4, 1, seed=5, fcz_std=0.5, dtype=torch.float64)
    g = torch.Generator().manual_seed(11)
    z0 = O.flow_reverse(p, torch.randn(B, nz, generator=g, dtype=torch.float64), torch.zeros(B, dtype=torch.float64))[0]
    noises = [torch.randn(B, nz, generator=g, dtype=torch.float64) for _ in range(K)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g, dtype=torch.float64).clamp_min(1e-300) for _ in range(K)]
    steps, (zk, _, uk) = M.chain(p, z0, None, s, noises, uniforms)
    ll0, llk = O.flow_log_prob(p, z0)[2], -uk
    assert torch.allclose(llk, O.flow_log_prob(p, zk)[2], rtol=0, atol=1e-12)               # the kept energy is U of the kept point
    rate = torch.stack([st.acc for st in steps]).double().mean().item()
    se = float(torch.sqrt(ll0.var() / B + llk.var() / B))
    drift = abs(float(llk.mean() - ll0.mean()))
    print(f"[mala] invariance: acceptance {rate:.3f}, mean ll {ll0.mean():.5f} -> {llk.mean():.5f}, drift {drift:.2e}, 4 SE {4 * se:.2e}")
    assert 0.15 < rate < 0.98 and drift <= 4.0 * se
    # the same proposals without the correction do drift: the check above is not vacuous
    z = z0
    for n in noises[:-1]:
        z = M.propose(z, M.potential(p, z, None, torch.float64)[1], n, s)
    assert abs(float(O.flow_log_prob(p, z)[2].mean() - ll0.mean())) > 4.0 * se


def test_cost_tool_is_a_driver_on_the_ab_harness():
    """tools/mala_step_vs_langevin_step.py: its child's source is valid and importing the driver does not import torch."""
    import subprocess
    import sys
    tools = os.path.join(ROOT, "tools")
    code = ("import sys; sys.path.insert(0, %r)\nimport ab_harness, mala_step_vs_langevin_step as t\n"
            "compile(ab_harness.PRELUDE + t.CHILD, 'child', 'exec')\nassert 'torch' not in sys.modules\n"
            "assert t.SIZES == (100, 16384)" % tools)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=60)

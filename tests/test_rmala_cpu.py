"""CPU: the base-space Metropolis-adjusted Langevin step without a GPU -- `lsnf_reverse_mala_step` is declared in
include/lsnf_flow_mcmc.h, exported and bound from the extension table (outside the core ABI's symbol set), the Python layers exist
with their signatures and have no CPU path, the entry point validates its arguments before any HIP call (every refusal is
LSNF_E_ARG / LSNF_E_GEOMETRY and names the entry point and the offending argument in lsnf_last_error()), and the float64
restatement the GPU tests compare with (tests/rmala_restated.py) is the step it claims to be.  None of this holds without the
feature."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from oracle import flow_oracle as O
import rmala_restated as RM

import lsnf_amd

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2
NAME = "lsnf_reverse_mala_step"
FAKE = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(16)]     # 16-byte aligned addresses that are never dereferenced on the host


def test_symbol_is_declared_exported_and_bound_outside_the_core_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow_mcmc.h")).read(), flags=re.S)
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, hdr) and NAME not in core
    assert hasattr(lib, NAME)
    ext = lsnf_amd._lib._EXT_SIGNATURES
    assert NAME in ext and len(ext[NAME][1]) == 23 and NAME in lsnf_amd._lib.extension_symbols()
    assert NAME not in lsnf_amd.exported_symbols() and NAME not in lsnf_amd._lib._SIGNATURES
    assert lib.lsnf_reverse_mala_step.argtypes == ext[NAME][1]      # attached in load()
    assert lib.lsnf_abi_version() == 5 and lsnf_amd._lib.ABI_VERSION == 5
    # the declaration's 23 parameters, in the order of the bound signature
    decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, hdr, flags=re.S).group(1)
    names = [re.sub(r".*[\s*]", "", a.strip()) for a in decl.split(",")]
    assert names == ["plan", "nz", "width", "depth", "coupling", "B", "eps_prop", "z_saved", "act_saved", "grad_g", "energy_g",
                     "eps_acc", "grad_acc", "u_acc", "noise", "uniform", "rng", "step_size", "flags", "eps_next", "accept_out",
                     "log_alpha_out", "stream"]


def test_python_layers_exist():
    F, L = lsnf_amd.flow, lsnf_amd.langevin
    assert F.reverse_mala_step is lsnf_amd.mcmc.reverse_mala_step
    sig = inspect.signature(F.reverse_mala_step)
    assert list(sig.parameters)[:9] == ["plan", "eps_prop", "z_saved", "act_saved", "grad_g", "energy_g", "state", "noise", "step_size"]
    for kw, default in (("init", False), ("uniform", None), ("propose", True), ("inplace", False), ("reuse_buffers", False)):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default == default
    assert [f for f in F.MalaState.__dataclass_fields__] == ["z", "grad", "energy"] and "eps" in F.MalaState.__doc__
    sig = inspect.signature(lsnf_amd._netF.reverse_mala_step)
    assert list(sig.parameters)[:4] == ["self", "eps_prop", "z_saved", "act_saved"]
    sig = inspect.signature(L.sample_mala_post_eps_with_flow)
    assert list(sig.parameters) == ["eps", "x", "netG", "netF", "g_l_steps", "g_l_step_size", "g_llhd_sigma", "philox"]
    for kw in ("g_l_steps", "g_l_step_size", "g_llhd_sigma", "philox"):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
    # the existing samplers and steps keep their signatures
    old = inspect.signature(L.sample_langevin_post_eps_with_flow).parameters
    assert list(old) == ["eps", "x", "netG", "netF", "g_l_steps", "g_l_step_size", "g_llhd_sigma", "noise", "philox", "fused"]
    assert old["noise"].default is True and old["philox"].default is None and old["fused"].default is False
    old = inspect.signature(L.sample_mala_post_z_with_flow).parameters
    assert list(old) == ["z", "x", "netG", "netF", "g_l_steps", "g_l_step_size", "g_llhd_sigma", "philox"]
    old = inspect.signature(L.sample_langevin_post_z_with_flow).parameters
    assert old["g_l_with_noise"].default is True and old["philox"].default is None
    assert list(inspect.signature(F.mala_step).parameters)[:7] == ["plan", "z_prop", "grad_g", "energy_g", "state", "noise", "step_size"]
    assert list(inspect.signature(F.reverse_langevin_step).parameters)[:7] == ["plan", "eps", "z_saved", "act_saved", "grad_g", "noise", "step_size"]


ARGS = ("plan", "eps_prop", "saved", "act", "grad_g", "energy", "eps_acc", "g_acc", "u_acc", "noise", "uniform")
WORD = {"saved": "z_saved", "act": "act_saved", "energy": "energy_g", "g_acc": "grad_acc", "accept": "accept_out", "la": "log_alpha_out"}


def _caller(lib):
    Rng = lsnf_amd._lib.LsnfRng
    ptrs = dict(zip(ARGS + ("eps_next", "accept", "la"), FAKE))
    base = dict(ptrs, nz=128, w=64, d=5, c=1, B=4, rng=None, step=0.9, flags=0, accept=None, la=None)

    def call(**kw):
        a = dict(base, **kw)
        return lib.lsnf_reverse_mala_step(a["plan"], a["nz"], a["w"], a["d"], a["c"], a["B"], a["eps_prop"], a["saved"], a["act"],
                                          a["grad_g"], a["energy"], a["eps_acc"], a["g_acc"], a["u_acc"], a["noise"], a["uniform"],
                                          None if a["rng"] is None else ctypes.byref(a["rng"]), a["step"], a["flags"], a["eps_next"],
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
    nulls = {k: None for k in ARGS + ("eps_next",)}
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
        for out in ("eps_acc", "g_acc", "u_acc", "eps_next", "accept", "la"):
            wording = WORD.get(out, out)
            for src in ARGS:
                if src in ("eps_acc", "g_acc", "u_acc") or (out, src) == ("eps_next", "eps_prop"):
                    continue
                assert refused("alias", B=B, **{out: P[src]}) and wording.encode() in lib.lsnf_last_error()
                assert WORD.get(src, src).encode() in lib.lsnf_last_error()
            for other in ("eps_acc", "g_acc", "u_acc", "eps_next"):
                if other != out:
                    assert refused("alias", B=B, **{out: P[other]}) and wording.encode() in lib.lsnf_last_error()
        assert refused("alias", B=B, accept=P["la"], la=P["la"])
    # the allowed alias: the next proposal over the proposal
    assert call(B=0, eps_next=P["eps_prop"]) == LSNF_OK
    assert call(B=0, eps_next=P["eps_prop"], accept=P["accept"], la=P["la"]) == LSNF_OK
    # required pointers, each named
    for arg, word in (("plan", "plan"), ("eps_prop", "eps_prop"), ("act", "act_saved"), ("eps_acc", "eps_acc"), ("g_acc", "grad_acc"),
                      ("u_acc", "u_acc"), ("saved", "z_saved")):
        assert refused(word, **{arg: None}) and b"required" in lib.lsnf_last_error()
    # without an rng: the uniform unless INIT, the noise iff a proposal is asked for
    assert refused("uniform", uniform=None)
    assert refused("noise", noise=None)
    assert refused("noise", eps_next=None)
    # alignment as lsnf_reverse_backward_z: 16 bytes for plan and act_saved, 4 bytes for every tensor, each named
    assert refused("plan must be 16-byte", plan=ctypes.c_void_p(0x10004))
    assert refused("act_saved must be 16-byte", act=ctypes.c_void_p(0x50008))
    for arg in ("eps_prop", "saved", "grad_g", "energy", "eps_acc", "g_acc", "u_acc", "noise", "uniform", "eps_next", "accept", "la"):
        assert refused(WORD.get(arg, arg) + " must be 4-byte", **{arg: ctypes.c_void_p(0xF00002)})


def test_depth_one_and_init_pass_the_pointer_rules():
    lib = lsnf_amd.load_library()
    call, refused, P, Rng = _caller(lib)
    # (the next rule -- a misaligned act_saved here -- is what refuses these calls, still before any HIP call)
    bad_act = ctypes.c_void_p(0x50008)
    assert refused("act_saved must be 16-byte", nz=64, w=32, d=1, saved=None, act=bad_act)           # depth 1: no block outputs
    assert refused("act_saved must be 16-byte", flags=1, uniform=None, act=bad_act)                  # INIT: no uniform
    assert refused("act_saved must be 16-byte", noise=None, eps_next=None, act=bad_act)              # deciding only: no noise
    assert refused("act_saved must be 16-byte", noise=None, uniform=None, rng=Rng(1, 0, None, 0), act=bad_act)
    assert refused("act_saved must be 16-byte", grad_g=None, energy=None, act=bad_act)               # the prior alone


def test_every_rule_speaks_word_for_word():
    """One call per rule: the first violated rule speaks, and lsnf_last_error() is this text to the letter."""
    lib = lsnf_amd.load_library()
    call, _, P, Rng = _caller(lib)
    stash = 'lsnf_reverse_mala_step: act_saved is required (the stash of lsnf_forward, lsnf_restash or lsnf_reverse_keep)'
    table = (
        (dict(B=-1), 'lsnf_reverse_mala_step: B=-1 out of range'),
        (dict(B=0, noise=None, rng=Rng(1, 0, None, 0)), 'lsnf_reverse_mala_step: pass either a uniform tensor or an rng, not both'),
        (dict(uniform=None, rng=Rng(1, 0, None, 0)), 'lsnf_reverse_mala_step: pass either a noise tensor or an rng, not both'),
        (dict(B=0, noise=None, uniform=None, rng=Rng(1, 0, None, -1)), 'lsnf_reverse_mala_step: rng->row0 must be >= 0'),
        (dict(noise=None, uniform=None, rng=Rng(1, 0, 0x30004, 0)), 'lsnf_reverse_mala_step: rng->offset_dev must be 8-byte aligned'),
        (dict(step=float('nan')), 'lsnf_reverse_mala_step: step_size must be finite and non-zero (got nan)'),
        (dict(B=0, step=0.0), 'lsnf_reverse_mala_step: step_size must be finite and non-zero (got 0)'),
        (dict(flags=2), 'lsnf_reverse_mala_step: unknown flag bits 0x2'),
        (dict(B=0, flags=0x80000003), 'lsnf_reverse_mala_step: unknown flag bits 0x80000002'),
        (dict(eps_acc=P['grad_g']), 'lsnf_reverse_mala_step: eps_acc must not alias grad_g'),
        (dict(B=0, eps_next=P['saved']), 'lsnf_reverse_mala_step: eps_next must not alias z_saved'),
        (dict(u_acc=P['uniform']), 'lsnf_reverse_mala_step: u_acc must not alias uniform'),
        (dict(g_acc=P['eps_next']), 'lsnf_reverse_mala_step: grad_acc must not alias eps_next'),
        (dict(accept=P['la'], la=P['la']), 'lsnf_reverse_mala_step: accept_out must not alias log_alpha_out'),
        (dict(la=P['eps_acc']), 'lsnf_reverse_mala_step: eps_acc must not alias log_alpha_out'),
        (dict(plan=None), 'lsnf_reverse_mala_step: plan is required (NULL)'),
        (dict(eps_prop=None), 'lsnf_reverse_mala_step: eps_prop is required (NULL)'),
        (dict(u_acc=None), 'lsnf_reverse_mala_step: u_acc is required (NULL)'),
        (dict(act=None), stash),
        (dict(act=None, saved=None), stash),
        (dict(saved=None), 'lsnf_reverse_mala_step: z_saved is required (NULL) for depth > 1'),
        (dict(uniform=None), 'lsnf_reverse_mala_step: uniform is required without an rng (unless LSNF_MALA_INIT)'),
        (dict(noise=None), 'lsnf_reverse_mala_step: noise is required with eps_next when no rng is given'),
        (dict(eps_next=None), 'lsnf_reverse_mala_step: noise goes with eps_next: nothing is proposed without it'),
        (dict(plan=ctypes.c_void_p(0x10004)), 'lsnf_reverse_mala_step: plan must be 16-byte aligned'),
        (dict(act=ctypes.c_void_p(0x50008)), 'lsnf_reverse_mala_step: act_saved must be 16-byte aligned'),
        (dict(energy=ctypes.c_void_p(0xF00002)), 'lsnf_reverse_mala_step: energy_g must be 4-byte aligned'),
        (dict(accept=ctypes.c_void_p(0xF00002)), 'lsnf_reverse_mala_step: accept_out must be 4-byte aligned'),
    )
    for kw, message in table:
        assert call(**kw) == LSNF_E_ARG and lib.lsnf_last_error().decode() == message, (kw, lib.lsnf_last_error())


def test_python_wrappers_have_no_cpu_path():
    F = lsnf_amd.flow
    plan = F.FlowPlan(8, 4, 2, 1, torch.zeros(1), torch.zeros(1, dtype=torch.float64))
    eps, saved, act = torch.zeros(3, 8), torch.zeros(1, 3, 8), torch.zeros(4096)
    state = F.MalaState(torch.zeros(3, 8), torch.zeros(3, 8), torch.zeros(3))
    with pytest.raises(lsnf_amd.LsnfError):
        F.reverse_mala_step(plan, eps, saved, act, None, None, state, F.PhiloxNoise(1), 0.5, init=True)
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    with pytest.raises(lsnf_amd.LsnfError):
        net.reverse_mala_step(eps, saved, act, None, None, state, F.PhiloxNoise(1), 0.5, init=True)
    with pytest.raises(lsnf_amd.LsnfError):
        lsnf_amd.langevin.sample_mala_post_eps_with_flow(eps, torch.zeros(3, 8), torch.nn.Flatten(), net, g_l_steps=2,
                                                         g_l_step_size=0.5, g_llhd_sigma=0.3, philox=F.PhiloxNoise(1))


def test_sampler_without_steps_or_rows_returns_without_a_launch(monkeypatch):
    from counting_lib import install
    F, L = lsnf_amd.flow, lsnf_amd.langevin
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    stand = install(monkeypatch, lsnf_amd)
    ph, eps = F.PhiloxNoise(5, 100), torch.randn(3, 8, 1, 1)
    none = L.sample_mala_post_eps_with_flow(eps, torch.zeros(3, 8), torch.nn.Flatten(), net, g_l_steps=0, g_l_step_size=0.5,
                                            g_llhd_sigma=0.3, philox=ph)
    assert torch.equal(none[0], eps.view(3, 8)) and none[2] is None and none[3] is None and ph.offset == 100
    empty = L.sample_mala_post_eps_with_flow(eps[:0], torch.zeros(0, 8), torch.nn.Flatten(), net, g_l_steps=4, g_l_step_size=0.5,
                                             g_llhd_sigma=0.3, philox=ph)
    assert empty[0].shape == (0, 8) and empty[1].shape == (0, 8, 1, 1) and empty[2] is None and empty[3] is None and ph.offset == 100
    assert stand.launching() == [], dict(stand.entered)


def test_cpu_tensors_are_refused_before_any_launch(monkeypatch):
    """tests/test_flow_checks_cpu.py's rule for the wrappers of flow.py, for this one of mcmc.py."""
    from counting_lib import install
    F = lsnf_amd.flow
    lib = lsnf_amd.load_library()
    plan = F.FlowPlan(8, 4, 2, 1, torch.zeros(lib.lsnf_plan_floats(8, 4, 2, 1)), torch.zeros(lib.lsnf_prepare_scratch_bytes(8, 4, 2) // 8, dtype=torch.float64))
    stand = install(monkeypatch, lsnf_amd)
    eps, v, saved = torch.zeros(5, 8), torch.zeros(5), torch.zeros(1, 5, 8)
    act = torch.zeros(lib.lsnf_act_saved_floats(8, 4, 2, 5))
    for kw in (dict(init=True), dict(uniform=v), dict(propose=False, inplace=True)):
        with pytest.raises(lsnf_amd.LsnfError):
            F.reverse_mala_step(plan, eps, saved, act, eps.clone(), v, F.new_mala_state(plan, 5, "cpu"), F.PhiloxNoise(3), 0.5, **kw)
    with pytest.raises(lsnf_amd.LsnfError):
        F.reverse_mala_step(plan, eps, saved, act, None, None, (eps, eps, v), F.PhiloxNoise(3), 0.5)      # the state is a MalaState
    assert stand.launching() == [], dict(stand.entered)


# ---- the restatement is the step it claims to be (float64, a tiny geometry) ----
def _tiny():
    nz, B = 4, 64
    p = O.init_params(nz, 3, 2, seed=5, fcz_std=0.5, dtype=torch.float64)
    g = torch.Generator().manual_seed(13)
    a, b = (torch.randn(B, nz, generator=g, dtype=torch.float64) for _ in range(2))
    return p, nz, B, a, a + 0.7 * b


def test_restated_log_alpha_is_antisymmetric():
    """log_alpha(a -> b) + log_alpha(b -> a) = 0 to 1e-9, the gradients recomputed at each end."""
    p, nz, B, a, b = _tiny()
    quad, s, u = RM.Quadratic(nz, 0.8, seed=3), 0.6, torch.full((B,), 0.5, dtype=torch.float64)
    Ua, ta, _, _, _ = RM.potential(p, a, quad, torch.float64)
    Ub, tb, _, _, _ = RM.potential(p, b, quad, torch.float64)
    ab = RM.decide(a, ta, Ua, b, tb, Ub, u, s)[0]
    ba = RM.decide(b, tb, Ub, a, ta, Ua, u, s)[0]
    assert ab.abs().max().item() > 1.0 and (ab + ba).abs().max().item() <= 1e-9
    # and it is the Metropolis-Hastings ratio of the Langevin proposal: log pi(b) q(a|b) - log pi(a) q(b|a), written out
    logq = lambda to, frm, t: -((to - frm + 0.5 * s * s * t) ** 2).sum(1) / (2.0 * s * s)
    assert ((-Ub + logq(a, b, tb)) - (-Ua + logq(b, a, ta)) - ab).abs().max().item() <= 1e-9


def test_restated_prior_alone_is_the_standard_normal():
    """energy_g = None: U is |eps|^2 / 2 and grad U = eps exactly, whatever the flow."""
    p, nz, B, a, _ = _tiny()
    U, t, e, ge, x = RM.potential(p, a, None, torch.float64)
    assert torch.equal(U, 0.5 * (a * a).sum(1)) and torch.equal(t, a) and not bool(e.any()) and not bool(ge.any())
    assert (O.flow_forward(p, x, torch.zeros(B, dtype=torch.float64))[0] - a).abs().max().item() <= 1e-9      # x = f^-1(eps)
    # with an energy the pulled-back gradient is that of e(f^-1(eps)) (central differences)
    quad = RM.Quadratic(nz, 0.8, seed=3)
    U, t, _, _, _ = RM.potential(p, a, quad, torch.float64)
    h, fd = 1e-6, torch.zeros_like(a)
    for c in range(nz):
        d = torch.zeros_like(a)
        d[:, c] = h
        fd[:, c] = (RM.potential(p, a + d, quad, torch.float64)[0] - RM.potential(p, a - d, quad, torch.float64)[0]) / (2 * h)
    assert (fd - t).abs().max().item() <= 1e-6 * max(1.0, t.abs().max().item())


def test_cost_tool_is_a_driver_on_the_ab_harness():
    """tools/rmala_step_vs_reverse_langevin_step.py: its child's source is valid and importing the driver does not import torch."""
    import subprocess
    import sys
    tools = os.path.join(ROOT, "tools")
    code = ("import sys; sys.path.insert(0, %r)\nimport ab_harness, rmala_step_vs_reverse_langevin_step as t\n"
            "compile(ab_harness.PRELUDE + t.CHILD, 'child', 'exec')\nassert 'torch' not in sys.modules\n"
            "assert t.SIZES == (100, 16384)" % tools)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=60)

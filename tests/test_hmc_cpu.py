"""CPU: Hamiltonian Monte Carlo in z without a GPU -- `lsnf_hmc_step` is declared in include/lsnf_flow_mcmc.h, exported and bound from
the extension table (outside the core ABI's symbol set), the Python layers exist and have no CPU path, the entry point validates its
arguments before any HIP call (every refusal is LSNF_E_ARG / LSNF_E_GEOMETRY, names the entry point and the offending argument in
lsnf_last_error()), and the float64 restatement the GPU tests compare with (tests/hmc_restated.py) is MALA's at L = 1, reversible,
and leaves its target invariant.  None of this holds without the feature."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from oracle import flow_oracle as O
import hmc_restated as H
import mala_restated as M

import lsnf_amd

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2
NAME = "lsnf_hmc_step"
INIT, INNER = 1, 2
FAKE = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(20)]     # 16-byte aligned addresses that are never dereferenced on the host


def test_symbol_is_declared_exported_and_bound_outside_the_core_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow_mcmc.h")).read(), flags=re.S)
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, hdr)
    assert re.search(r"#define\s+LSNF_HMC_INIT\s+1u", hdr) and re.search(r"#define\s+LSNF_HMC_INNER\s+2u", hdr)
    assert NAME not in core and hasattr(lib, NAME)
    ext = lsnf_amd._lib._EXT_SIGNATURES
    assert NAME in ext and len(ext[NAME][1]) == 27 and lsnf_amd._lib.extension_symbols() == sorted(ext)
    assert NAME not in lsnf_amd.exported_symbols() and NAME not in lsnf_amd._lib._SIGNATURES
    assert lib.lsnf_hmc_step.argtypes == ext[NAME][1]               # attached in load()
    assert lib.lsnf_abi_version() == 5 and lsnf_amd._lib.ABI_VERSION == 5
    assert (lsnf_amd.flow.HMC_INIT, lsnf_amd.flow.HMC_INNER) == (1, 2)


def test_python_layers_exist():
    F, L = lsnf_amd.flow, lsnf_amd.langevin
    sig = inspect.signature(F.hmc_step)
    assert list(sig.parameters)[:7] == ["plan", "z_prop", "grad_g", "energy_g", "state", "noise", "step_size"]
    for kw, default in (("phase", "end"), ("uniform", None), ("propose", True), ("inplace", False), ("reuse_buffers", False)):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default == default
    assert [f for f in F.HmcState.__dataclass_fields__] == ["z", "grad", "energy", "mom", "kin"] and callable(F.new_hmc_state)
    assert F.hmc_step is lsnf_amd.mcmc.hmc_step and F.HmcState is lsnf_amd.mcmc.HmcState and F.new_hmc_state is lsnf_amd.mcmc.new_hmc_state
    sig = inspect.signature(lsnf_amd._netF.hmc_step)
    assert sig.parameters["phase"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["phase"].default == "end"
    sig = inspect.signature(L.sample_hmc_post_z_with_flow)
    assert list(sig.parameters)[:4] == ["z", "x", "netG", "netF"]
    for kw in ("g_l_steps", "leapfrog_steps", "g_l_step_size", "g_llhd_sigma", "philox"):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
    # the MALA layers keep their signatures
    assert [f for f in F.MalaState.__dataclass_fields__] == ["z", "grad", "energy"]
    assert inspect.signature(F.mala_step).parameters["init"].default is False


ARGS = ("plan", "z_prop", "z_out", "saved", "act", "ll", "grad_g", "energy", "z_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")
OUTS = ("z_acc", "g_acc", "u_acc", "mom", "kin0")
WORD = {"g_acc": "grad_acc", "accept": "accept_out", "la": "log_alpha_out", "saved": "z_saved", "act": "act_saved", "ll": "ll_prop",
        "energy": "energy_g"}


def _caller(lib):
    Rng = lsnf_amd._lib.LsnfRng
    ptrs = dict(zip(ARGS + ("z_next", "accept", "la"), FAKE))
    base = dict(ptrs, nz=128, w=64, d=5, c=1, B=4, rng=None, step=0.9, flags=0, accept=None, la=None)

    def call(**kw):
        a = dict(base, **kw)
        return lib.lsnf_hmc_step(a["plan"], a["nz"], a["w"], a["d"], a["c"], a["B"], a["z_prop"], a["z_out"], a["saved"], a["act"],
                                 a["ll"], a["grad_g"], a["energy"], a["z_acc"], a["g_acc"], a["u_acc"], a["mom"], a["kin0"], a["noise"],
                                 a["uniform"], None if a["rng"] is None else ctypes.byref(a["rng"]), a["step"], a["flags"], a["z_next"],
                                 a["accept"], a["la"], None)

    def refused(word, **kw):
        err = lib.lsnf_last_error
        return call(**kw) == LSNF_E_ARG and NAME.encode() in err() and word.encode() in err()
    return call, refused, ptrs, Rng


def test_validates_before_any_hip_call():
    lib = lsnf_amd.load_library()
    call, refused, P, Rng = _caller(lib)
    inner = dict(flags=INNER, noise=None, uniform=None)
    for geo in (dict(nz=130), dict(d=17), dict(nz=7, w=4), dict(c=2), dict(w=200)):
        assert call(**geo) == LSNF_E_GEOMETRY and b"unsupported geometry" in lib.lsnf_last_error()      # (the shared rule's wording)
        assert call(B=0, **geo) == LSNF_E_GEOMETRY
    assert refused("B=-1", B=-1)
    nulls = {k: None for k in ARGS + ("z_next",)}
    assert call(B=0, **nulls) == LSNF_OK                        # empty batch: nothing to launch, NULL pointers allowed
    assert call(B=0, **dict(nulls, flags=INNER)) == LSNF_OK and call(B=0, **dict(nulls, flags=INIT)) == LSNF_OK
    # rules that precede the empty-batch return: the same answer for B = 0
    tensors = dict(noise=None, uniform=None)
    for B in (0, 4):
        assert refused("not both", B=B, uniform=None, rng=Rng(1, 0, None, 0)) and b"noise" in lib.lsnf_last_error()
        assert refused("not both", B=B, noise=None, rng=Rng(1, 0, None, 0)) and b"uniform" in lib.lsnf_last_error()
        assert refused("row0", B=B, rng=Rng(1, 0, None, -1), **tensors)
        assert refused("offset_dev", B=B, rng=Rng(1, 0, 0x30004, 0), **tensors)
        for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -0.0):
            assert refused("step_size", B=B, step=bad) and refused("step_size", B=B, step=bad, **inner)
        for bad in (4, 5, 8, 0x80000000, 0x80000002):
            assert refused("unknown flag", B=B, flags=bad)
        assert refused("exclude each other", B=B, flags=INIT | INNER, **tensors)
        # an inner call draws and decides nothing
        assert refused("noise is not taken", B=B, flags=INNER, uniform=None)
        assert refused("uniform is not taken", B=B, flags=INNER, noise=None)
        assert refused("rng is not taken", B=B, rng=Rng(1, 0, None, 0), **inner)
        assert refused("accept_out must be NULL", B=B, accept=P["accept"], **inner)
        assert refused("log_alpha_out must be NULL", B=B, la=P["la"], **inner)
        # aliases: no output may be a tensor the call reads, or another output; the message names both
        for out in OUTS + ("z_next", "accept", "la"):
            wording = WORD.get(out, out)
            for src in ARGS:
                if src in OUTS or (out, src) == ("z_next", "z_prop"):
                    continue
                assert refused("alias", B=B, **{out: P[src]}) and wording.encode() in lib.lsnf_last_error()
            for other in OUTS + ("z_next",):
                if other != out:
                    assert refused("alias", B=B, **{out: P[other]}) and wording.encode() in lib.lsnf_last_error()
        assert refused("alias", B=B, accept=P["la"], la=P["la"])
        assert refused("alias", B=B, z_next=P["mom"], **inner) and refused("alias", B=B, mom=P["grad_g"], **inner)
    # the allowed alias: the next point over the point
    assert call(B=0, z_next=P["z_prop"]) == LSNF_OK and call(B=0, z_next=P["z_prop"], **inner) == LSNF_OK
    assert call(B=0, z_next=P["z_prop"], accept=P["accept"], la=P["la"]) == LSNF_OK
    # required pointers, each named, in every phase
    for arg in ("plan", "z_prop", "z_out", "act", "z_acc", "g_acc", "u_acc", "mom", "kin0", "saved"):
        for extra in (dict(), inner, dict(flags=INIT)):
            assert refused(WORD.get(arg, arg), **dict(extra, **{arg: None})) and b"NULL" in lib.lsnf_last_error()
    assert refused("ll_prop", ll=None) and refused("ll_prop", ll=None, flags=INIT)
    assert refused("z_next", z_next=None, **inner) and b"NULL" in lib.lsnf_last_error()
    # without an rng: the uniform unless INIT, the noise iff a new trajectory is asked for
    assert refused("uniform", uniform=None)
    assert refused("noise", noise=None) and refused("noise", noise=None, flags=INIT)
    assert refused("noise", z_next=None) and refused("noise", z_next=None, flags=INIT)
    # alignment: 16 bytes for plan and act_saved, 4 bytes for every tensor, each named
    assert refused("plan must be 16-byte", plan=ctypes.c_void_p(0x10004))
    assert refused("act_saved must be 16-byte", act=ctypes.c_void_p(0x50008)) and refused("act_saved must be 16-byte", act=ctypes.c_void_p(0x50008), **inner)
    for arg in ("z_prop", "z_out", "saved", "ll", "grad_g", "energy", "z_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform", "z_next",
                "accept", "la"):
        assert refused(WORD.get(arg, arg) + " must be 4-byte", **{arg: ctypes.c_void_p(0xF00002)})
    for arg in ("mom", "kin0", "z_next", "grad_g"):
        assert refused(WORD.get(arg, arg) + " must be 4-byte", **dict(inner, **{arg: ctypes.c_void_p(0xF00002)}))


def test_depth_one_and_the_optional_pointers_pass_the_pointer_rules():
    lib = lsnf_amd.load_library()
    call, refused, P, Rng = _caller(lib)
    # (the next rule -- a misaligned act_saved here -- is what refuses these calls, still before any HIP call)
    bad_act = ctypes.c_void_p(0x50008)
    assert refused("act_saved must be 16-byte", nz=64, w=32, d=1, saved=None, act=bad_act)           # depth 1: no block outputs
    assert refused("act_saved must be 16-byte", flags=INIT, uniform=None, act=bad_act)               # INIT: no uniform
    assert refused("act_saved must be 16-byte", noise=None, z_next=None, act=bad_act)                # deciding only: no noise
    assert refused("act_saved must be 16-byte", noise=None, uniform=None, rng=Rng(1, 0, None, 0), act=bad_act)
    assert refused("act_saved must be 16-byte", grad_g=None, energy=None, act=bad_act)               # the prior alone
    # an inner call: ll_prop and energy_g may be NULL (they are never read)
    assert refused("act_saved must be 16-byte", flags=INNER, noise=None, uniform=None, ll=None, energy=None, act=bad_act)
    assert refused("act_saved must be 16-byte", flags=INNER, noise=None, uniform=None, nz=64, w=32, d=1, saved=None, act=bad_act)


def test_every_rule_speaks_word_for_word():
    """One call per rule and phase it applies in: the first violated rule speaks, and lsnf_last_error() is this text to the letter."""
    lib = lsnf_amd.load_library()
    call, _, P, Rng = _caller(lib)
    inner = dict(flags=INNER, noise=None, uniform=None)
    table = (
        (dict(B=-1), 'lsnf_hmc_step: B=-1 out of range'),
        (dict(B=0, noise=None, rng=Rng(1, 0, None, 0)), 'lsnf_hmc_step: pass either a uniform tensor or an rng, not both'),
        (dict(uniform=None, rng=Rng(1, 0, None, 0)), 'lsnf_hmc_step: pass either a noise tensor or an rng, not both'),
        (dict(B=0, noise=None, uniform=None, rng=Rng(1, 0, None, -1)), 'lsnf_hmc_step: rng->row0 must be >= 0'),
        (dict(noise=None, uniform=None, rng=Rng(1, 0, 0x30004, 0)), 'lsnf_hmc_step: rng->offset_dev must be 8-byte aligned'),
        (dict(step=float('nan')), 'lsnf_hmc_step: step_size must be finite and non-zero (got nan)'),
        (dict(B=0, step=0.0), 'lsnf_hmc_step: step_size must be finite and non-zero (got 0)'),
        (dict(inner, step=0.0), 'lsnf_hmc_step: step_size must be finite and non-zero (got 0)'),
        (dict(flags=4), 'lsnf_hmc_step: unknown flag bits 0x4'),
        (dict(B=0, flags=0x80000003), 'lsnf_hmc_step: unknown flag bits 0x80000000'),
        (dict(flags=INIT | INNER, noise=None, uniform=None), 'lsnf_hmc_step: flags: LSNF_HMC_INIT and LSNF_HMC_INNER exclude each other'),
        (dict(B=0, flags=INIT | INNER), 'lsnf_hmc_step: flags: LSNF_HMC_INIT and LSNF_HMC_INNER exclude each other'),
        (dict(flags=INNER, uniform=None), 'lsnf_hmc_step: noise is not taken with LSNF_HMC_INNER (an inner step draws nothing)'),
        (dict(B=0, flags=INNER, noise=None), 'lsnf_hmc_step: uniform is not taken with LSNF_HMC_INNER (an inner step draws nothing)'),
        (dict(inner, rng=Rng(1, 0, None, 0)), 'lsnf_hmc_step: rng is not taken with LSNF_HMC_INNER (an inner step draws nothing)'),
        (dict(inner, accept=P['accept']), 'lsnf_hmc_step: accept_out must be NULL with LSNF_HMC_INNER (an inner step decides nothing)'),
        (dict(inner, B=0, la=P['la']), 'lsnf_hmc_step: log_alpha_out must be NULL with LSNF_HMC_INNER (an inner step decides nothing)'),
        (dict(z_acc=P['grad_g']), 'lsnf_hmc_step: z_acc must not alias grad_g'),
        (dict(B=0, z_next=P['z_out'], flags=INIT), 'lsnf_hmc_step: z_next must not alias z_out'),
        (dict(kin0=P['uniform']), 'lsnf_hmc_step: kin0 must not alias uniform'),
        (dict(mom=P['z_next']), 'lsnf_hmc_step: z_next must not alias mom'),
        (dict(inner, mom=P['grad_g']), 'lsnf_hmc_step: mom must not alias grad_g'),
        (dict(inner, z_next=P['mom']), 'lsnf_hmc_step: z_next must not alias mom'),
        (dict(accept=P['la'], la=P['la']), 'lsnf_hmc_step: accept_out must not alias log_alpha_out'),
        (dict(plan=None), 'lsnf_hmc_step: plan is required (NULL)'),
        (dict(mom=None, flags=INIT), 'lsnf_hmc_step: mom is required (NULL)'),
        (dict(inner, kin0=None), 'lsnf_hmc_step: kin0 is required (NULL)'),
        (dict(ll=None), 'lsnf_hmc_step: ll_prop is required (NULL) unless LSNF_HMC_INNER'),
        (dict(ll=None, flags=INIT), 'lsnf_hmc_step: ll_prop is required (NULL) unless LSNF_HMC_INNER'),
        (dict(ll=None, saved=None), 'lsnf_hmc_step: ll_prop is required (NULL) unless LSNF_HMC_INNER'),
        (dict(saved=None), 'lsnf_hmc_step: z_saved is required (NULL) for depth > 1'),
        (dict(inner, saved=None, z_next=None), 'lsnf_hmc_step: z_saved is required (NULL) for depth > 1'),
        (dict(inner, z_next=None), 'lsnf_hmc_step: z_next is required (NULL) with LSNF_HMC_INNER'),
        (dict(uniform=None), 'lsnf_hmc_step: uniform is required without an rng (unless LSNF_HMC_INIT or LSNF_HMC_INNER)'),
        (dict(noise=None), 'lsnf_hmc_step: noise is required with z_next when no rng is given'),
        (dict(noise=None, flags=INIT, uniform=None), 'lsnf_hmc_step: noise is required with z_next when no rng is given'),
        (dict(z_next=None), 'lsnf_hmc_step: noise goes with z_next: nothing is proposed without it'),
        (dict(z_next=None, flags=INIT), 'lsnf_hmc_step: noise goes with z_next: nothing is proposed without it'),
        (dict(plan=ctypes.c_void_p(0x10004)), 'lsnf_hmc_step: plan must be 16-byte aligned'),
        (dict(inner, act=ctypes.c_void_p(0x50008), ll=None, energy=None), 'lsnf_hmc_step: act_saved must be 16-byte aligned'),
        (dict(inner, mom=ctypes.c_void_p(0xF00002)), 'lsnf_hmc_step: mom must be 4-byte aligned'),
        (dict(grad_g=ctypes.c_void_p(0xF00002)), 'lsnf_hmc_step: grad_g must be 4-byte aligned'),
        (dict(la=ctypes.c_void_p(0xF00002)), 'lsnf_hmc_step: log_alpha_out must be 4-byte aligned'),
    )
    for kw, message in table:
        assert call(**kw) == LSNF_E_ARG and lib.lsnf_last_error().decode() == message, (kw, lib.lsnf_last_error())


def test_python_wrappers_have_no_cpu_path():
    F = lsnf_amd.flow
    plan = F.FlowPlan(8, 4, 2, 1, torch.zeros(1), torch.zeros(1, dtype=torch.float64))
    z = torch.zeros(3, 8)
    state = F.HmcState(torch.zeros(3, 8), torch.zeros(3, 8), torch.zeros(3), torch.zeros(3, 8), torch.zeros(3))
    with pytest.raises(lsnf_amd.LsnfError):
        F.hmc_step(plan, z, None, None, state, F.PhiloxNoise(1), 0.5, phase="init")
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    with pytest.raises(lsnf_amd.LsnfError):
        net.hmc_step(z, None, None, state, F.PhiloxNoise(1), 0.5, phase="init")
    kw = dict(g_l_step_size=0.5, g_llhd_sigma=0.3, philox=F.PhiloxNoise(1))
    with pytest.raises(lsnf_amd.LsnfError):
        lsnf_amd.langevin.sample_hmc_post_z_with_flow(z.view(3, 8, 1, 1), torch.zeros(3, 8), torch.nn.Flatten(), net, g_l_steps=2,
                                                      leapfrog_steps=2, **kw)
    with pytest.raises(ValueError):
        lsnf_amd.langevin.sample_hmc_post_z_with_flow(z.view(3, 8, 1, 1), torch.zeros(3, 8), torch.nn.Flatten(), net, g_l_steps=2,
                                                      leapfrog_steps=0, **kw)
    ph = F.PhiloxNoise(1, 9)
    none = lsnf_amd.langevin.sample_hmc_post_z_with_flow(z.view(3, 8, 1, 1), torch.zeros(3, 8), torch.nn.Flatten(), net, g_l_steps=0,
                                                         leapfrog_steps=2, g_l_step_size=0.5, g_llhd_sigma=0.3, philox=ph)
    assert torch.equal(none[0], z.view(3, 8, 1, 1)) and none[1] is None and none[2] is None and ph.offset == 9


def test_cpu_tensors_are_refused_before_any_launch(monkeypatch):
    """tests/test_flow_checks_cpu.py's rule for the wrappers of flow.py, for `hmc_step` of mcmc.py (re-exported as flow.hmc_step)."""
    from counting_lib import install
    F = lsnf_amd.flow
    lib = lsnf_amd.load_library()
    plan = F.FlowPlan(8, 4, 2, 1, torch.zeros(lib.lsnf_plan_floats(8, 4, 2, 1)), torch.zeros(lib.lsnf_prepare_scratch_bytes(8, 4, 2) // 8, dtype=torch.float64))
    stand = install(monkeypatch, lsnf_amd)
    z, v = torch.zeros(5, 8), torch.zeros(5)
    for kw in (dict(phase="init"), dict(uniform=v), dict(propose=False, inplace=True)):
        with pytest.raises(lsnf_amd.LsnfError):
            F.hmc_step(plan, z, z.clone(), v, F.new_hmc_state(plan, 5, "cpu"), F.PhiloxNoise(3), 0.5, **kw)
    with pytest.raises(lsnf_amd.LsnfError):
        F.hmc_step(plan, z, z.clone(), v, F.new_hmc_state(plan, 5, "cpu"), None, 0.5, phase="inner")
    with pytest.raises(lsnf_amd.LsnfError):
        F.hmc_step(plan, z, None, None, F.new_mala_state(plan, 5, "cpu"), F.PhiloxNoise(3), 0.5)      # the state is an HmcState
    with pytest.raises(lsnf_amd.LsnfError):
        F.hmc_step(plan, z, None, None, F.new_hmc_state(plan, 5, "cpu"), F.PhiloxNoise(3), 0.5, phase="middle")
    assert stand.launching() == [], dict(stand.entered)


# ---- the float64 restatement -----------------------------------------------------------------------------------------------
def _setup(nz=8, w=4, depth=3, B=64, seed=5):
    p = O.init_params(nz, w, depth, seed=seed, dtype=torch.float64)
    g = torch.Generator().manual_seed(17)
    z0 = torch.randn(B, nz, generator=g, dtype=torch.float64)
    return p, g, z0, M.Quadratic(nz, 0.3, seed=9)


def test_one_leapfrog_step_is_the_mala_decision():
    """L = 1: log_alpha equals mala_restated.decide's on the same state, proposal and uniform (kinL = A / (2 s^2), kin0 = Bq / (2 s^2))."""
    p, g, z0, quad = _setup()
    s, B, nz = 0.7, z0.shape[0], z0.shape[1]
    noises = [torch.randn(B, nz, generator=g, dtype=torch.float64) for _ in range(3)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g, dtype=torch.float64).clamp_min(1e-300) for _ in range(3)]
    calls, _ = H.chain(p, z0, quad, s, 1, noises, uniforms)
    steps, _ = M.chain(p, z0, quad, s, noises, uniforms)
    assert [c.phase for c in calls] == ["init", "end", "end", "end"] and len(steps) == 3
    for c, st in zip(calls[1:], steps):
        assert torch.allclose(c.z_prop, st.z_prop, rtol=0, atol=1e-12)                       # the leapfrog proposal is MALA's
        la = M.decide(c.z_acc, c.g_acc, c.u_acc, c.z_prop, c.g, c.U_prop, c.u, s)[0]
        assert float((c.la - la).abs().max()) <= 1e-12
        assert torch.equal(c.acc, st.acc)
    assert 0 < sum(int(c.acc.sum()) for c in calls[1:]) < 3 * B


@pytest.mark.parametrize("L", [1, 3, 5])
def test_a_trajectory_is_reversible(L):
    """L steps, the momentum negated, L steps: back at the start to 1e-10, and the second log_alpha is minus the first."""
    p, g, z0, quad = _setup()
    s, B, nz = 0.4, z0.shape[0], z0.shape[1]
    xi = torch.randn(B, nz, generator=g, dtype=torch.float64)
    u = torch.full((B,), 0.5, dtype=torch.float64)
    calls, _ = H.chain(p, z0, quad, s, L, [xi, None], [None, u])
    last = calls[-1]
    assert last.phase == "end" and len(calls) == L + 1
    back, _ = H.chain(p, last.z_prop, quad, s, L, [-last.pL, None], [None, u])
    assert float((back[-1].z_prop - z0).abs().max()) <= 1e-10
    assert float((back[-1].pL + xi).abs().max()) <= 1e-10
    assert float((back[-1].la + last.la).abs().max()) <= 1e-10 and float(last.la.abs().max()) > 1e-3


def test_restated_chain_leaves_its_target_invariant():
    """20 000 float64 rows started from exact prior samples, K = 4 trajectories of L = 3 steps, the prior alone: the mean of ll must
    not drift beyond 4 standard errors (the standard error of a difference of two means, without credit for their correlation); the
    same trajectories without the accept step do (tests/test_mala_cpu.py's rule)."""
    nz, B, K, L, s = 2, 20000, 4, 3, 0.9
    p = O.init_params(nz, 4, 1, seed=5, fcz_std=0.5, dtype=torch.float64)
    g = torch.Generator().manual_seed(11)
    z0 = O.flow_reverse(p, torch.randn(B, nz, generator=g, dtype=torch.float64), torch.zeros(B, dtype=torch.float64))[0]
    noises = [torch.randn(B, nz, generator=g, dtype=torch.float64) for _ in range(K)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g, dtype=torch.float64).clamp_min(1e-300) for _ in range(K)]
    calls, (zk, _, uk) = H.chain(p, z0, None, s, L, noises, uniforms)
    assert len(calls) == K * L + 1
    ll0, llk = O.flow_log_prob(p, z0)[2], -uk
    assert torch.allclose(llk, O.flow_log_prob(p, zk)[2], rtol=0, atol=1e-12)               # the kept energy is U of the kept point
    rate = torch.stack([c.acc for c in calls if c.phase == "end"]).double().mean().item()
    se = float(torch.sqrt(ll0.var() / B + llk.var() / B))
    drift = abs(float(llk.mean() - ll0.mean()))
    print(f"[hmc] invariance: acceptance {rate:.3f}, mean ll {ll0.mean():.5f} -> {llk.mean():.5f}, drift {drift:.2e}, 4 SE {4 * se:.2e}")
    assert 0.15 < rate < 0.98 and drift <= 4.0 * se
    # the same trajectories without the correction do drift: the check above is not vacuous
    z = z0
    for n in noises[:-1]:
        z = H.trajectory(p, None, z, M.potential(p, z, None, torch.float64)[1], n, s, L).z[L]
    raw = abs(float(O.flow_log_prob(p, z)[2].mean() - ll0.mean()))
    print(f"[hmc] unadjusted drift {raw:.2e}")
    assert raw > 4.0 * se


def test_cost_tool_is_a_driver_on_the_ab_harness():
    """tools/hmc_step_vs_mala_step.py: its child's source is valid and importing the driver does not import torch."""
    import subprocess
    import sys
    tools = os.path.join(ROOT, "tools")
    code = ("import sys; sys.path.insert(0, %r)\nimport ab_harness, hmc_step_vs_mala_step as t\n"
            "compile(ab_harness.PRELUDE + t.CHILD, 'child', 'exec')\nassert 'torch' not in sys.modules\n"
            "assert t.SIZES == (100, 16384)" % tools)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=60)

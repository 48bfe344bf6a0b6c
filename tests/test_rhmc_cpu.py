"""CPU: Hamiltonian Monte Carlo in the flow's base space without a GPU -- `lsnf_reverse_hmc_step` is declared in
include/lsnf_flow_mcmc.h, exported and bound from the extension table (outside the core ABI's symbol set), the Python layers exist
and have no CPU path, the entry point validates its arguments before any HIP call (every refusal is LSNF_E_ARG / LSNF_E_GEOMETRY,
names the entry point and the offending argument in lsnf_last_error()), and the float64 restatement the GPU tests compare with
(tests/rhmc_restated.py) is base-space MALA's at L = 1, reversible, and leaves N(0, I) invariant.  The symbol, wrapper and refusal
tests do not hold without the feature; the restatement's property tests exercise tests/rhmc_restated.py alone and hold wherever that
file is present."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from oracle import flow_oracle as O
import rhmc_restated as RH
import rmala_restated as RM

import lsnf_amd

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2
NAME = "lsnf_reverse_hmc_step"
INIT, INNER = 1, 2
FAKE = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(20)]     # 16-byte aligned addresses that are never dereferenced on the host


def test_symbol_is_declared_exported_and_bound_outside_the_core_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow_mcmc.h")).read(), flags=re.S)
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, hdr)
    assert len(re.findall(r"#define\s+LSNF_HMC_INIT\s+1u", hdr)) == 1 and len(re.findall(r"#define\s+LSNF_HMC_INNER\s+2u", hdr)) == 1
    assert NAME not in core and hasattr(lib, NAME)
    ext = lsnf_amd._lib._EXT_SIGNATURES
    assert NAME in ext and len(ext[NAME][1]) == 25 and lsnf_amd._lib.extension_symbols() == sorted(ext)
    assert NAME not in lsnf_amd.exported_symbols() and NAME not in lsnf_amd._lib._SIGNATURES
    assert lib.lsnf_reverse_hmc_step.argtypes == ext[NAME][1]       # attached in load()
    assert lib.lsnf_abi_version() == 5 and lsnf_amd._lib.ABI_VERSION == 5
    # the declaration's 25 parameters: lsnf_reverse_mala_step's, plus mom and kin0 after u_acc
    decl = lambda name: [re.sub(r".*[\s*]", "", a.strip())
                         for a in re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1).split(",")]
    names, rmala = decl(NAME), decl("lsnf_reverse_mala_step")
    at = rmala.index("u_acc") + 1
    assert len(names) == 25 and names == rmala[:at] + ["mom", "kin0"] + rmala[at:]


def test_python_layers_exist():
    F, L = lsnf_amd.flow, lsnf_amd.langevin
    assert F.reverse_hmc_step is lsnf_amd.mcmc.reverse_hmc_step
    sig = inspect.signature(F.reverse_hmc_step)
    assert list(sig.parameters)[:9] == ["plan", "eps_prop", "z_saved", "act_saved", "grad_g", "energy_g", "state", "noise", "step_size"]
    for kw, default in (("phase", "end"), ("uniform", None), ("propose", True), ("inplace", False), ("reuse_buffers", False)):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[kw].default == default
    assert [f for f in F.HmcState.__dataclass_fields__] == ["z", "grad", "energy", "mom", "kin"] and "eps" in F.HmcState.__doc__
    sig = inspect.signature(lsnf_amd._netF.reverse_hmc_step)
    assert list(sig.parameters)[:4] == ["self", "eps_prop", "z_saved", "act_saved"]
    assert sig.parameters["phase"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["phase"].default == "end"
    sig = inspect.signature(L.sample_hmc_post_eps_with_flow)
    assert list(sig.parameters) == ["eps", "x", "netG", "netF", "g_l_steps", "leapfrog_steps", "g_l_step_size", "g_llhd_sigma", "philox"]
    for kw in ("g_l_steps", "leapfrog_steps", "g_l_step_size", "g_llhd_sigma", "philox"):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
    # the existing layers keep their signatures
    assert list(inspect.signature(F.hmc_step).parameters)[:7] == ["plan", "z_prop", "grad_g", "energy_g", "state", "noise", "step_size"]
    assert inspect.signature(F.reverse_mala_step).parameters["init"].default is False


ARGS = ("plan", "eps_prop", "saved", "act", "grad_g", "energy", "eps_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")
OUTS = ("eps_acc", "g_acc", "u_acc", "mom", "kin0")
WORD = {"g_acc": "grad_acc", "accept": "accept_out", "la": "log_alpha_out", "saved": "z_saved", "act": "act_saved", "energy": "energy_g"}


def _caller(lib):
    Rng = lsnf_amd._lib.LsnfRng
    ptrs = dict(zip(ARGS + ("eps_next", "accept", "la"), FAKE))
    base = dict(ptrs, nz=128, w=64, d=5, c=1, B=4, rng=None, step=0.9, flags=0, accept=None, la=None)

    def call(**kw):
        a = dict(base, **kw)
        return lib.lsnf_reverse_hmc_step(a["plan"], a["nz"], a["w"], a["d"], a["c"], a["B"], a["eps_prop"], a["saved"], a["act"],
                                         a["grad_g"], a["energy"], a["eps_acc"], a["g_acc"], a["u_acc"], a["mom"], a["kin0"], a["noise"],
                                         a["uniform"], None if a["rng"] is None else ctypes.byref(a["rng"]), a["step"], a["flags"],
                                         a["eps_next"], a["accept"], a["la"], None)

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
    nulls = {k: None for k in ARGS + ("eps_next",)}
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
        for out in OUTS + ("eps_next", "accept", "la"):
            wording = WORD.get(out, out)
            for src in ARGS:
                if src in OUTS or (out, src) == ("eps_next", "eps_prop"):
                    continue
                assert refused("alias", B=B, **{out: P[src]}) and wording.encode() in lib.lsnf_last_error()
                assert WORD.get(src, src).encode() in lib.lsnf_last_error()
            for other in OUTS + ("eps_next",):
                if other != out:
                    assert refused("alias", B=B, **{out: P[other]}) and wording.encode() in lib.lsnf_last_error()
        assert refused("alias", B=B, accept=P["la"], la=P["la"])
        assert refused("alias", B=B, eps_next=P["mom"], **inner) and refused("alias", B=B, mom=P["grad_g"], **inner)
    # the allowed alias: the next point over the point
    assert call(B=0, eps_next=P["eps_prop"]) == LSNF_OK and call(B=0, eps_next=P["eps_prop"], **inner) == LSNF_OK
    assert call(B=0, eps_next=P["eps_prop"], accept=P["accept"], la=P["la"]) == LSNF_OK
    # required pointers, each named, in every phase
    for arg in ("plan", "eps_prop", "act", "eps_acc", "g_acc", "u_acc", "mom", "kin0", "saved"):
        for extra in (dict(), inner, dict(flags=INIT)):
            assert refused(WORD.get(arg, arg), **dict(extra, **{arg: None})) and b"required" in lib.lsnf_last_error()
    assert refused("eps_next", eps_next=None, **inner) and b"NULL" in lib.lsnf_last_error()
    # without an rng: the uniform unless INIT, the noise iff a new trajectory is asked for
    assert refused("uniform", uniform=None)
    assert refused("noise", noise=None) and refused("noise", noise=None, flags=INIT)
    assert refused("noise", eps_next=None) and refused("noise", eps_next=None, flags=INIT)
    # alignment: 16 bytes for plan and act_saved, 4 bytes for every tensor, each named
    assert refused("plan must be 16-byte", plan=ctypes.c_void_p(0x10004))
    assert refused("act_saved must be 16-byte", act=ctypes.c_void_p(0x50008)) and refused("act_saved must be 16-byte", act=ctypes.c_void_p(0x50008), **inner)
    for arg in ("eps_prop", "saved", "grad_g", "energy", "eps_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform", "eps_next", "accept", "la"):
        assert refused(WORD.get(arg, arg) + " must be 4-byte", **{arg: ctypes.c_void_p(0xF00002)})
    for arg in ("mom", "kin0", "eps_next", "grad_g"):
        assert refused(WORD.get(arg, arg) + " must be 4-byte", **dict(inner, **{arg: ctypes.c_void_p(0xF00002)}))


def test_depth_one_and_the_optional_pointers_pass_the_pointer_rules():
    lib = lsnf_amd.load_library()
    call, refused, P, Rng = _caller(lib)
    # (the next rule -- a misaligned act_saved here -- is what refuses these calls, still before any HIP call)
    bad_act = ctypes.c_void_p(0x50008)
    assert refused("act_saved must be 16-byte", nz=64, w=32, d=1, saved=None, act=bad_act)           # depth 1: no block outputs
    assert refused("act_saved must be 16-byte", flags=INIT, uniform=None, act=bad_act)               # INIT: no uniform
    assert refused("act_saved must be 16-byte", flags=INIT, noise=None, uniform=None, eps_next=None, act=bad_act)      # INIT: the state alone
    assert refused("act_saved must be 16-byte", noise=None, eps_next=None, act=bad_act)              # deciding only: no noise
    assert refused("act_saved must be 16-byte", noise=None, uniform=None, rng=Rng(1, 0, None, 0), act=bad_act)
    assert refused("act_saved must be 16-byte", grad_g=None, energy=None, act=bad_act)               # the prior alone
    # an inner call: energy_g may be NULL (it is never read)
    assert refused("act_saved must be 16-byte", flags=INNER, noise=None, uniform=None, energy=None, act=bad_act)
    assert refused("act_saved must be 16-byte", flags=INNER, noise=None, uniform=None, nz=64, w=32, d=1, saved=None, act=bad_act)


def test_every_rule_speaks_word_for_word():
    """One call per rule and phase it applies in: the first violated rule speaks, and lsnf_last_error() is this text to the letter
    (tests/test_hmc_cpu.py's table of messages under this entry's names)."""
    lib = lsnf_amd.load_library()
    call, _, P, Rng = _caller(lib)
    inner = dict(flags=INNER, noise=None, uniform=None)
    N = NAME
    stash = N + ': act_saved is required (the stash of lsnf_forward, lsnf_restash or lsnf_reverse_keep)'
    table = (
        (dict(B=-1), N + ': B=-1 out of range'),
        (dict(B=0, noise=None, rng=Rng(1, 0, None, 0)), N + ': pass either a uniform tensor or an rng, not both'),
        (dict(uniform=None, rng=Rng(1, 0, None, 0)), N + ': pass either a noise tensor or an rng, not both'),
        (dict(B=0, noise=None, uniform=None, rng=Rng(1, 0, None, -1)), N + ': rng->row0 must be >= 0'),
        (dict(noise=None, uniform=None, rng=Rng(1, 0, 0x30004, 0)), N + ': rng->offset_dev must be 8-byte aligned'),
        (dict(step=float('nan')), N + ': step_size must be finite and non-zero (got nan)'),
        (dict(B=0, step=0.0), N + ': step_size must be finite and non-zero (got 0)'),
        (dict(inner, step=0.0), N + ': step_size must be finite and non-zero (got 0)'),
        (dict(flags=4), N + ': unknown flag bits 0x4'),
        (dict(B=0, flags=0x80000003), N + ': unknown flag bits 0x80000000'),
        (dict(flags=INIT | INNER, noise=None, uniform=None), N + ': flags: LSNF_HMC_INIT and LSNF_HMC_INNER exclude each other'),
        (dict(B=0, flags=INIT | INNER), N + ': flags: LSNF_HMC_INIT and LSNF_HMC_INNER exclude each other'),
        (dict(flags=INNER, uniform=None), N + ': noise is not taken with LSNF_HMC_INNER (an inner step draws nothing)'),
        (dict(B=0, flags=INNER, noise=None), N + ': uniform is not taken with LSNF_HMC_INNER (an inner step draws nothing)'),
        (dict(inner, rng=Rng(1, 0, None, 0)), N + ': rng is not taken with LSNF_HMC_INNER (an inner step draws nothing)'),
        (dict(inner, accept=P['accept']), N + ': accept_out must be NULL with LSNF_HMC_INNER (an inner step decides nothing)'),
        (dict(inner, B=0, la=P['la']), N + ': log_alpha_out must be NULL with LSNF_HMC_INNER (an inner step decides nothing)'),
        (dict(eps_acc=P['grad_g']), N + ': eps_acc must not alias grad_g'),
        (dict(B=0, eps_next=P['saved'], flags=INIT), N + ': eps_next must not alias z_saved'),
        (dict(kin0=P['uniform']), N + ': kin0 must not alias uniform'),
        (dict(mom=P['eps_next']), N + ': eps_next must not alias mom'),
        (dict(inner, mom=P['grad_g']), N + ': mom must not alias grad_g'),
        (dict(inner, eps_next=P['mom']), N + ': eps_next must not alias mom'),
        (dict(B=0, mom=P['eps_prop']), N + ': mom must not alias eps_prop'),
        (dict(accept=P['la'], la=P['la']), N + ': accept_out must not alias log_alpha_out'),
        (dict(plan=None), N + ': plan is required (NULL)'),
        (dict(eps_prop=None), N + ': eps_prop is required (NULL)'),
        (dict(mom=None, flags=INIT), N + ': mom is required (NULL)'),
        (dict(inner, kin0=None), N + ': kin0 is required (NULL)'),
        (dict(act=None), stash),
        (dict(inner, act=None, saved=None), stash),
        (dict(saved=None), N + ': z_saved is required (NULL) for depth > 1'),
        (dict(inner, saved=None, eps_next=None), N + ': z_saved is required (NULL) for depth > 1'),
        (dict(inner, eps_next=None), N + ': eps_next is required (NULL) with LSNF_HMC_INNER'),
        (dict(uniform=None), N + ': uniform is required without an rng (unless LSNF_HMC_INIT or LSNF_HMC_INNER)'),
        (dict(noise=None), N + ': noise is required with eps_next when no rng is given'),
        (dict(noise=None, flags=INIT, uniform=None), N + ': noise is required with eps_next when no rng is given'),
        (dict(eps_next=None), N + ': noise goes with eps_next: nothing is proposed without it'),
        (dict(eps_next=None, flags=INIT), N + ': noise goes with eps_next: nothing is proposed without it'),
        (dict(plan=ctypes.c_void_p(0x10004)), N + ': plan must be 16-byte aligned'),
        (dict(inner, act=ctypes.c_void_p(0x50008), energy=None), N + ': act_saved must be 16-byte aligned'),
        (dict(inner, mom=ctypes.c_void_p(0xF00002)), N + ': mom must be 4-byte aligned'),
        (dict(grad_g=ctypes.c_void_p(0xF00002)), N + ': grad_g must be 4-byte aligned'),
        (dict(la=ctypes.c_void_p(0xF00002)), N + ': log_alpha_out must be 4-byte aligned'),
    )
    for kw, message in table:
        assert call(**kw) == LSNF_E_ARG and lib.lsnf_last_error().decode() == message, (kw, lib.lsnf_last_error())


def test_python_wrappers_have_no_cpu_path():
    F = lsnf_amd.flow
    plan = F.FlowPlan(8, 4, 2, 1, torch.zeros(1), torch.zeros(1, dtype=torch.float64))
    eps, saved, act = torch.zeros(3, 8), torch.zeros(1, 3, 8), torch.zeros(4096)
    state = F.HmcState(torch.zeros(3, 8), torch.zeros(3, 8), torch.zeros(3), torch.zeros(3, 8), torch.zeros(3))
    with pytest.raises(lsnf_amd.LsnfError):
        F.reverse_hmc_step(plan, eps, saved, act, None, None, state, F.PhiloxNoise(1), 0.5, phase="init")
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    with pytest.raises(lsnf_amd.LsnfError):
        net.reverse_hmc_step(eps, saved, act, None, None, state, F.PhiloxNoise(1), 0.5, phase="init")
    kw = dict(g_l_step_size=0.5, g_llhd_sigma=0.3, philox=F.PhiloxNoise(1))
    with pytest.raises(lsnf_amd.LsnfError):
        lsnf_amd.langevin.sample_hmc_post_eps_with_flow(eps, torch.zeros(3, 8), torch.nn.Flatten(), net, g_l_steps=2, leapfrog_steps=2, **kw)
    with pytest.raises(ValueError):
        lsnf_amd.langevin.sample_hmc_post_eps_with_flow(eps, torch.zeros(3, 8), torch.nn.Flatten(), net, g_l_steps=2, leapfrog_steps=0, **kw)


def test_sampler_without_steps_or_rows_returns_without_a_launch(monkeypatch):
    from counting_lib import install
    F, L = lsnf_amd.flow, lsnf_amd.langevin
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    stand = install(monkeypatch, lsnf_amd)
    ph, eps = F.PhiloxNoise(5, 100), torch.randn(3, 8, 1, 1)
    kw = dict(leapfrog_steps=3, g_l_step_size=0.5, g_llhd_sigma=0.3, philox=ph)
    none = L.sample_hmc_post_eps_with_flow(eps, torch.zeros(3, 8), torch.nn.Flatten(), net, g_l_steps=0, **kw)
    assert torch.equal(none[0], eps.view(3, 8)) and none[1] is None and none[2] is None and none[3] is None and ph.offset == 100
    empty = L.sample_hmc_post_eps_with_flow(eps[:0], torch.zeros(0, 8), torch.nn.Flatten(), net, g_l_steps=4, **kw)
    assert empty[0].shape == (0, 8) and empty[1].shape == (0, 8, 1, 1) and empty[2] is None and empty[3] is None and ph.offset == 100
    assert stand.launching() == [], dict(stand.entered)


def test_cpu_tensors_are_refused_before_any_launch(monkeypatch):
    """tests/test_flow_checks_cpu.py's rule for the wrappers of flow.py, for `reverse_hmc_step` of mcmc.py: the one checking path
    (`_check_chain` with the stash) refuses, and nothing is launched."""
    from counting_lib import install
    F = lsnf_amd.flow
    lib = lsnf_amd.load_library()
    plan = F.FlowPlan(8, 4, 2, 1, torch.zeros(lib.lsnf_plan_floats(8, 4, 2, 1)), torch.zeros(lib.lsnf_prepare_scratch_bytes(8, 4, 2) // 8, dtype=torch.float64))
    stand = install(monkeypatch, lsnf_amd)
    seen = []
    real = lsnf_amd.mcmc._check_chain

    def spy(*a, **k):
        seen.append(k.get("stash"))
        return real(*a, **k)
    monkeypatch.setattr(lsnf_amd.mcmc, "_check_chain", spy)
    eps, v, saved = torch.zeros(5, 8), torch.zeros(5), torch.zeros(1, 5, 8)
    act = torch.zeros(lib.lsnf_act_saved_floats(8, 4, 2, 5))
    for kw in (dict(phase="init"), dict(uniform=v), dict(propose=False, inplace=True)):
        with pytest.raises(lsnf_amd.LsnfError):
            F.reverse_hmc_step(plan, eps, saved, act, eps.clone(), v, F.new_hmc_state(plan, 5, "cpu"), F.PhiloxNoise(3), 0.5, **kw)
    with pytest.raises(lsnf_amd.LsnfError):
        F.reverse_hmc_step(plan, eps, saved, act, eps.clone(), v, F.new_hmc_state(plan, 5, "cpu"), None, 0.5, phase="inner")
    with pytest.raises(lsnf_amd.LsnfError):
        F.reverse_hmc_step(plan, eps, saved, act, None, None, F.new_mala_state(plan, 5, "cpu"), F.PhiloxNoise(3), 0.5)      # the state is an HmcState
    assert len(seen) == 5 and all(st is not None and st[0] is saved and st[1] is act for st in seen)      # every call went through _check_chain
    with pytest.raises(lsnf_amd.LsnfError):
        F.reverse_hmc_step(plan, eps, saved, act, None, None, F.new_hmc_state(plan, 5, "cpu"), F.PhiloxNoise(3), 0.5, phase="middle")
    assert stand.launching() == [], dict(stand.entered)


# ---- the float64 restatement -----------------------------------------------------------------------------------------------
def _setup(nz=8, w=4, depth=3, B=64, seed=5):
    p = O.init_params(nz, w, depth, seed=seed, dtype=torch.float64)
    g = torch.Generator().manual_seed(17)
    eps0 = torch.randn(B, nz, generator=g, dtype=torch.float64)
    return p, g, eps0, RM.Quadratic(nz, 0.3, seed=9)


def test_one_leapfrog_step_is_the_base_space_mala_decision():
    """L = 1: log_alpha equals rmala_restated.decide's on the same state, proposal and uniform to 1e-10 relative (kinL = A / (2 s^2),
    kin0 = Bq / (2 s^2)), and the chains are the same chain."""
    p, g, eps0, quad = _setup()
    s, B, nz = 0.7, eps0.shape[0], eps0.shape[1]
    noises = [torch.randn(B, nz, generator=g, dtype=torch.float64) for _ in range(3)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g, dtype=torch.float64).clamp_min(1e-300) for _ in range(3)]
    calls, _ = RH.chain(p, eps0, quad, s, 1, noises, uniforms)
    steps, _ = RM.chain(p, eps0, quad, s, noises, uniforms)
    assert [c.phase for c in calls] == ["init", "end", "end", "end"] and len(steps) == 3
    for c, st in zip(calls[1:], steps):
        assert torch.allclose(c.e_prop, st.e_prop, rtol=0, atol=1e-12)                       # the leapfrog proposal is MALA's
        la, _, A, Bq = RM.decide(c.e_acc, c.g_acc, c.u_acc, c.e_prop, c.g, c.U_prop, c.u, s)
        scale = c.u_acc.abs() + c.U_prop.abs() + (A + Bq) / (2.0 * s * s)
        assert bool(((c.la - la).abs() <= 1e-10 * scale).all())
        assert torch.equal(c.acc, st.acc)
    assert 0 < sum(int(c.acc.sum()) for c in calls[1:]) < 3 * B


@pytest.mark.parametrize("L", [1, 3, 5])
def test_a_trajectory_is_reversible(L):
    """L steps, the momentum negated, L steps: back at the start to 1e-10, and the second log_alpha is minus the first."""
    p, g, eps0, quad = _setup()
    s, B, nz = 0.4, eps0.shape[0], eps0.shape[1]
    xi = torch.randn(B, nz, generator=g, dtype=torch.float64)
    u = torch.full((B,), 0.5, dtype=torch.float64)
    calls, _ = RH.chain(p, eps0, quad, s, L, [xi, None], [None, u])
    last = calls[-1]
    assert last.phase == "end" and len(calls) == L + 1
    back, _ = RH.chain(p, last.e_prop, quad, s, L, [-last.pL, None], [None, u])
    assert float((back[-1].e_prop - eps0).abs().max()) <= 1e-10
    assert float((back[-1].pL + xi).abs().max()) <= 1e-10
    assert float((back[-1].la + last.la).abs().max()) <= 1e-10 and float(last.la.abs().max()) > 1e-3


def test_restated_chain_leaves_the_standard_normal_invariant():
    """quad = None: the target is N(0, I) whatever the flow.  20 000 float64 rows started from exact N(0, I) samples, K = 4 trajectories
    of L = 3 steps: per column, the mean stays within four standard errors of 0 (SE = 1 / sqrt(B)) and the variance within four of 1
    (SE = sqrt(2 / B), a normal's); both outcomes of the accept step occur, so the check covers it."""
    nz, B, K, L, s = 2, 20000, 4, 3, 1.3
    p = O.init_params(nz, 4, 1, seed=5, fcz_std=0.5, dtype=torch.float64)
    g = torch.Generator().manual_seed(11)
    eps0 = torch.randn(B, nz, generator=g, dtype=torch.float64)
    noises = [torch.randn(B, nz, generator=g, dtype=torch.float64) for _ in range(K)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g, dtype=torch.float64).clamp_min(1e-300) for _ in range(K)]
    calls, (ek, gk, uk) = RH.chain(p, eps0, None, s, L, noises, uniforms)
    assert len(calls) == K * L + 1
    assert torch.equal(gk, ek) and torch.allclose(uk, 0.5 * (ek * ek).sum(1), rtol=0, atol=1e-12)      # the prior's gradient is eps itself
    rate = torch.stack([c.acc for c in calls if c.phase == "end"]).double().mean().item()
    mean, var = ek.mean(0), ek.var(0)
    se_m, se_v = (1.0 / B) ** 0.5, (2.0 / B) ** 0.5
    print(f"[rhmc] invariance: acceptance {rate:.3f}, column means {mean.tolist()} (4 SE {4 * se_m:.3e}), variances {var.tolist()} (4 SE {4 * se_v:.3e})")
    assert 0.15 < rate < 0.999 and bool((ek != eps0).any(1).float().mean() > 0.5)
    assert bool((mean.abs() <= 4.0 * se_m).all()) and bool(((var - 1.0).abs() <= 4.0 * se_v).all())


def test_redraw_keeps_every_point_of_a_trajectory_clear_of_a_kink():
    nz, w, depth, B, L, s = 8, 4, 3, 64, 3, 0.9
    p = O.init_params(nz, w, depth, seed=3)
    g = torch.Generator().manual_seed(3)
    eps0 = torch.randn(B, nz, generator=g)
    noises = [torch.randn(B, nz, generator=g) for _ in range(2)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g) for _ in range(2)]
    calls, _ = RH.chain(p, eps0, RM.Quadratic(nz, 0.1, seed=9), s, L, noises, uniforms, redraw=g)
    assert len(calls) == 2 * L + 1
    for c in calls[1:]:
        assert bool((O.relu_margin(p, c.x) > 2e-5).all())


def test_cost_tool_is_a_driver_on_the_ab_harness():
    """tools/rhmc_step_vs_rmala_step.py: its child's source is valid and importing the driver does not import torch."""
    import subprocess
    import sys
    tools = os.path.join(ROOT, "tools")
    code = ("import sys; sys.path.insert(0, %r)\nimport ab_harness, rhmc_step_vs_rmala_step as t\n"
            "compile(ab_harness.PRELUDE + t.CHILD, 'child', 'exec')\nassert 'torch' not in sys.modules\n"
            "assert t.SIZES == (100, 16384)" % tools)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=60)

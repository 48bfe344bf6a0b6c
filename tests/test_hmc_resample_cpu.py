"""CPU: the resampling move of the annealing HMC end calls (`lsnf_hmc_step_resample`, `lsnf_reverse_hmc_step_resample`,
include/lsnf_flow_mcmc.h): the C declarations and the ctypes binding outside the core ABI, the Python layers, every refusal the move
adds pinned through the entry points' own check before any HIP call (fake aligned pointers that are never dereferenced, as
tests/test_hmc_exchange_cpu.py), and the properties of the restated systematic resampling (tests/hmc_resample_restated.py): the
offspring counts, their sum, their mean over a fine grid of u, the clamp at u -> 1, the hand-made group, and that the forcing of
tests/hmc_resample_gpu.py finds a uniform for every group of every case from the restatement alone."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from conftest import ROOT
import hmc_resample_restated as R

import lsnf_amd

LSNF_OK, LSNF_E_ARG = 0, -1
INIT, INNER, ADAPT, LAST, FOLD, CLOSE, ANNEAL, SWAP, ODD, RESAMPLE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
NAMES = ("lsnf_hmc_step_resample", "lsnf_reverse_hmc_step_resample")
TEMPERED = {"lsnf_hmc_step_resample": "lsnf_hmc_step_tempered", "lsnf_reverse_hmc_step_resample": "lsnf_reverse_hmc_step_tempered"}
COUNT = {"lsnf_hmc_step_resample": 44, "lsnf_reverse_hmc_step_resample": 42}
FIVE = ["group", "ess_frac", "resample_uniform", "ancestor_out", "ess_out"]
FAKE = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(40)]     # 16-byte aligned addresses that are never dereferenced on the host


def test_symbols_are_declared_exported_and_bound_outside_the_core_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow_mcmc.h")).read(), flags=re.S)
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    ext = lsnf_amd._lib._EXT_SIGNATURES
    assert len(re.findall(r"#define\s+LSNF_HMC_RESAMPLE\s+512u", hdr)) == 1
    decl = lambda name: [re.sub(r".*[\s*]", "", a.strip())
                         for a in re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1).split(",")]
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and name not in core and hasattr(lib, name)
        assert name in ext and len(ext[name][1]) == COUNT[name] and name not in lsnf_amd.exported_symbols() and name not in lsnf_amd._lib._SIGNATURES
        assert getattr(lib, name).argtypes == ext[name][1]               # attached in load()
        names, tempered = decl(name), decl(TEMPERED[name])
        assert tempered[-1] == "stream" and names == tempered[:-1] + FIVE + ["stream"] and len(names) == COUNT[name]
        args, targs = ext[name][1], ext[TEMPERED[name]][1]
        assert args[:len(targs) - 1] == targs[:-1] and args[-1] == targs[-1]
        assert args[-6:-1] == [ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        assert len(targs) == COUNT[name] - 5                 # the tempered declarations are what they were
    assert lsnf_amd._lib.extension_symbols() == sorted(ext)
    assert lib.lsnf_abi_version() == 5 and lsnf_amd._lib.ABI_VERSION == 5
    # the header states the move line by line, and the counter field of its uniform
    text = open(os.path.join(ROOT, "include", "lsnf_flow_mcmc.h")).read()
    for said in ("l_i = w_i - c_i", "e_i = expf(l_i - m)", "ess = (S1 * S1) / S2", "tau_k = (((float)k + u) / P) * S1", "counter field value 4",
                 "a_k = min(#{ j : cum_j <= tau_k }, P - 1)", "m + logf(S1 / P)"):
        assert said in text, said


def test_python_layers_exist():
    F, L, M = lsnf_amd.flow, lsnf_amd.langevin, lsnf_amd.mcmc
    assert F.hmc_step_resample is M.hmc_step_resample and F.reverse_hmc_step_resample is M.reverse_hmc_step_resample
    assert F.HMC_RESAMPLE == M.HMC_RESAMPLE == 512
    new = ["resample", "ess_threshold", "resample_uniform"]
    for fn, old in ((F.hmc_step_resample, F.hmc_step_tempered), (F.reverse_hmc_step_resample, F.reverse_hmc_step_tempered),
                    (lsnf_amd._netF.hmc_step_resample, lsnf_amd._netF.hmc_step_tempered),
                    (lsnf_amd._netF.reverse_hmc_step_resample, lsnf_amd._netF.reverse_hmc_step_tempered)):
        a, b = inspect.signature(fn).parameters, inspect.signature(old).parameters
        assert [n for n in a] == [n for n in b] + new
        for n in new:
            assert a[n].kind is inspect.Parameter.KEYWORD_ONLY
        assert a["resample"].default is None and a["ess_threshold"].default == 0.5 and a["resample_uniform"].default is None
        for n in b:
            assert a[n].kind == b[n].kind and a[n].default == b[n].default
    for fn in (L.estimate_log_px_smc_z_with_flow, L.estimate_log_px_smc_eps_with_flow):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["x", "netG", "netF", "betas", "chains", "particles", "leapfrog_steps", "g_l_step_size", "g_llhd_sigma",
                                        "philox", "ess_threshold", "steps", "metric"]
        for kw in list(sig.parameters)[3:]:
            assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
        assert sig.parameters["ess_threshold"].default == 0.5 and sig.parameters["steps"].default is None
        for said in ("Philox field 4", "resampled", "without a host synchronisation"):
            assert said in fn.__doc__
    # the tempered and exchanging layers keep their signatures
    assert list(inspect.signature(F.hmc_step_tempered).parameters)[-1] == "anneal"
    assert list(inspect.signature(F.hmc_step_exchange).parameters)[-1] == "swap_uniform"
    assert len(lsnf_amd._lib._EXT_SIGNATURES["lsnf_hmc_step_tempered"][1]) == 39
    assert len(lsnf_amd._lib._EXT_SIGNATURES["lsnf_hmc_step_exchange"][1]) == 43


# ---- the refusals of the two entry points ------------------------------------------------------------------------------------
Z_ARGS = ("plan", "point", "z_out", "saved", "act", "ll", "grad_g", "energy", "p_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")
E_ARGS = ("plan", "point", "saved", "act", "grad_g", "energy", "p_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")


def _caller(lib, name):
    Rng, Da, Reg = lsnf_amd._lib.LsnfRng, lsnf_amd._lib.LsnfDualAvg, lsnf_amd._lib.LsnfMetricReg
    order = Z_ARGS if name == "lsnf_hmc_step_resample" else E_ARGS
    ptrs = dict(zip(order + ("step_rows", "adapt", "scale", "mean", "m2", "count", "beta", "beta_next", "like_grad", "like_u", "log_w", "next",
                             "accept", "la", "resample_uniform", "ancestor_out", "ess_out"), FAKE))
    base = dict(ptrs, nz=128, w=64, d=5, c=1, B=16, rng=None, da=None, adapt=None, mean=None, m2=None, count=None, reg=None, beta_next=None,
                log_w=None, flags=0, accept=None, la=None, group=0, ess_frac=0.5, resample_uniform=None, ancestor_out=None, ess_out=None)
    fn = getattr(lib, name)

    def call(**kw):
        a = dict(base, **kw)
        return fn(a["plan"], a["nz"], a["w"], a["d"], a["c"], a["B"], *(a[k] for k in order[1:]),
                  None if a["rng"] is None else ctypes.byref(a["rng"]), a["step_rows"], a["adapt"],
                  None if a["da"] is None else ctypes.byref(a["da"]), a["scale"], a["mean"], a["m2"], a["count"],
                  None if a["reg"] is None else ctypes.byref(a["reg"]), a["beta"], a["beta_next"], a["like_grad"], a["like_u"], a["log_w"],
                  a["flags"], a["next"], a["accept"], a["la"], a["group"], a["ess_frac"], a["resample_uniform"], a["ancestor_out"],
                  a["ess_out"], None)

    def said(code, text, **kw):
        rc = call(**kw)
        return rc == code and lib.lsnf_last_error().decode() == name + ": " + text
    return call, said, ptrs, Rng, Da, Reg


@pytest.mark.parametrize("name", NAMES)
def test_every_new_rule_refuses_before_any_hip_call(name):
    lib = lsnf_amd.load_library()
    call, said, P, Rng, Da, Reg = _caller(lib, name)
    z = name == "lsnf_hmc_step_resample"
    point = "z_prop" if z else "eps_prop"
    da = Da(target_accept=0.8, gamma=0.05, t0=10.0, kappa=0.75, step_min=1e-4, step_max=1e2)
    reg = Reg(n0=5.0, var0=1e-3, scale_min=1e-3, scale_max=1e3)
    annealing = dict(beta_next=P["beta_next"], log_w=P["log_w"])
    moving = dict(flags=RESAMPLE | ANNEAL, group=4, resample_uniform=P["resample_uniform"], ancestor_out=P["ancestor_out"], ess_out=P["ess_out"],
                  **annealing)
    folding = dict(mean=P["mean"], m2=P["m2"], count=P["count"], reg=reg)
    adapting = dict(adapt=P["adapt"], da=da)
    philox = dict(noise=None, uniform=None, rng=Rng(1, 0, None, 0))
    E = LSNF_E_ARG
    for B in (0, 16):                                        # rules that precede the empty-batch return: the same answer for B = 0
        assert said(E, "unknown flag bits 0x400", B=B, **dict(moving, flags=RESAMPLE | ANNEAL | 0x400))
        # the swap is not among these entries' flags
        assert said(E, "unknown flag bits 0x80", B=B, **dict(moving, flags=RESAMPLE | ANNEAL | SWAP))
        assert said(E, "unknown flag bits 0x180", B=B, flags=SWAP | ODD)
        end_only = "flags: LSNF_HMC_RESAMPLE goes with an end call (neither LSNF_HMC_INIT nor LSNF_HMC_INNER)"
        assert said(E, end_only, B=B, **dict(moving, flags=RESAMPLE | ANNEAL | INIT, uniform=None))
        assert said(E, end_only, B=B, **dict(moving, flags=RESAMPLE | INNER, noise=None, uniform=None, beta_next=None, log_w=None))
        assert said(E, "flags: LSNF_HMC_RESAMPLE goes with LSNF_HMC_ANNEAL", B=B, **dict(moving, flags=RESAMPLE, beta_next=None, log_w=None))
        frozen = "flags: LSNF_HMC_RESAMPLE excludes LSNF_HMC_ADAPT, LSNF_HMC_METRIC_FOLD and LSNF_HMC_METRIC_CLOSE"
        assert said(E, frozen, B=B, **dict(moving, flags=RESAMPLE | ANNEAL | ADAPT, **adapting))
        assert said(E, frozen, B=B, **dict(moving, flags=RESAMPLE | ANNEAL | ADAPT | LAST, **adapting))
        assert said(E, frozen, B=B, **dict(moving, flags=RESAMPLE | ANNEAL | FOLD, **folding))
        assert said(E, frozen, B=B, **dict(moving, flags=RESAMPLE | ANNEAL | FOLD | CLOSE, **folding))
        for bad in (0, 1, 3, 5, 6, 12, 32, -4):
            assert said(E, f"group must be 2, 4, 8 or 16 with LSNF_HMC_RESAMPLE (got {bad})", B=B, **dict(moving, group=bad))
        none = "resample_uniform, ancestor_out and ess_out must be NULL without LSNF_HMC_RESAMPLE"
        for k in ("resample_uniform", "ancestor_out", "ess_out"):
            assert said(E, none, B=B, **{k: P[k]}) and said(E, none, B=B, flags=INIT, uniform=None, **{k: P[k]})
            assert said(E, none, B=B, flags=ANNEAL, group=4, **dict(annealing, **{k: P[k]}))
        assert said(E, "resample_uniform goes with a noise tensor, not with an rng (the group's uniform is drawn in-kernel)", B=B,
                    **dict(moving, **philox))
        # the move's arrays alias nothing else the call touches
        assert said(E, "ancestor_out must not alias uniform", B=B, **dict(moving, ancestor_out=P["uniform"]))
        assert said(E, "ancestor_out must not alias resample_uniform", B=B, **dict(moving, ancestor_out=P["resample_uniform"]))
        assert said(E, "u_acc must not alias resample_uniform", B=B, **dict(moving, resample_uniform=P["u_acc"]))
        assert said(E, "log_w must not alias ess_out", B=B, **dict(moving, ess_out=P["log_w"]))
        assert said(E, "ancestor_out must not alias ess_out", B=B, **dict(moving, ess_out=P["ancestor_out"]))
        assert said(E, "accept_out must not alias ancestor_out", B=B, **dict(moving, accept=P["ancestor_out"]))
        # the tempered call's rules, word for word (a sample: the whole table is tests/test_hmc_tempered_cpu.py's)
        assert said(E, "beta_next and log_w must be NULL without LSNF_HMC_ANNEAL", B=B, beta_next=P["beta_next"])
        assert said(E, "flags: LSNF_HMC_INIT and LSNF_HMC_INNER exclude each other", B=B, flags=INIT | INNER, noise=None, uniform=None)
        assert said(E, f"like_grad_acc must not alias {point}", B=B, **dict(moving, like_grad=P["point"]))
    for B, G in ((15, 2), (18, 4), (20, 8), (24, 16), (8, 16), (1, 2)):
        assert said(E, f"B={B} is not a multiple of group={G}", B=B, **dict(moving, group=G))
    # an empty batch: nothing to launch, NULL pointers allowed, resampling or not
    nulls = {k: None for k in P}
    assert call(B=0, **nulls) == LSNF_OK and call(B=0, **dict(nulls, flags=RESAMPLE | ANNEAL, group=8)) == LSNF_OK
    assert call(B=0, **moving) == LSNF_OK
    # the pointers of a non-empty call
    assert said(E, "resample_uniform is required with LSNF_HMC_RESAMPLE when no rng is given", **dict(moving, resample_uniform=None))
    assert said(E, "beta_next and log_w are required with LSNF_HMC_ANNEAL", **dict(moving, log_w=None))
    odd = ctypes.c_void_p(0xF00002)
    for k in ("resample_uniform", "ancestor_out", "ess_out"):
        assert said(E, f"{k} must be 4-byte aligned", **dict(moving, **{k: odd}))
    assert said(E, "beta_rows is required (NULL)", **dict(moving, beta=None))
    assert said(E, "uniform is required without an rng (unless LSNF_HMC_INIT or LSNF_HMC_INNER)", **dict(moving, uniform=None))
    # (the next rule -- a misaligned act_saved -- is what refuses a call that passed all others: ancestor_out and ess_out are optional,
    # the uniform comes from a tensor or from the rng, every group length and every ess_frac pass, a call without the flag ignores group)
    bad_act = ctypes.c_void_p(0x50008)
    off4 = lambda k: ctypes.c_void_p(P[k].value + 4)
    for ok in (dict(), dict(group=3), moving, dict(moving, ancestor_out=None), dict(moving, ess_out=None), dict(moving, ancestor_out=None, ess_out=None),
               dict(moving, resample_uniform=None, **philox), dict(moving, noise=None, **{"next": None}),
               dict(moving, resample_uniform=off4("resample_uniform"), ancestor_out=off4("ancestor_out"), ess_out=off4("ess_out")),
               dict(moving, ess_frac=0.0), dict(moving, ess_frac=-1.0), dict(moving, ess_frac=2.0),
               dict(flags=ANNEAL, **annealing), dict(flags=INNER, noise=None, uniform=None)) + \
            tuple(dict(moving, group=G) for G in (2, 4, 8, 16)):
        assert said(E, "act_saved must be 16-byte aligned", **dict(ok, act=bad_act))


def test_the_tempered_and_exchanging_entry_points_still_refuse_the_new_bit():
    """Nothing about the tempered and the exchanging entry points changed: bit 0x200 is unknown there."""
    import test_hmc_tempered_cpu as T
    import test_hmc_exchange_cpu as XC
    lib = lsnf_amd.load_library()
    for mod in (T, XC):
        for name in mod.NAMES:
            said = mod._caller(lib, name)[1]
            assert said(LSNF_E_ARG, "unknown flag bits 0x200", flags=RESAMPLE)
            assert said(LSNF_E_ARG, "unknown flag bits 0x200", flags=RESAMPLE | ANNEAL)


# ---- the Python wrappers on CPU tensors ------------------------------------------------------------------------------------------------
def _plan():
    F, lib = lsnf_amd.flow, lsnf_amd.load_library()
    return F.FlowPlan(8, 4, 2, 1, torch.zeros(lib.lsnf_plan_floats(8, 4, 2, 1)), torch.zeros(lib.lsnf_prepare_scratch_bytes(8, 4, 2) // 8, dtype=torch.float64))


def test_wrappers_refuse_a_misplaced_resample_before_anything_else(monkeypatch):
    F, M = lsnf_amd.flow, lsnf_amd.mcmc
    lib = lsnf_amd.load_library()
    plan, B = _plan(), 8
    z, saved = torch.zeros(B, 8), torch.zeros(1, B, 8)
    act = torch.zeros(lib.lsnf_act_saved_floats(8, 4, 2, B))
    steps, state, metric = F.new_hmc_row_steps(B, "cpu", 0.5), F.new_hmc_state(plan, B, "cpu"), F.new_hmc_row_metric(plan, B, "cpu")
    temper, bn = F.new_hmc_row_temper(plan, B, "cpu"), torch.full((B,), 0.25)
    zcall = lambda **kw: F.hmc_step_resample(plan, z, None, None, state, F.PhiloxNoise(3), steps, metric, temper, **kw)
    ecall = lambda **kw: F.reverse_hmc_step_resample(plan, z, saved, act, None, None, state, F.PhiloxNoise(3), steps, metric, temper, **kw)
    for call in (zcall, ecall):
        for bad in (3, 1, 32, "4", 0):
            with pytest.raises(lsnf_amd.LsnfError, match="resample must be None, 2, 4, 8 or 16"):
                call(anneal=bn, resample=bad)
        for kw in (dict(phase="init", anneal=bn), dict(phase="inner"), dict(anneal=None), dict(anneal=bn, adapt="update"),
                   dict(anneal=bn, window="fold")):
            with pytest.raises(lsnf_amd.LsnfError, match="resample goes with phase='end' and anneal="):
                call(resample=4, **kw)
        for kw in (dict(), dict(anneal=bn), dict(anneal=bn, resample=4), dict(anneal=bn, resample=8, ess_threshold=2.0, propose=False)):
            with pytest.raises(lsnf_amd.LsnfError, match="no CPU path"):
                call(**kw)
    # the move's uniforms go through the one checking path; its own rules come after it
    cpu, ru, rng = torch.device("cpu"), torch.zeros(B), object()
    with pytest.raises(lsnf_amd.LsnfError, match="resample_uniform must live on"):
        M._row_resample_args(plan, 4, 0.5, ru, None, B, torch.device("cuda:0"), False)
    with monkeypatch.context() as m:
        m.setattr(M, "_check_in", lambda t, name, need, dev, *a, **k: None)
        assert M._row_resample_args(plan, None, 0.5, None, rng, B, cpu, False) == ((0, 0.0, None, None, None), None, None)
        with pytest.raises(lsnf_amd.LsnfError, match="resample_uniform goes with resample=P"):
            M._row_resample_args(plan, None, 0.5, ru, None, B, cpu, False)
        with pytest.raises(lsnf_amd.LsnfError, match="are not a multiple of resample=16"):
            M._row_resample_args(plan, 16, 0.5, None, rng, B, cpu, False)
        for bad in ((ru, rng), (None, None)):
            with pytest.raises(lsnf_amd.LsnfError, match="the move draws as the trajectory does"):
                M._row_resample_args(plan, 4, 0.5, bad[0], bad[1], B, cpu, False)
        args, ancestor, ess = M._row_resample_args(plan, 4, 0.75, ru, None, B, cpu, False)
        assert args == (4, 0.75, ru.data_ptr(), ancestor.data_ptr(), ess.data_ptr()) and ancestor.shape == ess.shape == (B,)
        args = M._row_resample_args(plan, 8, 0.5, None, rng, B, cpu, False)[0]
        assert args[:3] == (8, 0.5, None)            # (reuse_buffers keeps the outputs on the plan per stream: tests/hmc_resample_gpu.py)
    L = lsnf_amd.langevin
    for fn in (L.estimate_log_px_smc_z_with_flow, L.estimate_log_px_smc_eps_with_flow):
        for chains, particles in ((8, 3), (8, 16), (12, 8), (8, 1), (64, 32)):
            with pytest.raises(ValueError, match="particles must be 2, 4, 8 or 16 and divide chains"):
                fn(torch.zeros(2, 8), None, None, betas=[0.0, 1.0], chains=chains, particles=particles, leapfrog_steps=1, g_l_step_size=0.1,
                   g_llhd_sigma=1.0, philox=None)
        assert fn(torch.zeros(2, 8), None, None, betas=[0.0], chains=8, particles=4, leapfrog_steps=1, g_l_step_size=0.1, g_llhd_sigma=1.0,
                  philox=None) == (None,) * 7


# ---- the restated systematic resampling --------------------------------------------------------------------------------------------
def _weights(P, seed, spread=3.0):
    g = torch.Generator().manual_seed(seed)
    return (spread * torch.randn(64 * P, generator=g, dtype=torch.float64)).clamp(-60.0, 60.0)


@pytest.mark.parametrize("P", R.GROUPS)
def test_offspring_counts_are_floor_or_ceil_of_the_expected_number_and_sum_to_P(P):
    l = _weights(P, 10 + P)
    G = l.shape[0] // P
    W = torch.softmax(l.view(G, P), dim=1)
    grid = (torch.arange(2048, dtype=torch.float64) + 0.5) / 2048.0
    mean = torch.zeros(G, P, dtype=torch.float64)
    for u in grid.tolist():
        d = R.decide(l, torch.full_like(l, u), P, 2.0)       # (ess_frac = 2: every group resamples)
        assert bool(d.on.all())
        n = R.offspring(d.rung, P)
        assert bool((n.sum(dim=1) == P).all())
        assert bool(((n >= torch.floor(P * W - 1e-9)) & (n <= torch.ceil(P * W + 1e-9))).all())
        r = d.rung.view(G, P)
        assert bool((r[:, 1:] >= r[:, :-1]).all())           # systematic: the ancestors are sorted
        mean += n
    mean /= grid.numel()
    # the mean over a grid of n points is within one grid cell per threshold crossing of the expected number
    assert bool(((mean - P * W).abs() <= P / grid.numel() + 1e-12).all())


def test_clamp_at_u_to_one_and_the_threshold_edges():
    f32 = torch.float32
    for P in R.GROUPS:
        l = torch.zeros(P, dtype=f32)                        # equal weights: e_i = 1, cum_j = j + 1, tau_k = k + u
        for u in (0.0, 0.25, 1.0 - 2.0 ** -12):
            d = R.decide(l, torch.full((P,), u, dtype=f32), P, 2.0)
            assert d.rung.tolist() == list(range(P)) and d.ess[0].item() == float(P) and d.lw[0].item() == 0.0
        # u = 1.0f (the in-kernel number's formula can round to it): tau_k = k + 1 = cum_k, the count is k + 1 and the last rung's P
        # is clamped to P - 1
        d = R.decide(l, torch.ones(P, dtype=f32), P, 2.0)
        assert d.rung.tolist() == [min(k + 1, P - 1) for k in range(P)] and int(d.rung.max()) == P - 1
        # in float64 a u just below 1 keeps every rung its own
        d = R.decide(l.double(), torch.full((P,), 1.0 - 2.0 ** -25, dtype=torch.float64), P, 2.0)
        assert d.rung.tolist() == list(range(P))
        # never and always; ess = P at equal weights is not below 1.0 * P
        assert not R.decide(l, torch.zeros(P), P, 0.0).on.any() and not R.decide(l, torch.zeros(P), P, -1.0).on.any()
        assert not R.decide(l, torch.zeros(P), P, 1.0).on.any() and bool(R.decide(l, torch.zeros(P), P, 1.0 + 1e-6).on.all())
        # a group of two can never resample at 0.5: ess >= 1
        if P == 2:
            assert not R.decide(torch.tensor([0.0, -50.0], dtype=f32), torch.zeros(2), 2, 0.5).on.any()
    # a NaN anywhere leaves the group alone and the other groups as they are
    l = torch.tensor([0.0, -5.0, float("nan"), -5.0, 0.0, -5.0, -5.0, -5.0], dtype=torch.float64)
    d = R.decide(l, torch.full((8,), 0.5, dtype=torch.float64), 4, 2.0)
    assert d.on.tolist() == [False] * 4 + [True] * 4 and d.rung.tolist() == [0, 1, 2, 3, 0, 0, 0, 0] and bool(torch.isnan(d.ess[:4]).all())


def test_the_lines_on_a_hand_made_group():
    f64 = torch.float64
    l = torch.log(torch.tensor([0.5, 0.25, 0.125, 0.125], dtype=f64)) + 7.0
    d = R.decide(l, torch.full((4,), 0.5, dtype=f64), 4, 0.9)
    # e = 1, 1/2, 1/4, 1/4; S1 = 2, S2 = 1.375; ess = 2.909 < 3.6; tau = (k + 0.5) / 4 * 2 = 0.25, 0.75, 1.25, 1.75; cum = 1, 1.5, 1.75, 2
    assert torch.allclose(d.s1, torch.tensor([2.0], dtype=f64)) and abs(d.ess[0].item() - 4.0 / 1.375) < 1e-12 and bool(d.on.all())
    assert d.rung.tolist() == [0, 0, 1, 3] and d.ancestor.tolist() == [0, 0, 1, 3]
    assert abs(d.lw[0].item() - (7.0 + math.log(0.25))) < 1e-12      # log of the mean weight: the normalising constant's estimate is kept
    assert not R.decide(l, torch.full((4,), 0.5, dtype=f64), 4, 0.7).on.any()
    beta = torch.tensor([0.25, 0.5, 0.5, 1.0], dtype=f64)
    z, g, gl = (torch.arange(8, dtype=f64).view(4, 2) + k for k in (0.0, 10.0, 20.0))
    u, el = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=f64), torch.tensor([5.0, 3.0, 1.0, 4.0], dtype=f64)
    z2, g2, u2, gl2, el2 = R.gather(beta, z, g, u, gl, el, d.ancestor)
    assert torch.equal(z2[0], z[0]) and torch.equal(z2[3], z[3]) and torch.equal(g2[0], g[0]) and u2[3].item() == 4.0
    assert torch.equal(z2[1], z[0]) and torch.equal(z2[2], z[1]) and torch.equal(gl2[1], gl[0]) and el2.tolist() == [5.0, 5.0, 3.0, 4.0]
    assert torch.equal(g2[1], g[0] + (0.5 - 0.25) * gl[0]) and torch.equal(g2[2], g[1]) and u2[1].item() == 1.0 + 0.25 * 5.0 and u2[2].item() == 2.0
    # the potential at a row's own beta is what a fresh evaluation of the ancestor's state gives: u = prior + beta el
    prior = u - beta * el
    assert torch.allclose(u2, prior[d.ancestor] + beta * el[d.ancestor], rtol=0, atol=1e-14)


def test_the_forcing_finds_a_uniform_for_every_group_of_every_case_from_the_restatement_alone():
    """tests/hmc_resample_gpu.py `targets` / `forced` on the CPU: every group of every case gets a candidate that clears the margin,
    the meant decisions come out, and every launch of more than one group has both kinds of group and a row that moves."""
    import hmc_resample_gpu as SG
    assert SG.MARGIN >= 50.0 and R.err(16, SG.LMAX) == 2.0 ** -24 * (128.0 + 2.0 * R.EXP_ULP + 18.0)
    worst = (float("inf"), float("inf"))
    for case in SG.MOVE + SG.FORMS:
        B, P = case[-2:]
        for first in (True, False):
            tgt, want = SG.targets(B, P, first, P + SG.DESIGN_SEED.get(tuple(case), 0))
            assert float(tgt.abs().max()) <= 48.0
            u, d, gap, edge = SG.forced(tgt, P, SG.threshold_of(P))
            assert torch.equal(d.group_on, want) and gap >= SG.MARGIN and edge >= SG.MARGIN, (case, first, gap, edge)
            if B // P > 1:
                assert bool((d.ancestor != torch.arange(B)).any()) and bool(d.on.any()) and bool((~d.on).any())
            worst = (min(worst[0], gap), min(worst[1], edge))
    print(f"forcing: nearest threshold {worst[0]:.1f} err, nearest ess edge {worst[1]:.0f} x 4 err over {len(SG.MOVE + SG.FORMS)} cases")

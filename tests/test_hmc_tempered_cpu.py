"""CPU: the likelihood temperature per row of Hamiltonian Monte Carlo and annealed importance sampling (`lsnf_hmc_step_tempered`,
`lsnf_reverse_hmc_step_tempered`, include/lsnf_flow_mcmc.h): the C declarations and the ctypes binding outside the core ABI, the Python
layers, every refusal the entry points make before any HIP call (fake aligned pointers that are never dereferenced, as
tests/test_hmc_metric_cpu.py), the samplers' exact sequence of calls, the schedule, and the properties of the float64 restatements
alone (tests/hmc_tempered_restated.py, tests/ais_restated.py).

The AIS experiment (`ais_restated.experiment`: the affine TINY flow as a Gaussian prior, netG(z) = diag(a) z with a log-spaced from 0.3
to 3.0, sigma = 1, two data x 64 chains, T = 100 sigmoid temperatures, L = 3, frozen step 0.28) was run on the CPU at seeds 0 .. 7 for the
chain on z and for the one on eps (profiles/ais_cpu.txt has every seed's figures and the arithmetic of the bands: the observed range
widened by 3 standard errors of one run).  The bands are on `estimate - closed form`; the closed form itself lies inside them."""
import ctypes
import inspect
import math
import os
import re
import types

import pytest
import torch

from conftest import ROOT
import ais_restated as A
import hmc_metric_restated as MR
import hmc_rows_restated as R
import hmc_tempered_restated as TR

import lsnf_amd

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2
INIT, INNER, ADAPT, LAST, FOLD, CLOSE, ANNEAL = 1, 2, 4, 8, 16, 32, 64
NAMES = ("lsnf_hmc_step_tempered", "lsnf_reverse_hmc_step_tempered")
METRIC = {"lsnf_hmc_step_tempered": "lsnf_hmc_step_metric", "lsnf_reverse_hmc_step_tempered": "lsnf_reverse_hmc_step_metric"}
COUNT = {"lsnf_hmc_step_tempered": 39, "lsnf_reverse_hmc_step_tempered": 37}
FIVE = ["beta_rows", "beta_next", "like_grad_acc", "like_u_acc", "log_w"]
FAKE = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(34)]     # 16-byte aligned addresses that are never dereferenced on the host
BAND = {                                                     # (profiles/ais_cpu.txt; ais_restated.BAND is held to it below)
    "z": {"error": (-0.863, 0.797), "ess": (9.1, 55.3), "accept": (0.954, 0.971)},
    "eps": {"error": (-0.642, 0.582), "ess": (18.1, 54.2), "accept": (0.888, 0.912)},
}


def test_symbols_are_declared_exported_and_bound_outside_the_core_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow_mcmc.h")).read(), flags=re.S)
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    ext = lsnf_amd._lib._EXT_SIGNATURES
    assert len(re.findall(r"#define\s+LSNF_HMC_ANNEAL\s+64u", hdr)) == 1 and len(re.findall(r"#define\s+LSNF_HMC_ANNEAL\b", hdr)) == 1
    decl = lambda name: [re.sub(r".*[\s*]", "", a.strip())
                         for a in re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1).split(",")]
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and name not in core and hasattr(lib, name)
        assert name in ext and len(ext[name][1]) == COUNT[name] and name not in lsnf_amd.exported_symbols() and name not in lsnf_amd._lib._SIGNATURES
        assert getattr(lib, name).argtypes == ext[name][1]               # attached in load()
        # the declaration's parameters: the metric call's with the five inserted between reg and flags
        names, metric = decl(name), decl(METRIC[name])
        at = metric.index("reg") + 1
        assert metric[at] == "flags" and len(names) == COUNT[name] == len(metric) + 5 and names == metric[:at] + FIVE + metric[at:]
        args, margs = ext[name][1], ext[METRIC[name]][1]
        assert args[:at] == margs[:at] and args[at + 5:] == margs[at:] and args[at:at + 5] == [ctypes.c_void_p] * 5
        assert len(margs) == COUNT[name] - 5                  # the metric declarations are what they were
    assert lsnf_amd._lib.extension_symbols() == sorted(ext)
    assert lib.lsnf_abi_version() == 5 and lsnf_amd._lib.ABI_VERSION == 5


def test_python_layers_exist_and_the_existing_ones_are_unchanged():
    F, L, M = lsnf_amd.flow, lsnf_amd.langevin, lsnf_amd.mcmc
    assert F.hmc_step_tempered is M.hmc_step_tempered and F.reverse_hmc_step_tempered is M.reverse_hmc_step_tempered
    assert F.HmcRowTemper is M.HmcRowTemper and F.new_hmc_row_temper is M.new_hmc_row_temper and F.HMC_ANNEAL == M.HMC_ANNEAL == 64
    for new, old in ((F.hmc_step_tempered, F.hmc_step_metric), (F.reverse_hmc_step_tempered, F.reverse_hmc_step_metric),
                     (lsnf_amd._netF.hmc_step_tempered, lsnf_amd._netF.hmc_step_metric),
                     (lsnf_amd._netF.reverse_hmc_step_tempered, lsnf_amd._netF.reverse_hmc_step_metric)):
        a, b = inspect.signature(new).parameters, inspect.signature(old).parameters
        want = []
        for n in b:
            want.append(n)
            if n == "metric":
                want.append("temper")
        assert [n for n in a] == want + ["anneal"]
        assert a["anneal"].kind is inspect.Parameter.KEYWORD_ONLY and a["anneal"].default is None
        for n in b:
            assert a[n].kind == b[n].kind and a[n].default == b[n].default
    assert [f for f in F.HmcRowTemper.__dataclass_fields__] == ["beta", "like_grad", "like_energy", "log_w"]
    sig = inspect.signature(F.new_hmc_row_temper)
    assert list(sig.parameters) == ["plan", "B", "device", "beta"] and sig.parameters["beta"].default == 0.0
    sig = inspect.signature(L.ais_schedule)
    assert list(sig.parameters) == ["T", "kind", "delta"] and (sig.parameters["kind"].default, sig.parameters["delta"].default) == ("sigmoid", 4.0)
    for fn in (L.estimate_log_px_ais_z_with_flow, L.estimate_log_px_ais_eps_with_flow):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["x", "netG", "netF", "betas", "chains", "leapfrog_steps", "g_l_step_size", "g_llhd_sigma", "philox",
                                        "steps", "metric", "adapt"]
        for kw in list(sig.parameters)[3:]:
            assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
        assert sig.parameters["steps"].default is None and sig.parameters["metric"].default is None and sig.parameters["adapt"].default is False
        for said in ("conservative", "approximately", "log(2 pi)", "philox.step(0)"):
            assert said in fn.__doc__
    # the existing layers keep their signatures and their fields
    assert [f for f in F.HmcRowMetric.__dataclass_fields__] == ["scale", "mean", "m2", "count", "n0", "var0", "scale_min", "scale_max"]
    assert [f for f in F.HmcRowSteps.__dataclass_fields__] == ["step", "adapt", "target_accept", "gamma", "t0", "kappa", "step_min", "step_max"]
    assert list(inspect.signature(M._check_chain).parameters) == ["plan", "point", "name", "grad_g", "energy_g", "state", "state_cls", "noise",
                                                                  "uniform", "stash"]
    assert len(lsnf_amd._lib._EXT_SIGNATURES["lsnf_hmc_step_metric"][1]) == 34 and len(lsnf_amd._lib._EXT_SIGNATURES["lsnf_reverse_hmc_step_metric"][1]) == 32
    assert list(inspect.signature(F.hmc_step_metric).parameters)[-1] == "window"


def _plan():
    F, lib = lsnf_amd.flow, lsnf_amd.load_library()
    return F.FlowPlan(8, 4, 2, 1, torch.zeros(lib.lsnf_plan_floats(8, 4, 2, 1)), torch.zeros(lib.lsnf_prepare_scratch_bytes(8, 4, 2) // 8, dtype=torch.float64))


def test_new_row_temper_fills_the_state():
    F, plan = lsnf_amd.flow, _plan()
    t = F.new_hmc_row_temper(plan, 5, "cpu")
    assert t.beta.shape == t.like_energy.shape == (5,) and t.like_grad.shape == (5, 8) and t.log_w.shape == (5, 2)
    assert all(x.dtype == torch.float32 for x in (t.beta, t.like_grad, t.like_energy, t.log_w))
    assert not t.beta.any() and not t.like_grad.any() and not t.like_energy.any() and not t.log_w.any()
    assert bool((F.new_hmc_row_temper(plan, 3, "cpu", 0.25).beta == 0.25).all())
    b = torch.rand(5)
    t = F.new_hmc_row_temper(plan, 5, "cpu", b)
    assert torch.equal(t.beta, b) and t.beta.data_ptr() != b.data_ptr()
    with pytest.raises(lsnf_amd.LsnfError):
        F.new_hmc_row_temper(plan, 4, "cpu", b)
    t.log_w[:, 0], t.log_w[:, 1] = torch.arange(5.0), 0.5
    lw = t.log_weight()
    assert lw.dtype == torch.float64 and lw.shape == (5,) and torch.equal(lw, torch.arange(5.0, dtype=torch.float64) - 0.5)


# ---- the refusals of the two entry points ------------------------------------------------------------------------------------
Z_ARGS = ("plan", "point", "z_out", "saved", "act", "ll", "grad_g", "energy", "p_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")
E_ARGS = ("plan", "point", "saved", "act", "grad_g", "energy", "p_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")


def _caller(lib, name):
    Rng, Da, Reg = lsnf_amd._lib.LsnfRng, lsnf_amd._lib.LsnfDualAvg, lsnf_amd._lib.LsnfMetricReg
    order = Z_ARGS if name == "lsnf_hmc_step_tempered" else E_ARGS
    ptrs = dict(zip(order + ("step_rows", "adapt", "scale", "mean", "m2", "count", "beta", "beta_next", "like_grad", "like_u", "log_w", "next",
                             "accept", "la"), FAKE))
    base = dict(ptrs, nz=128, w=64, d=5, c=1, B=4, rng=None, da=None, adapt=None, mean=None, m2=None, count=None, reg=None, beta_next=None,
                log_w=None, flags=0, accept=None, la=None)
    fn = getattr(lib, name)

    def call(**kw):
        a = dict(base, **kw)
        return fn(a["plan"], a["nz"], a["w"], a["d"], a["c"], a["B"], *(a[k] for k in order[1:]),
                  None if a["rng"] is None else ctypes.byref(a["rng"]), a["step_rows"], a["adapt"],
                  None if a["da"] is None else ctypes.byref(a["da"]), a["scale"], a["mean"], a["m2"], a["count"],
                  None if a["reg"] is None else ctypes.byref(a["reg"]), a["beta"], a["beta_next"], a["like_grad"], a["like_u"], a["log_w"],
                  a["flags"], a["next"], a["accept"], a["la"], None)

    def said(code, text, **kw):
        rc = call(**kw)
        return rc == code and lib.lsnf_last_error().decode() == name + ": " + text
    return call, said, ptrs, Rng, Da, Reg


@pytest.mark.parametrize("name", NAMES)
def test_every_new_rule_refuses_before_any_hip_call(name):
    lib = lsnf_amd.load_library()
    call, said, P, Rng, Da, Reg = _caller(lib, name)
    z = name == "lsnf_hmc_step_tempered"
    nxt, acc_name, point = ("z_next", "z_acc", "z_prop") if z else ("eps_next", "eps_acc", "eps_prop")
    da = Da(target_accept=0.8, gamma=0.05, t0=10.0, kappa=0.75, step_min=1e-4, step_max=1e2)
    reg = Reg(n0=5.0, var0=1e-3, scale_min=1e-3, scale_max=1e3)
    annealing = dict(flags=ANNEAL, beta_next=P["beta_next"], log_w=P["log_w"])
    folding = dict(flags=FOLD, mean=P["mean"], m2=P["m2"], count=P["count"], reg=reg)
    adapting = dict(flags=ADAPT, adapt=P["adapt"], da=da)
    inner = dict(flags=INNER, noise=None, uniform=None)
    E = LSNF_E_ARG
    for B in (0, 4):                                         # rules that precede the empty-batch return: the same answer for B = 0
        assert said(E, "unknown flag bits 0x80", B=B, flags=0x80) and said(E, "unknown flag bits 0x80", B=B, **dict(annealing, flags=0x80 | ANNEAL))
        assert said(E, "unknown flag bits 0x80000000", B=B, **dict(annealing, flags=0x80000000 | ANNEAL))
        not_inner = "flags: LSNF_HMC_ANNEAL goes with LSNF_HMC_INIT or an end call, not with LSNF_HMC_INNER"
        assert said(E, not_inner, B=B, **dict(annealing, **dict(inner, flags=ANNEAL | INNER)))
        assert said(E, not_inner, B=B, **dict(inner, flags=ANNEAL | INNER))
        none = "beta_next and log_w must be NULL without LSNF_HMC_ANNEAL"
        for k in ("beta_next", "log_w"):
            assert said(E, none, B=B, **{k: P[k]}) and said(E, none, B=B, **dict(inner, **{k: P[k]})) and said(E, none, B=B, flags=INIT, uniform=None, **{k: P[k]})
            assert said(E, none, B=B, **dict(folding, **{k: P[k]}))
        # the five arrays alias nothing else the call touches
        assert said(E, "beta_rows must not alias grad_g", B=B, beta=P["grad_g"]) and said(E, "beta_rows must not alias energy_g", B=B, beta=P["energy"])
        assert said(E, "u_acc must not alias beta_rows", B=B, beta=P["u_acc"]) and said(E, "step_rows must not alias beta_rows", B=B, beta=P["step_rows"])
        assert said(E, "like_grad_acc must not alias grad_g", B=B, like_grad=P["grad_g"]) and said(E, f"like_grad_acc must not alias {point}", B=B, like_grad=P["point"])
        assert said(E, "grad_acc must not alias like_grad_acc", B=B, like_grad=P["g_acc"]) and said(E, "mom must not alias like_grad_acc", B=B, like_grad=P["mom"])
        assert said(E, f"{nxt} must not alias like_grad_acc", B=B, like_grad=P["next"]) and said(E, "scale_rows must not alias like_grad_acc", B=B, like_grad=P["scale"])
        assert said(E, "like_u_acc must not alias energy_g", B=B, like_u=P["energy"]) and said(E, "kin0 must not alias like_u_acc", B=B, like_u=P["kin0"])
        assert said(E, "beta_rows must not alias like_u_acc", B=B, like_u=P["beta"])
        assert said(E, "beta_next must not alias uniform", B=B, **dict(annealing, beta_next=P["uniform"]))
        assert said(E, "beta_rows must not alias beta_next", B=B, **dict(annealing, beta_next=P["beta"]))
        assert said(E, "log_w must not alias noise", B=B, **dict(annealing, log_w=P["noise"]))
        assert said(E, "like_u_acc must not alias log_w", B=B, **dict(annealing, log_w=P["like_u"]))
        assert said(E, f"{acc_name} must not alias log_w", B=B, **dict(annealing, log_w=P["p_acc"]))
        assert said(E, "mean_rows must not alias log_w", B=B, **dict(folding, **dict(annealing, flags=FOLD | ANNEAL, log_w=P["mean"])))
        # the metric call's rules, word for word (a sample: the whole table is tests/test_hmc_metric_cpu.py's)
        assert said(E, "flags: LSNF_HMC_INIT and LSNF_HMC_INNER exclude each other", B=B, flags=INIT | INNER, noise=None, uniform=None)
        assert said(E, "flags: LSNF_HMC_ADAPT goes with an end call (neither LSNF_HMC_INIT nor LSNF_HMC_INNER)", B=B, **dict(adapting, flags=ADAPT | INIT))
        assert said(E, "flags: LSNF_HMC_METRIC_CLOSE goes with LSNF_HMC_METRIC_FOLD", B=B, **dict(annealing, flags=CLOSE | ANNEAL))
        assert said(E, "mean_rows, m2_rows, count_rows and reg must be NULL without LSNF_HMC_METRIC_FOLD", B=B, **dict(annealing, mean=P["mean"]))
        assert said(E, "pass either a uniform tensor or an rng, not both", B=B, noise=None, rng=Rng(1, 0, None, 0))
        assert said(E, "scale_rows must not alias grad_g", B=B, scale=P["grad_g"]) and said(E, f"{nxt} must not alias mom", B=B, mom=P["next"])
    assert call(nz=130) == LSNF_E_GEOMETRY and call(nz=130, B=0) == LSNF_E_GEOMETRY and said(E, "B=-1 out of range", B=-1)
    # an empty batch: nothing to launch, NULL pointers allowed, in every phase, annealing or not
    nulls = {k: None for k in P}
    assert call(B=0, **nulls) == LSNF_OK and call(B=0, **dict(nulls, flags=INNER)) == LSNF_OK and call(B=0, **dict(nulls, flags=INIT)) == LSNF_OK
    assert call(B=0, **dict(nulls, flags=ANNEAL)) == LSNF_OK and call(B=0, **dict(nulls, flags=ANNEAL | INIT)) == LSNF_OK
    assert call(B=0, **dict(nulls, flags=ANNEAL | FOLD | CLOSE | ADAPT, reg=reg, da=da)) == LSNF_OK
    assert call(B=0, **annealing) == LSNF_OK and call(B=0, **{"next": P["point"]}) == LSNF_OK
    # the pointers of a non-empty call
    for extra in (dict(), inner, dict(flags=INIT, uniform=None), annealing, dict(annealing, flags=ANNEAL | INIT, uniform=None), folding):
        assert said(E, "beta_rows is required (NULL)", **dict(extra, beta=None))
        assert said(E, "like_grad_acc is required (NULL)", **dict(extra, like_grad=None))
        assert said(E, "like_u_acc is required (NULL)", **dict(extra, like_u=None))
        assert said(E, "scale_rows is required (NULL)", **dict(extra, scale=None))
    both = "beta_next and log_w are required with LSNF_HMC_ANNEAL"
    for k in ("beta_next", "log_w"):
        assert said(E, both, **dict(annealing, **{k: None})) and said(E, both, **dict(annealing, flags=ANNEAL | INIT, uniform=None, **{k: None}))
    assert said(E, both, flags=ANNEAL)
    off4 = lambda k: ctypes.c_void_p(P[k].value + 4)
    assert said(E, "log_w must be 8-byte aligned", **dict(annealing, log_w=off4("log_w")))
    assert said(E, "log_w must be 8-byte aligned", **dict(annealing, flags=ANNEAL | INIT, uniform=None, log_w=off4("log_w")))
    odd = ctypes.c_void_p(0xF00002)
    assert said(E, "beta_rows must be 4-byte aligned", beta=odd) and said(E, "beta_rows must be 4-byte aligned", **dict(inner, beta=odd))
    assert said(E, "like_grad_acc must be 4-byte aligned", like_grad=odd) and said(E, "like_u_acc must be 4-byte aligned", like_u=odd)
    assert said(E, "beta_next must be 4-byte aligned", **dict(annealing, beta_next=odd))
    assert said(E, "uniform is required without an rng (unless LSNF_HMC_INIT or LSNF_HMC_INNER)", **dict(annealing, uniform=None))
    assert said(E, f"{nxt} is required (NULL) with LSNF_HMC_INNER", **dict(inner, **{"next": None}))
    # (the next rule -- a misaligned act_saved -- is what refuses a call that passed all others; 4 bytes off a 16-byte boundary is
    # allowed for four of the arrays, 8 bytes off for log_w)
    bad_act = ctypes.c_void_p(0x50008)
    all_on = dict(adapting, **dict(folding, **dict(annealing, flags=ADAPT | LAST | FOLD | CLOSE | ANNEAL)))
    for ok in (dict(), annealing, dict(annealing, flags=ANNEAL | INIT, uniform=None), dict(annealing, noise=None, **{"next": None}), inner, all_on,
               dict(annealing, noise=None, uniform=None, rng=Rng(1, 0, None, 0)),
               dict(annealing, beta=off4("beta"), beta_next=off4("beta_next"), like_grad=off4("like_grad"), like_u=off4("like_u"),
                    log_w=ctypes.c_void_p(P["log_w"].value + 8))):
        assert said(E, "act_saved must be 16-byte aligned", **dict(ok, act=bad_act))


def test_the_older_entry_points_still_refuse_the_new_bit():
    """Nothing about lsnf_hmc_step_metric / lsnf_hmc_step_rows changed: bit 0x40 is unknown there."""
    lib = lsnf_amd.load_library()
    for name, n_ptr, extra in (("lsnf_hmc_step_metric", 14, 5), ("lsnf_reverse_hmc_step_metric", 12, 5), ("lsnf_hmc_step_rows", 14, 0),
                               ("lsnf_reverse_hmc_step_rows", 12, 0)):
        fn = getattr(lib, name)
        head = [FAKE[0], 128, 64, 5, 1, 4] + FAKE[1:1 + n_ptr]
        tail = [None, FAKE[20], None, None] + ([FAKE[21], None, None, None, None] if extra else [])
        rc = fn(*head, *tail, ANNEAL, FAKE[22], None, None, None)
        assert rc == LSNF_E_ARG and lib.lsnf_last_error().decode() == name + ": unknown flag bits 0x40"


# ---- the Python wrappers and the samplers on CPU tensors ----------------------------------------------------------------------------
def test_python_wrappers_speak_on_cpu_tensors(monkeypatch):
    from counting_lib import install
    F, L = lsnf_amd.flow, lsnf_amd.langevin
    lib = lsnf_amd.load_library()
    plan = _plan()
    stand = install(monkeypatch, lsnf_amd)
    seen = []
    real = lsnf_amd.mcmc._check_chain

    def spy(*a, **k):
        seen.append(k.get("stash"))
        return real(*a, **k)
    monkeypatch.setattr(lsnf_amd.mcmc, "_check_chain", spy)
    z, saved = torch.zeros(5, 8), torch.zeros(1, 5, 8)
    act = torch.zeros(lib.lsnf_act_saved_floats(8, 4, 2, 5))
    steps, state, metric = F.new_hmc_row_steps(5, "cpu", 0.5), F.new_hmc_state(plan, 5, "cpu"), F.new_hmc_row_metric(plan, 5, "cpu")
    temper, nxt = F.new_hmc_row_temper(plan, 5, "cpu"), torch.full((5,), 0.25)
    zcall = lambda temper=temper, **kw: F.hmc_step_tempered(plan, z, None, None, state, F.PhiloxNoise(3), steps, metric, temper, **kw)
    ecall = lambda temper=temper, **kw: F.reverse_hmc_step_tempered(plan, z, saved, act, None, None, state, F.PhiloxNoise(3), steps, metric, temper,
                                                                    **kw)
    for call in (zcall, ecall):
        n = len(seen)
        with pytest.raises(lsnf_amd.LsnfError, match="phase must be one of"):
            call(phase="middle")
        with pytest.raises(lsnf_amd.LsnfError, match=r"temper must be a flow.HmcRowTemper \(new_hmc_row_temper\(\)\)"):
            call(temper=torch.ones(5))
        with pytest.raises(lsnf_amd.LsnfError, match="anneal must be None or a"):
            call(anneal=0.5)
        with pytest.raises(lsnf_amd.LsnfError, match="anneal goes with phase='init' or 'end'"):
            call(phase="inner", anneal=nxt)
        with pytest.raises(lsnf_amd.LsnfError, match="window must be None, 'fold' or 'close'"):
            call(window="open", anneal=nxt)
        assert len(seen) == n                                # (refused before the tensors are looked at)
        for kw in (dict(), dict(anneal=nxt), dict(anneal=nxt, window="close", adapt="update"), dict(anneal=nxt, propose=False),
                   dict(phase="init", anneal=nxt)):
            with pytest.raises(lsnf_amd.LsnfError, match="no CPU path"):
                call(**kw)
        assert len(seen) == n + 5                            # every such call went through _check_chain
    assert all(st is None for st in seen[:5]) and all(st is not None and st[0] is saved and st[1] is act for st in seen[5:])
    # the arrays of `temper` and the next temperatures go through the one checking path, in the order of the C call's arguments
    with pytest.raises(lsnf_amd.LsnfError, match="temper.beta must live on"):
        lsnf_amd.mcmc._row_temper_args(plan, temper, 5, torch.device("cuda:0"), None)
    names = []
    with monkeypatch.context() as m:
        m.setattr(lsnf_amd.mcmc, "_check_out", lambda t, name, need, dev, *a, **k: names.append((name, need)))
        m.setattr(lsnf_amd.mcmc, "_check_in", lambda t, name, need, dev, *a, **k: names.append((name, need)))
        for anneal in (None, nxt):
            args = lsnf_amd.mcmc._row_temper_args(plan, temper, 5, torch.device("cpu"), anneal)
            assert len(args) == 5 and args[0] == temper.beta.data_ptr() and args[2] == temper.like_grad.data_ptr() and args[3] == temper.like_energy.data_ptr()
            assert (args[1], args[4]) == ((None, None) if anneal is None else (nxt.data_ptr(), temper.log_w.data_ptr()))
    assert names == [("temper.beta", 5), ("anneal", 5), ("temper.like_grad", 40), ("temper.like_energy", 5), ("temper.log_w", 10)] * 2
    with monkeypatch.context() as m:                         # (past the buffers' rule, which speaks first on CPU tensors)
        m.setattr(lsnf_amd.mcmc, "_check_out", lambda *a, **k: None)
        with pytest.raises(lsnf_amd.LsnfError, match="anneal has 4 elements, the kernel reads 5"):
            lsnf_amd.mcmc._row_temper_args(plan, temper, 5, torch.device("cpu"), nxt[:4])
        with pytest.raises(lsnf_amd.LsnfError, match="anneal must live on the GPU"):      # (a float64 one: through `_need_cuda`)
            lsnf_amd.mcmc._row_temper_args(plan, temper, 5, torch.device("cpu"), nxt.double())
    M = lsnf_amd.mcmc
    flags = lambda phase, adapt, window, anneal: (M._row_step_mode(steps, phase, adapt) | M._row_metric_mode(metric, phase, window) |
                                                  M._row_temper_mode(temper, phase, anneal))
    assert flags("init", None, None, nxt) == INIT | ANNEAL and flags("end", "last", "close", nxt) == ADAPT | LAST | FOLD | CLOSE | ANNEAL
    assert flags("end", None, None, None) == 0 and flags("inner", None, None, None) == INNER
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    with pytest.raises(lsnf_amd.LsnfError):
        net.hmc_step_tempered(z, None, None, state, F.PhiloxNoise(1), steps, metric, temper, phase="init", anneal=nxt)
    with pytest.raises(lsnf_amd.LsnfError):
        net.reverse_hmc_step_tempered(z, saved, act, None, None, state, F.PhiloxNoise(1), steps, metric, temper, phase="init", anneal=nxt)
    # the samplers: their own rules, then the wrappers'; nothing to do returns without a launch
    x, G = torch.zeros(2, 8), torch.nn.Flatten()
    kw = dict(chains=3, g_l_step_size=0.5, g_llhd_sigma=0.3)
    for fn in (L.estimate_log_px_ais_z_with_flow, L.estimate_log_px_ais_eps_with_flow):
        with pytest.raises(ValueError, match="leapfrog_steps"):
            fn(x, G, net, betas=[0.0, 1.0], leapfrog_steps=0, philox=F.PhiloxNoise(1), **kw)
        with pytest.raises(ValueError, match="chains"):
            fn(x, G, net, betas=[0.0, 1.0], leapfrog_steps=2, philox=F.PhiloxNoise(1), **dict(kw, chains=0))
        with pytest.raises(ValueError, match="betas must start at 0"):
            fn(x, G, net, betas=[0.1, 1.0], leapfrog_steps=2, philox=F.PhiloxNoise(1), **kw)
        with pytest.raises(ValueError, match="must not decrease"):
            fn(x, G, net, betas=[0.0, 0.6, 0.5, 1.0], leapfrog_steps=2, philox=F.PhiloxNoise(1), **kw)
        with pytest.raises(lsnf_amd.LsnfError, match="metric must be a flow.HmcRowMetric"):
            fn(x, G, net, betas=[0.0, 1.0], leapfrog_steps=2, philox=F.PhiloxNoise(1), metric=1.0, **kw)
        with pytest.raises(lsnf_amd.LsnfError, match="steps must be a flow.HmcRowSteps"):
            fn(x, G, net, betas=[0.0, 1.0], leapfrog_steps=2, philox=F.PhiloxNoise(1), steps=0.5, **kw)
        with pytest.raises(lsnf_amd.LsnfError):              # (the sample's launch is refused: the module lives on the CPU)
            fn(x, G, net, betas=[0.0, 1.0], leapfrog_steps=2, philox=F.PhiloxNoise(1), **kw)
        ph = F.PhiloxNoise(5, 100)
        assert fn(x, G, net, betas=[0.0], leapfrog_steps=2, philox=ph, **kw) == (None,) * 6
        empty = fn(x[:0], G, net, betas=[0.0, 0.5, 1.0], leapfrog_steps=2, philox=ph, **kw)
        assert empty[0].shape == (0,) and empty[0].dtype == torch.float64 and empty[1].shape == (0, 3) and empty[2].shape == (0,)
        assert all(t is None for t in empty[3:]) and ph.offset == 100
    assert stand.launching() == [], dict(stand.entered)


class _FakeNet:
    """What a sampler asks of netF, recording every call: `sample`, the two tempered steps and `_plan`."""

    def __init__(self, plan, log):
        self.plan, self.log = plan, log

    def _plan(self):
        return self.plan

    def sample(self, n, philox, temperature=1.0, return_eps=False, return_log_prob=False):
        self.log.append(("sample", philox.offset, n, return_eps))
        g = torch.Generator().manual_seed(0)
        return torch.randn(n, 8, generator=g), torch.randn(n, 8, generator=g)

    def _step(self, name, point, state, noise, steps, metric, temper, kw):
        F = lsnf_amd.flow
        assert isinstance(steps, F.HmcRowSteps) and isinstance(metric, F.HmcRowMetric) and isinstance(temper, F.HmcRowTemper)
        assert kw["inplace"] and kw["reuse_buffers"] and kw.get("window") is None
        anneal = kw.get("anneal")
        if anneal is not None:
            assert anneal.dtype == torch.float32 and anneal.shape == (point.shape[0],) and anneal.is_contiguous() and bool((anneal == anneal[0]).all())
        self.log.append((name, kw["phase"], None if noise is None else noise.offset, kw["propose"], kw.get("adapt"),
                         None if anneal is None else float(anneal[0])))
        acc = None if kw["phase"] == "inner" else torch.ones(point.shape[0])
        return None, acc, None

    def hmc_step_tempered(self, z_prop, grad_g, energy_g, state, noise, steps, metric, temper, **kw):
        assert grad_g.shape == z_prop.shape and energy_g.shape == (z_prop.shape[0],)
        return self._step("z", z_prop, state, noise, steps, metric, temper, kw) + (None,)

    def reverse_hmc_step_tempered(self, eps_prop, z_saved, act_saved, grad_g, energy_g, state, noise, steps, metric, temper, **kw):
        assert grad_g.shape == eps_prop.shape and energy_g.shape == (eps_prop.shape[0],)
        return self._step("eps", eps_prop, state, noise, steps, metric, temper, kw)


@pytest.mark.parametrize("space", R.SPACES)
@pytest.mark.parametrize("adapt", (False, True))
def test_a_sampler_is_the_exact_sequence_of_calls(monkeypatch, space, adapt):
    """K = 3 temperatures' trajectories of L = 2 steps: one sample at offset 0, one init call annealing to beta_1, then per trajectory
    one inner call and one end call; flags and Philox offsets of each."""
    F, Lv, M = lsnf_amd.flow, lsnf_amd.langevin, lsnf_amd.mcmc
    plan, log = _plan(), []
    net = _FakeNet(plan, log)
    monkeypatch.setattr(F, "reverse_keep_supported", lambda plan, B: True)
    monkeypatch.setattr(F, "reverse", lambda plan, eps, obj, **kw: (eps.clone(), None, None) if kw.get("save_for_backward") else (eps.clone(), None))
    N, C, T, Ls = 2, 3, 3, 2
    x, G = torch.zeros(N, 8), torch.nn.Flatten()
    betas = Lv.ais_schedule(T, "linear")
    ph = F.PhiloxNoise(9, 40)
    fn = Lv.estimate_log_px_ais_z_with_flow if space == "z" else Lv.estimate_log_px_ais_eps_with_flow
    log_px, log_w, ess, rate, z_T, temper = fn(x, G, net, betas=betas, chains=C, leapfrog_steps=Ls, g_l_step_size=0.5, g_llhd_sigma=1.0, philox=ph,
                                               adapt=adapt)
    up = "update" if adapt else None
    third = float(torch.tensor(1.0 / 3.0, dtype=torch.float64).float()), float(torch.tensor(2.0 / 3.0, dtype=torch.float64).float())
    assert log == [("sample", 40, N * C, True),
                   (space, "init", 41, True, None, third[0]),
                   (space, "inner", None, True, None, None), (space, "end", 42, True, up, third[1]),
                   (space, "inner", None, True, None, None), (space, "end", 43, True, up, 1.0),
                   (space, "inner", None, True, None, None), (space, "end", 44, False, up, None)]
    assert ph.offset == 40 + T + 1 and all(e[2] != 40 for e in log[1:])      # offset 0 is the sample's alone
    steps, metric = F.new_hmc_row_steps(N * C, "cpu", 0.5), F.new_hmc_row_metric(plan, N * C, "cpu")
    nxt = torch.zeros(N * C)
    flags = [M._row_step_mode(steps, e[1], e[4]) | M._row_metric_mode(metric, e[1], None) | M._row_temper_mode(temper, e[1], None if e[5] is None else nxt)
             for e in log[1:]]
    a = ADAPT if adapt else 0
    assert flags == [INIT | ANNEAL, INNER, a | ANNEAL, INNER, a | ANNEAL, INNER, a]
    # the reduction: float64, (N, chains); with zero weights log_px is the Gaussian normaliser alone and every chain counts
    assert log_px.dtype == log_w.dtype == ess.dtype == torch.float64 and log_px.shape == (N,) and log_w.shape == (N, C) and ess.shape == (N,)
    assert bool(((log_px + 0.5 * 8 * math.log(2.0 * math.pi)).abs() <= 1e-12).all()) and bool(((ess - C).abs() <= 1e-12).all())
    assert rate.shape == (N * C,) and bool((rate == 1.0).all()) and z_T.shape == (N * C, 8, 1, 1) and isinstance(temper, F.HmcRowTemper)
    temper.log_w[:, 0] = torch.tensor([0.0, 1.0, 2.0, -1.0, -1.0, -1.0]); temper.log_w[:, 1] = 0.25
    lp, lw, es = Lv._ais_reduce(temper, N, C, 8, 2.0)
    want = torch.tensor([[-0.25, 0.75, 1.75], [-1.25, -1.25, -1.25]], dtype=torch.float64)
    assert torch.equal(lw, want)
    const = math.log(C) + 4.0 * math.log(2.0 * math.pi * 4.0)
    assert bool(((lp - (torch.logsumexp(want, 1) - const)).abs() <= 1e-12).all())
    w = torch.exp(want)
    assert bool(((es - w.sum(1) ** 2 / (w * w).sum(1)).abs() <= 1e-12).all()) and abs(es[1].item() - C) <= 1e-12


# ---- the schedule ---------------------------------------------------------------------------------------------------------------
def test_ais_schedule():
    S = lsnf_amd.langevin.ais_schedule
    for T in (1, 2, 7, 100, 1000):
        for kind in ("sigmoid", "linear"):
            b = S(T, kind)
            assert b.dtype == torch.float64 and b.shape == (T + 1,) and b[0].item() == 0.0 and b[-1].item() == 1.0
            assert bool((b[1:] >= b[:-1]).all()) and bool(((b + b.flip(0) - 1.0).abs() <= 1e-15).all())      # nondecreasing, symmetric
            assert bool(((b - A.schedule(T, kind)).abs() <= 1e-15).all())
    assert torch.equal(S(4, "linear"), torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0], dtype=torch.float64))
    b = S(100)
    sg = lambda v: 1.0 / (1.0 + math.exp(-v))
    assert abs(b[25].item() - (sg(-2.0) - sg(-4.0)) / (sg(4.0) - sg(-4.0))) <= 1e-15 and b[50].item() == 0.5
    d = b[1:] - b[:-1]
    assert d[0] < 0.25 * d[49] and d[-1] < 0.25 * d[49]       # Wu et al.'s: the steps are spent near both ends
    assert bool(((S(50, delta=1e-3) - S(50, "linear")).abs() <= 1e-6).all())
    for bad in (0, -3):
        with pytest.raises(ValueError):
            S(bad)
    with pytest.raises(ValueError):
        S(5, "cosine")


# ---- the restatements alone ------------------------------------------------------------------------------------------------------
def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _setup(B=24, seed=5, T=3):
    import hmc_restated as H
    from oracle import flow_oracle as O
    nz = 8
    p = O.init_params(nz, 4, 5, seed=3)
    quad = H.Quadratic(nz, 0.1, seed=7 + nz)
    g = torch.Generator().manual_seed(seed)
    z0, _ = O.smooth_batch(p, B, nz, seed=1000 + seed)
    noises = [torch.randn(B, nz, generator=g, dtype=torch.float64) for _ in range(T)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g, dtype=torch.float64).clamp_min(2.0 ** -25) for _ in range(T)]
    return p, quad, z0.double(), noises, uniforms, g


@pytest.mark.parametrize("space", R.SPACES)
def test_a_constant_unit_temperature_is_the_metric_chain(space):
    p, quad, z0, noises, uniforms, g = _setup()
    B, L = z0.shape[0], 3
    sd = torch.exp2(2.0 * torch.rand(B, 8, generator=g, dtype=torch.float64) - 1.0)
    step = torch.full((B,), 0.6, dtype=torch.float64)
    clone = lambda xs: [None if x is None else x.clone() for x in xs]
    ref = MR.chain(MR.flow_potential(space, p, quad), z0, step, sd, L, clone(noises), uniforms)
    got = TR.chain(TR.flow_parts(space, p, quad), z0, step, sd, L, clone(noises), uniforms, torch.ones(B, dtype=torch.float64))
    assert same(got.la, ref.la) and torch.equal(got.acc, ref.acc) and same(got.states, ref.states) and 0 < int(got.acc.sum()) < got.acc.numel()
    assert all(same(a, b) for a, b in zip(got.state[:3], ref.state)) and not got.weights.any() and bool((got.beta == 1.0).all())
    # another temperature is another chain; beta = 0 is the prior's: the likelihood's parts are kept and do not enter
    cold = TR.chain(TR.flow_parts(space, p, quad), z0, step, sd, L, clone(noises), uniforms, torch.zeros(B, dtype=torch.float64))
    prior = MR.chain(MR.flow_potential(space, p, None), z0, step, sd, L, clone(noises), uniforms) if space == "z" else None
    assert not same(cold.la, ref.la)
    if prior is not None:
        assert same(cold.la, prior.la) and same(cold.states, prior.states)
    assert cold.state[4].abs().min() > 0 and cold.state[3].abs().max() > 0


@pytest.mark.parametrize("space", R.SPACES)
def test_the_retempered_state_is_a_fresh_evaluation_at_the_next_temperature(space):
    p, quad, z0, noises, uniforms, g = _setup(T=4)
    B, L = z0.shape[0], 2
    f64 = torch.float64
    beta0 = torch.rand(B, generator=g, dtype=f64)
    anneals = [None] + [torch.rand(B, generator=g, dtype=f64) * 1.5 for _ in range(3)] + [None]
    step, sd = torch.full((B,), 0.5, dtype=f64), torch.ones(B, 8, dtype=f64)
    clone = lambda xs: [None if x is None else x.clone() for x in xs]
    parts = TR.flow_parts(space, p, quad)
    for K in (1, 2, 3):                                      # stop after end call K's anneal: the kept state is the one at anneals[K]
        tr = TR.chain(parts, z0, step, sd, L, clone(noises[:K]) + [None], uniforms[:K + 1], beta0, anneals[:K + 1])
        x, gk, uk, gl, el = tr.state
        P = parts(x)
        U, G = TR.tempered(P, anneals[K])
        assert same(tr.beta, anneals[K]) and same(P.el, el) and same(P.gl, gl)
        assert bool(((uk - U).abs() <= 1e-12 * (1.0 + U.abs())).all()) and bool(((gk - G).abs() <= 1e-12 * (1.0 + G.abs())).all())
    # the weight: the sum over the anneals of -(beta' - beta) el(state), state by state
    tr = TR.chain(parts, z0, step, sd, L, clone(noises[:3]) + [None], uniforms[:4], beta0, anneals[:4])
    betas = [beta0, anneals[1], anneals[2], anneals[3]]
    want = sum(-(betas[k + 1] - betas[k]) * parts(tr.states[k]).el for k in range(3))
    assert bool(((tr.weights[-1] - want).abs() <= 1e-12 * (1.0 + want.abs())).all()) and 0 < int(tr.acc.sum()) < tr.acc.numel()
    # the fp32 lines: Kahan's pair carries what a plain fp32 sum loses
    f32 = torch.float32
    el32 = (100.0 * torch.rand(4000, generator=g)).to(f32)
    d = torch.full((1,), 1e-3, dtype=f32)
    w, c, plain = torch.zeros(1, dtype=f32), torch.zeros(1, dtype=f32), torch.zeros(1, dtype=f32)
    for e in el32:
        w, c = TR.weigh(w, c, d, e.reshape(1))
        plain = plain + (-(d * e.reshape(1)))
    exact = -(d.double() * el32.double()).sum()
    assert w.dtype == f32 and abs((w.double() - c.double()).item() - exact.item()) <= 1e-7 * (d.double() * el32.double()).sum().item()
    assert abs(plain.double().item() - exact.item()) > 10 * abs((w.double() - c.double()).item() - exact.item())


def test_the_closed_form_and_plain_importance_sampling():
    p = A.affine_flow()
    quads = [A.datum(s) for s in A.EXP_DATA]
    assert abs(A.closed_form(p, quads[0]) - (-7.8267)) <= 5e-5
    W, b, m, S = A.prior_gaussian(p)
    assert bool(((S - S.T).abs() <= 1e-14).all()) and bool((torch.linalg.eigvalsh(S) > 0).all())
    # the closed form against brute force: plain importance sampling from the Gaussian prior with 2 x 10^5 draws
    g = torch.Generator().manual_seed(0)
    n = 200000
    z, eps = A.prior_draws(p, "z", n, g)
    assert bool(((z.mean(0) - m).abs() <= 5.0 * torch.sqrt(torch.diag(S) / n)).all())
    for q in quads:
        e = q(z)[0]
        est = (torch.logsumexp(-e, 0) - math.log(n)).item()
        assert abs(est - A.closed_form(p, q)) <= 0.05, (est, A.closed_form(p, q))
    # T = 1 IS plain importance sampling: the init call weighs the start with the whole energy, log_w = -E(z_0) exactly, and the one
    # trajectory that follows does not touch the weight
    for space in R.SPACES:
        C = 16
        logz, ess, acc, tr = A.run(p, quads, space, A.schedule(1), 3, C, A.EXP_STEP, seed=3)
        g = torch.Generator().manual_seed(5000 + 3)
        x0, _ = A.prior_draws(p, space, 2 * C, g)
        e0 = TR.parts(space, p, x0, A.Stacked(quads, C)).el
        assert same(tr.weights[0], -e0) and same(tr.weights[-1], -e0) and same(logz, torch.logsumexp((-e0).view(2, C), 1) - math.log(C))
        assert bool((tr.beta == 1.0).all())


@pytest.mark.parametrize("space", R.SPACES)
def test_the_estimator_finds_the_closed_form(space):
    seed = 11                                                # (a seed that is not one of those the bands were taken from)
    err, ess, acc = A.experiment(seed, space)
    band = BAND[space]
    print(f"[ais] {space}: T={A.EXP_T}, L={A.EXP_L}, {A.EXP_CHAINS} chains, step {A.EXP_STEP}: errors log Z_hat - closed form "
          + " ".join(f"{e:+.4f}" for e in err.tolist()) + f" (band {band['error']}), ess " + " ".join(f"{e:.2f}" for e in ess.tolist())
          + f" (band {band['ess']}), mean acceptance {acc:.4f} (band {band['accept']})")
    assert A.BAND[space] == band
    assert band["error"][0] < 0.0 < band["error"][1]         # the condition on the estimator: the closed form lies inside the band
    assert bool(((err >= band["error"][0]) & (err <= band["error"][1])).all())
    assert bool(((ess >= band["ess"][0]) & (ess <= band["ess"][1])).all())
    assert band["accept"][0] <= acc <= band["accept"][1]


def test_cost_tool_is_a_driver_on_the_ab_harness():
    """tools/hmc_tempered_vs_hmc_metric.py: its child's source is valid and importing the driver does not import torch."""
    import subprocess
    import sys
    tools = os.path.join(ROOT, "tools")
    code = ("import sys; sys.path.insert(0, %r)\nimport ab_harness, hmc_tempered_vs_hmc_metric as t\n"
            "compile(ab_harness.PRELUDE + t.CHILD, 'child', 'exec')\nassert 'torch' not in sys.modules\n"
            "assert t.SIZES == (100, 16384)" % tools)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=60)

"""CPU: the schedule search of the annealing HMC calls (`lsnf_hmc_step_schedule`, `lsnf_reverse_hmc_step_schedule`,
include/lsnf_flow_mcmc.h): the C declarations and the ctypes binding outside the core ABI, the Python layers, every refusal the search
adds pinned through the entry points' own check before any HIP call (fake aligned pointers that are never dereferenced, as
tests/test_hmc_resample_cpu.py), the restated search (tests/hmc_schedule_restated.py) on hand-made groups, and its fp32 form against
the float64 root of cess64(delta) = target within the bound derived in that helper's docstring."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
import hmc_schedule_restated as S

import lsnf_amd

LSNF_OK, LSNF_E_ARG = 0, -1
INIT, INNER, ADAPT, LAST, FOLD, CLOSE, ANNEAL, SWAP, ODD, RESAMPLE, SCHEDULE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024
NAMES = ("lsnf_hmc_step_schedule", "lsnf_reverse_hmc_step_schedule")
RESAMPLING = {"lsnf_hmc_step_schedule": "lsnf_hmc_step_resample", "lsnf_reverse_hmc_step_schedule": "lsnf_reverse_hmc_step_resample"}
COUNT = {"lsnf_hmc_step_schedule": 46, "lsnf_reverse_hmc_step_schedule": 44}
TWO = ["cess_frac", "min_step"]
FAKE = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(40)]     # 16-byte aligned addresses that are never dereferenced on the host


def test_symbols_are_declared_exported_and_bound_outside_the_core_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow_mcmc.h")).read(), flags=re.S)
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    ext = lsnf_amd._lib._EXT_SIGNATURES
    assert len(re.findall(r"#define\s+LSNF_HMC_SCHEDULE\s+1024u", hdr)) == 1
    decl = lambda name: [re.sub(r".*[\s*]", "", a.strip())
                         for a in re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1).split(",")]
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and name not in core and hasattr(lib, name)
        assert name in ext and len(ext[name][1]) == COUNT[name] and name not in lsnf_amd.exported_symbols() and name not in lsnf_amd._lib._SIGNATURES
        assert getattr(lib, name).argtypes == ext[name][1]               # attached in load()
        names, resampling = decl(name), decl(RESAMPLING[name])
        assert resampling[-1] == "stream" and resampling[-2] == "ess_out"
        assert names == resampling[:-1] + TWO + ["stream"] and len(names) == COUNT[name]
        args, rargs = ext[name][1], ext[RESAMPLING[name]][1]
        assert args[:len(rargs) - 1] == rargs[:-1] and args[-1] == rargs[-1] and args[-3:-1] == [ctypes.c_float, ctypes.c_float]
        assert len(rargs) == COUNT[name] - 2                 # the resampling declarations are what they were
    assert lsnf_amd._lib.extension_symbols() == sorted(ext)
    assert lib.lsnf_abi_version() == 5 and lsnf_amd._lib.ABI_VERSION == 5
    # the header states the search line by line
    text = open(os.path.join(ROOT, "include", "lsnf_flow_mcmc.h")).read()
    for said in ("b = beta_rows[rung 0];  cap = beta_next[rung 0];  D = cap - b", "W_i = expf(l_i - m);  S0 = tree + W_i",
                 "emin = tree fminf el_s_i;  r_i = el_s_i - emin", "cess = (N1 * N1) / (N2 * S0)", "mid = 0.5f * (lo + hi)",
                 "delta = fmaxf(lo, min_step);  beta' = fminf(b + delta, cap)", "the caller keeps both equal on the rows of a group",
                 "t1_i = x_i o x_{i^1}"):
        assert said in text, said


def test_python_layers_exist():
    F, L, M = lsnf_amd.flow, lsnf_amd.langevin, lsnf_amd.mcmc
    assert F.hmc_step_schedule is M.hmc_step_schedule and F.reverse_hmc_step_schedule is M.reverse_hmc_step_schedule
    assert F.HMC_SCHEDULE == M.HMC_SCHEDULE == 1024
    new = ["schedule", "cess_target", "min_step"]
    for fn, old in ((F.hmc_step_schedule, F.hmc_step_resample), (F.reverse_hmc_step_schedule, F.reverse_hmc_step_resample),
                    (lsnf_amd._netF.hmc_step_schedule, lsnf_amd._netF.hmc_step_resample),
                    (lsnf_amd._netF.reverse_hmc_step_schedule, lsnf_amd._netF.reverse_hmc_step_resample)):
        a, b = inspect.signature(fn).parameters, inspect.signature(old).parameters
        assert [n for n in a] == [n for n in b] + new
        for n in new:
            assert a[n].kind is inspect.Parameter.KEYWORD_ONLY
        assert a["schedule"].default is None and a["cess_target"].default == 0.95 and a["min_step"].default == 0.0
        for n in b:
            assert a[n].kind == b[n].kind and a[n].default == b[n].default
    for fn in (L.estimate_log_px_smc_adaptive_z_with_flow, L.estimate_log_px_smc_adaptive_eps_with_flow):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["x", "netG", "netF", "max_steps", "chains", "particles", "leapfrog_steps", "g_l_step_size",
                                        "g_llhd_sigma", "philox", "cess_target", "ess_threshold", "min_step", "check_every", "steps", "metric",
                                        "return_schedule"]
        for kw in list(sig.parameters)[3:]:
            assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
        d = {k: v.default for k, v in sig.parameters.items()}
        assert (d["cess_target"], d["ess_threshold"], d["min_step"], d["check_every"], d["steps"], d["metric"], d["return_schedule"]) == \
            (0.95, 0.5, None, 0, None, None, False)
        for said in ("consistent", "no longer exactly", "unbiased", "Beskos", "only host synchronisation", "1 / (4 max_steps)", "`resampled`",
                     "`steps_used`"):
            assert said in fn.__doc__, said
    # the resampling layer keeps its signatures
    assert list(inspect.signature(F.hmc_step_resample).parameters)[-1] == "resample_uniform"
    assert len(lsnf_amd._lib._EXT_SIGNATURES["lsnf_hmc_step_resample"][1]) == 44


# ---- the refusals of the two entry points ------------------------------------------------------------------------------------
Z_ARGS = ("plan", "point", "z_out", "saved", "act", "ll", "grad_g", "energy", "p_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")
E_ARGS = ("plan", "point", "saved", "act", "grad_g", "energy", "p_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")


def _caller(lib, name):
    Rng, Da, Reg = lsnf_amd._lib.LsnfRng, lsnf_amd._lib.LsnfDualAvg, lsnf_amd._lib.LsnfMetricReg
    order = Z_ARGS if name == "lsnf_hmc_step_schedule" else E_ARGS
    ptrs = dict(zip(order + ("step_rows", "adapt", "scale", "mean", "m2", "count", "beta", "beta_next", "like_grad", "like_u", "log_w", "next",
                             "accept", "la", "resample_uniform", "ancestor_out", "ess_out"), FAKE))
    base = dict(ptrs, nz=128, w=64, d=5, c=1, B=16, rng=None, da=None, adapt=None, mean=None, m2=None, count=None, reg=None, beta_next=None,
                log_w=None, flags=0, accept=None, la=None, group=0, ess_frac=0.5, resample_uniform=None, ancestor_out=None, ess_out=None,
                cess_frac=0.95, min_step=0.0)
    fn = getattr(lib, name)

    def call(**kw):
        a = dict(base, **kw)
        return fn(a["plan"], a["nz"], a["w"], a["d"], a["c"], a["B"], *(a[k] for k in order[1:]),
                  None if a["rng"] is None else ctypes.byref(a["rng"]), a["step_rows"], a["adapt"],
                  None if a["da"] is None else ctypes.byref(a["da"]), a["scale"], a["mean"], a["m2"], a["count"],
                  None if a["reg"] is None else ctypes.byref(a["reg"]), a["beta"], a["beta_next"], a["like_grad"], a["like_u"], a["log_w"],
                  a["flags"], a["next"], a["accept"], a["la"], a["group"], a["ess_frac"], a["resample_uniform"], a["ancestor_out"],
                  a["ess_out"], a["cess_frac"], a["min_step"], None)

    def said(code, text, **kw):
        rc = call(**kw)
        got = lib.lsnf_last_error().decode()
        return rc == code and got == name + ": " + text
    return call, said, ptrs, Rng, Da, Reg


@pytest.mark.parametrize("name", NAMES)
def test_every_new_rule_refuses_before_any_hip_call(name):
    lib = lsnf_amd.load_library()
    call, said, P, Rng, Da, Reg = _caller(lib, name)
    da = Da(target_accept=0.8, gamma=0.05, t0=10.0, kappa=0.75, step_min=1e-4, step_max=1e2)
    reg = Reg(n0=5.0, var0=1e-3, scale_min=1e-3, scale_max=1e3)
    annealing = dict(beta_next=P["beta_next"], log_w=P["log_w"])
    searching = dict(flags=SCHEDULE | ANNEAL, group=4, **annealing)
    both = dict(flags=SCHEDULE | RESAMPLE | ANNEAL, group=4, resample_uniform=P["resample_uniform"], ancestor_out=P["ancestor_out"],
                ess_out=P["ess_out"], **annealing)
    folding = dict(mean=P["mean"], m2=P["m2"], count=P["count"], reg=reg)
    adapting = dict(adapt=P["adapt"], da=da)
    E = LSNF_E_ARG
    for B in (0, 16):                                        # every rule of the search precedes the empty-batch return
        assert said(E, "unknown flag bits 0x800", B=B, **dict(searching, flags=SCHEDULE | ANNEAL | 0x800))
        assert said(E, "unknown flag bits 0x80", B=B, **dict(searching, flags=SCHEDULE | ANNEAL | SWAP))
        assert said(E, "flags: LSNF_HMC_SCHEDULE goes with LSNF_HMC_INIT or an end call, not with LSNF_HMC_INNER", B=B,
                    **dict(searching, flags=SCHEDULE | INNER, noise=None, uniform=None, beta_next=None, log_w=None))
        assert said(E, "flags: LSNF_HMC_SCHEDULE goes with LSNF_HMC_ANNEAL", B=B, **dict(searching, flags=SCHEDULE, beta_next=None, log_w=None))
        assert said(E, "flags: LSNF_HMC_SCHEDULE goes with LSNF_HMC_ANNEAL", B=B,
                    **dict(searching, flags=SCHEDULE | INIT, uniform=None, beta_next=None, log_w=None))
        frozen = "flags: LSNF_HMC_SCHEDULE excludes LSNF_HMC_ADAPT, LSNF_HMC_METRIC_FOLD and LSNF_HMC_METRIC_CLOSE"
        assert said(E, frozen, B=B, **dict(searching, flags=SCHEDULE | ANNEAL | ADAPT, **adapting))
        assert said(E, frozen, B=B, **dict(searching, flags=SCHEDULE | ANNEAL | ADAPT | LAST, **adapting))
        assert said(E, frozen, B=B, **dict(searching, flags=SCHEDULE | ANNEAL | FOLD, **folding))
        assert said(E, frozen, B=B, **dict(searching, flags=SCHEDULE | ANNEAL | FOLD | CLOSE, **folding))
        for bad in (0, 1, 3, 5, 6, 12, 32, -4):
            assert said(E, f"group must be 2, 4, 8 or 16 with LSNF_HMC_SCHEDULE (got {bad})", B=B, **dict(searching, group=bad))
            assert said(E, f"group must be 2, 4, 8 or 16 with LSNF_HMC_RESAMPLE (got {bad})", B=B, **dict(both, group=bad))
        for bad, shown in ((0.0, "0"), (1.0, "1"), (-0.5, "-0.5"), (1.5, "1.5"), (float("nan"), "nan"), (float("inf"), "inf")):
            assert said(E, f"cess_frac must lie in (0, 1) with LSNF_HMC_SCHEDULE (got {shown})", B=B, **dict(searching, cess_frac=bad))
        for bad, shown in ((-1e-3, "-0.001"), (float("nan"), "nan"), (float("inf"), "inf"), (-float("inf"), "-inf")):
            assert said(E, f"min_step must be finite and not negative with LSNF_HMC_SCHEDULE (got {shown})", B=B, **dict(searching, min_step=bad))
        # RESAMPLE on INIT stays refused, with or without the search; without RESAMPLE its three pointers stay NULL
        end_only = "flags: LSNF_HMC_RESAMPLE goes with an end call (neither LSNF_HMC_INIT nor LSNF_HMC_INNER)"
        assert said(E, end_only, B=B, **dict(both, flags=SCHEDULE | RESAMPLE | ANNEAL | INIT, uniform=None))
        none = "resample_uniform, ancestor_out and ess_out must be NULL without LSNF_HMC_RESAMPLE"
        for k in ("resample_uniform", "ancestor_out", "ess_out"):
            assert said(E, none, B=B, **dict(searching, **{k: P[k]}))
        assert said(E, "beta_rows must not alias beta_next", B=B, **dict(searching, beta_next=P["beta"]))
    for B, G in ((15, 2), (18, 4), (20, 8), (24, 16), (8, 16), (1, 2)):
        assert said(E, f"B={B} is not a multiple of group={G}", B=B, **dict(searching, group=G))
        assert said(E, f"B={B} is not a multiple of group={G}", B=B, **dict(both, group=G))
    nulls = {k: None for k in P}
    assert call(B=0, **nulls) == LSNF_OK and call(B=0, **dict(nulls, flags=SCHEDULE | ANNEAL, group=8)) == LSNF_OK
    assert call(B=0, **searching) == LSNF_OK and call(B=0, **both) == LSNF_OK
    # the pointers of a non-empty call
    assert said(E, "beta_next and log_w are required with LSNF_HMC_ANNEAL", **dict(searching, log_w=None))
    assert said(E, "resample_uniform is required with LSNF_HMC_RESAMPLE when no rng is given", **dict(both, resample_uniform=None))
    # (the next rule -- a misaligned act_saved -- is what refuses a call that passed all others: the search on an init or an end call,
    # with and without the move, every group length, the edges of cess_frac and min_step; without the flag its scalars are not looked at)
    bad_act = ctypes.c_void_p(0x50008)
    for ok in (dict(), dict(group=3, cess_frac=7.0, min_step=-1.0), dict(flags=ANNEAL, cess_frac=float("nan"), min_step=float("nan"), **annealing),
               searching, both, dict(searching, flags=SCHEDULE | ANNEAL | INIT, uniform=None), dict(searching, noise=None, **{"next": None}),
               dict(searching, cess_frac=1e-6), dict(searching, cess_frac=1.0 - 2.0 ** -24), dict(searching, min_step=0.0),
               dict(searching, min_step=3.0e38), dict(searching, min_step=2.0),
               dict(both, flags=RESAMPLE | ANNEAL), dict(flags=INNER, noise=None, uniform=None)) + \
            tuple(dict(searching, group=G) for G in (2, 4, 8, 16)):
        assert said(E, "act_saved must be 16-byte aligned", **dict(ok, act=bad_act))


def test_the_older_twelve_entry_points_still_refuse_the_new_bit():
    """Nothing about the older entry points changed: bit 0x400 is unknown there."""
    import test_hmc_tempered_cpu as T
    import test_hmc_exchange_cpu as XC
    import test_hmc_resample_cpu as RC
    import test_hmc_rows_cpu as RW
    import test_hmc_metric_cpu as MC
    lib = lsnf_amd.load_library()
    seen = 0
    for mod in (T, XC, RC, RW, MC):
        for name in mod.NAMES:
            said = mod._caller(lib, name)[1]
            assert said(LSNF_E_ARG, "unknown flag bits 0x400", flags=SCHEDULE), name
            seen += 1
    assert seen == 10
    import test_hmc_cpu as HC
    import test_rhmc_cpu as RHC
    for mod in (HC, RHC):                                    # the two scalar entries
        call = mod._caller(lib)[0]
        assert call(flags=SCHEDULE) == LSNF_E_ARG and lib.lsnf_last_error().decode() == mod.NAME + ": unknown flag bits 0x400"


# ---- the Python wrappers on CPU tensors ------------------------------------------------------------------------------------------------
def _plan():
    F, lib = lsnf_amd.flow, lsnf_amd.load_library()
    return F.FlowPlan(8, 4, 2, 1, torch.zeros(lib.lsnf_plan_floats(8, 4, 2, 1)), torch.zeros(lib.lsnf_prepare_scratch_bytes(8, 4, 2) // 8, dtype=torch.float64))


def test_wrappers_refuse_a_misplaced_schedule_before_anything_else(monkeypatch):
    F, M = lsnf_amd.flow, lsnf_amd.mcmc
    lib = lsnf_amd.load_library()
    plan, B = _plan(), 8
    z, saved = torch.zeros(B, 8), torch.zeros(1, B, 8)
    act = torch.zeros(lib.lsnf_act_saved_floats(8, 4, 2, B))
    steps, state, metric = F.new_hmc_row_steps(B, "cpu", 0.5), F.new_hmc_state(plan, B, "cpu"), F.new_hmc_row_metric(plan, B, "cpu")
    temper, cap = F.new_hmc_row_temper(plan, B, "cpu"), torch.ones(B)
    zcall = lambda **kw: F.hmc_step_schedule(plan, z, None, None, state, F.PhiloxNoise(3), steps, metric, temper, **kw)
    ecall = lambda **kw: F.reverse_hmc_step_schedule(plan, z, saved, act, None, None, state, F.PhiloxNoise(3), steps, metric, temper, **kw)
    for call in (zcall, ecall):
        for bad in (3, 1, 32, "4", 0):
            with pytest.raises(lsnf_amd.LsnfError, match="schedule must be None, 2, 4, 8 or 16"):
                call(anneal=cap, schedule=bad)
        for kw in (dict(phase="inner"), dict(anneal=None), dict(phase="init", anneal=None), dict(anneal=cap, adapt="update"),
                   dict(anneal=cap, window="fold")):
            with pytest.raises(lsnf_amd.LsnfError, match="schedule goes with phase='init' or 'end' and anneal="):
                call(schedule=4, **kw)
        with pytest.raises(lsnf_amd.LsnfError, match="they must be equal"):
            call(anneal=cap, schedule=4, resample=8)
        for bad in (0.0, 1.0, -1.0, float("nan")):
            with pytest.raises(lsnf_amd.LsnfError, match="cess_target must lie in"):
                call(anneal=cap, schedule=4, cess_target=bad)
        for bad in (-0.1, float("inf"), float("nan")):
            with pytest.raises(lsnf_amd.LsnfError, match="min_step must be finite and not negative"):
                call(anneal=cap, schedule=4, min_step=bad)
        with pytest.raises(lsnf_amd.LsnfError, match="resample goes with phase='end' and anneal="):
            call(phase="init", anneal=cap, schedule=4, resample=4)
        for kw in (dict(), dict(anneal=cap), dict(anneal=cap, schedule=4), dict(phase="init", anneal=cap, schedule=8, cess_target=0.5),
                   dict(anneal=cap, schedule=8, resample=8, min_step=0.01, propose=False)):
            with pytest.raises(lsnf_amd.LsnfError, match="no CPU path"):
                call(**kw)
    # the group's length goes through the resampling path: one path, one more argument
    cpu, rng = torch.device("cpu"), object()
    with monkeypatch.context() as m:
        m.setattr(M, "_check_in", lambda t, name, need, dev, *a, **k: None)
        assert M._row_resample_args(plan, None, 0.5, None, rng, B, cpu, False, 4) == ((4, 0.0, None, None, None), None, None)
        assert M._row_resample_args(plan, None, 0.5, None, rng, B, cpu, False, None) == ((0, 0.0, None, None, None), None, None)
        with pytest.raises(lsnf_amd.LsnfError, match="are not a multiple of schedule=16"):
            M._row_resample_args(plan, None, 0.5, None, rng, B, cpu, False, 16)
        assert M._row_resample_args(plan, 8, 0.5, None, rng, B, cpu, False, 8)[0][:3] == (8, 0.5, None)
    assert M._row_resample_mode(None, "end", None, None, cap, 4, 0.9, 0.0) == 1024
    assert M._row_resample_mode(4, "end", None, None, cap, 4, 0.9, 0.0) == 1024 | 512
    assert M._row_resample_mode(None, "init", None, None, cap, 2, 0.9, 0.0) == 1024 and M._row_resample_mode(4, "end", None, None, cap) == 512
    L = lsnf_amd.langevin
    for fn in (L.estimate_log_px_smc_adaptive_z_with_flow, L.estimate_log_px_smc_adaptive_eps_with_flow):
        kw = dict(max_steps=4, chains=8, particles=4, leapfrog_steps=1, g_l_step_size=0.1, g_llhd_sigma=1.0, philox=None)
        for chains, particles in ((8, 3), (8, 16), (12, 8), (8, 1), (64, 32)):
            with pytest.raises(ValueError, match="particles must be 2, 4, 8 or 16 and divide chains"):
                fn(torch.zeros(2, 8), None, None, **dict(kw, chains=chains, particles=particles))
        for bad in (dict(cess_target=0.0), dict(cess_target=1.0), dict(min_step=-1.0), dict(min_step=float("nan")), dict(check_every=-1),
                    dict(max_steps=-1)):
            with pytest.raises(ValueError):
                fn(torch.zeros(2, 8), None, None, **dict(kw, **bad))
        assert fn(torch.zeros(2, 8), None, None, **dict(kw, max_steps=0)) == (None,) * 8
        assert fn(torch.zeros(2, 8), None, None, **dict(kw, max_steps=0, return_schedule=True)) == (None,) * 9


# ---- the restated search -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float32, torch.float64))
@pytest.mark.parametrize("P", S.GROUPS)
def test_the_search_on_hand_made_groups(P, dtype):
    """Five groups: equal energies (the ceiling exactly, in one call), one at its ceiling (left alone), one past it (left alone), a
    huge energy spread (b + min_step), a NaN row (b + min_step); beta' identical on the rows of a group."""
    t = lambda v: torch.tensor(v, dtype=dtype)
    ramp = torch.arange(P, dtype=dtype)
    b = torch.cat([t([0.25] * P), t([0.75] * P), t([0.875] * P), t([0.125] * P), t([0.5] * P)])
    cap = torch.cat([t([1.0] * P), t([0.75] * P), t([0.75] * P), t([1.0] * P), t([1.0] * P)])
    l = torch.cat([-0.5 * ramp, ramp, -ramp, 0.25 * ramp, -0.125 * ramp])
    nan_row = 3.0 + ramp
    nan_row[P - 1] = float("nan")
    el = torch.cat([t([7.5] * P), 2.0 * ramp, 3.0 * ramp, 1.0e6 * ramp, nan_row])
    ms = 2.0 ** -6
    d = S.search(b, cap, l, el, P, 0.9, ms)
    beta = d.beta.view(5, P)
    assert bool((beta == beta[:, :1]).all())
    assert beta[:, 0].tolist() == [1.0, 0.75, 0.875, 0.125 + ms, 0.5 + ms]
    assert d.whole.tolist() == [True, False, False, False, False] and d.idle.tolist() == [False, True, True, False, False]
    assert d.lo[3].item() == 0.0 and d.lo[4].item() == 0.0
    # the rows of a group at different temperatures: rung 0's are the group's
    b2, cap2 = b.clone(), cap.clone()
    b2[1::P] += 0.0625
    cap2[1::P] -= 0.0625
    assert torch.equal(S.search(b2, cap2, l, el, P, 0.9, ms).beta, d.beta)
    # a NaN weight as well; and min_step = 0 leaves such groups where they are
    l2 = l.clone()
    l2[0] = float("nan")
    assert S.search(b, cap, l2, el, P, 0.9, ms).beta[0].item() == 0.25 + ms
    assert S.search(b, cap, l2, el, P, 0.9, 0.0).beta.view(5, P)[:, 0].tolist() == [0.25, 0.75, 0.875, 0.125, 0.5]
    # a step past the ceiling is cut to it
    assert S.search(b, cap, l, el, P, 0.9, 4.0).beta.view(5, P)[:, 0].tolist() == [1.0, 0.75, 0.875, 1.0, 1.0]


def random_groups(P, G, seed, D=1.0):
    """G groups of fp32 inputs whose searches cover the span: log weights of spread 3 (|l| <= 24), energies of spread 0.5 .. 40 / D."""
    g = torch.Generator().manual_seed(seed)
    l = (3.0 * torch.randn(G * P, generator=g)).clamp(-24.0, 24.0)
    scale = torch.exp(torch.rand(G, generator=g) * (torch.log(torch.tensor(40.0)) - torch.log(torch.tensor(0.5))) + torch.log(torch.tensor(0.5)))
    el = (5.0 + (scale[:, None] / D) * torch.rand(G, P, generator=g)).reshape(-1)
    return l.float(), el.float()


@pytest.mark.parametrize("target", (0.9, 0.98))
@pytest.mark.parametrize("P", S.GROUPS)
def test_the_fp32_search_lies_within_the_derived_bound_of_the_float64_root(P, target):
    G = 4096
    l, el = random_groups(P, G, 100 * P + int(100 * target))
    b, cap = torch.zeros(G * P), torch.ones(G * P)
    d = S.search(b, cap, l, el, P, target, 0.0)
    D = torch.ones(G, dtype=torch.float64)
    end = S.cess64(D, l, el, P)
    e = S.eps_c(P, 24.0, 40.0)
    clear = (end < target * (1.0 - e)) | (end >= target * (1.0 + e))          # the ceiling's own comparison is not within fp32 of a tie
    assert bool(torch.equal(d.whole[clear], (end >= target)[clear])) and int(clear.sum()) >= G - 4
    srch = d.searching & clear
    assert int(srch.sum()) >= G // 4 and int(d.whole.sum()) >= G // 100, (int(srch.sum()), int(d.whole.sum()))
    idx = srch.nonzero()[:, 0]
    rows = (idx[:, None] * P + torch.arange(P)[None, :]).reshape(-1)
    ls, es, Ds = l[rows], el[rows], D[idx]
    assert bool(S.monotone(Ds, ls, es, P).all())              # (a condition on these inputs, in float64)
    root = S.root64(Ds, ls, es, P, target)
    s = S.slack(Ds, torch.zeros_like(Ds), ls, es, P, target, root)
    h = Ds * 2.0 ** -S.HALVINGS
    err = (d.beta.view(G, P)[idx, 0].double() - root) / h
    print(f"P={P} target={target}: {idx.numel()} searching groups, delta32 - delta* in [{err.min():+.3f}, {err.max():+.3f}] brackets; "
          f"s in [{s.min():.3g}, {s.max():.3g}]")
    assert bool((err >= -(1.0 + s)).all()) and bool((err <= s).all())
    assert float(s.median()) < 1.0                            # the bound is about one bracket, not a licence


def test_the_designed_launches_of_the_gpu_tests_are_clear_in_float64():
    """tests/hmc_schedule_gpu.py `design` / `expected` on the CPU: every launch of every case has its kinds of group clear of the
    target by the fp32 error of cess, the searching groups' cess falls monotonically, the restated fp32 search lands inside the bound the
    device is held to, and every launch of three groups or more has all three kinds."""
    import hmc_schedule_gpu as AG
    worst = 0.0
    for case in AG.MOVE + AG.FORMS + AG.EDGE:
        B, P = case[-2:]
        for seed in (P, P + 1, 40 + P, 90 + P):
            beta, cap, pair, energy, kind = AG.design(B, P, seed)
            D, idx, root, slack = AG.expected(beta, cap, pair, energy, kind, P, AG.FRAC)
            if B // P >= 3:
                assert all(bool((kind == k).any()) for k in (AG.SEARCH, AG.WHOLE, AG.IDLE))
            d = S.search(beta, cap, pair[:, 0] - pair[:, 1], energy, P, AG.FRAC, 0.0)
            assert torch.equal(d.searching, kind == AG.SEARCH) and torch.equal(d.whole, kind == AG.WHOLE) and torch.equal(d.idle, kind == AG.IDLE)
            if idx.numel():
                g0, b0 = d.beta.view(-1, P)[idx, 0].double(), beta.view(-1, P)[idx, 0].double()
                err = ((g0 - b0) - root) / (D[idx] * 2.0 ** -S.HALVINGS)
                assert bool((err >= -(1.0 + slack)).all()) and bool((err <= slack).all())
                worst = max(worst, float(slack.max()))
    print(f"designed launches: s up to {worst:.3g}")

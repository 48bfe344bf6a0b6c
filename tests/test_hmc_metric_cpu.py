"""CPU: the per-row diagonal metric of Hamiltonian Monte Carlo and its windowed estimation (`lsnf_hmc_step_metric`,
`lsnf_reverse_hmc_step_metric`, include/lsnf_flow_mcmc.h): the C declarations and the ctypes binding outside the core ABI, the Python
layers, every refusal the entry points make before any HIP call (fake aligned pointers that are never dereferenced, as
tests/test_hmc_rows_cpu.py), Stan's window schedule, and the properties of the float64 restatement alone
(tests/hmc_metric_restated.py).

The warm-up experiment (`hmc_metric_restated.experiment`: TINY flow prior plus an axis-aligned quadratic energy with a log-spaced from
0.3 to 30, 64 rows at a first step of 0.3, L = 3, 300 warm-up trajectories with windows closing at 100 / 150 / 250 and 60 frozen ones)
was run on the CPU at seeds 0 .. 7, for the chain on z and for the one on eps (profiles/hmc_metric_cpu.txt has every seed's figures
and the arithmetic of the bands: the observed range widened by 3 standard errors of one run)."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

from conftest import ROOT
import hmc_rows_restated as R
import hmc_metric_restated as MR

import lsnf_amd

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2
INIT, INNER, ADAPT, LAST, FOLD, CLOSE = 1, 2, 4, 8, 16, 32
NAMES = ("lsnf_hmc_step_metric", "lsnf_reverse_hmc_step_metric")
ROWS = {"lsnf_hmc_step_metric": "lsnf_hmc_step_rows", "lsnf_reverse_hmc_step_metric": "lsnf_reverse_hmc_step_rows"}
COUNT = {"lsnf_hmc_step_metric": 34, "lsnf_reverse_hmc_step_metric": 32}
FIVE = ["scale_rows", "mean_rows", "m2_rows", "count_rows", "reg"]
FAKE = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(28)]     # 16-byte aligned addresses that are never dereferenced on the host
BAND = {                                                     # (profiles/hmc_metric_cpu.txt; hmc_metric_restated.BAND is held to it below)
    "z": {"accept": (0.871, 0.925), "step": (0.646, 0.739), "scale": (0.093, 0.127)},
    "eps": {"accept": (0.963, 0.984), "step": (0.115, 0.168), "scale": (1.095, 1.338)},
}


def test_symbols_are_declared_exported_and_bound_outside_the_core_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow_mcmc.h")).read(), flags=re.S)
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    ext = lsnf_amd._lib._EXT_SIGNATURES
    assert len(re.findall(r"#define\s+LSNF_HMC_METRIC_FOLD\s+16u", hdr)) == 1 and len(re.findall(r"#define\s+LSNF_HMC_METRIC_CLOSE\s+32u", hdr)) == 1
    assert re.search(r"typedef\s+struct\s+LsnfMetricReg\s*\{\s*float\s+n0,\s*var0,\s*scale_min,\s*scale_max;\s*\}\s*LsnfMetricReg;", hdr)
    Reg = lsnf_amd._lib.LsnfMetricReg
    assert [f for f, _ in Reg._fields_] == ["n0", "var0", "scale_min", "scale_max"] and all(t is ctypes.c_float for _, t in Reg._fields_)
    assert ctypes.sizeof(Reg) == 16 and [getattr(Reg, f).offset for f, _ in Reg._fields_] == [0, 4, 8, 12]
    decl = lambda name: [re.sub(r".*[\s*]", "", a.strip())
                         for a in re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1).split(",")]
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and name not in core and hasattr(lib, name)
        assert name in ext and len(ext[name][1]) == COUNT[name] and name not in lsnf_amd.exported_symbols() and name not in lsnf_amd._lib._SIGNATURES
        assert getattr(lib, name).argtypes == ext[name][1]               # attached in load()
        # the declaration's parameters: the per-row call's with the five inserted between da and flags
        names, rows = decl(name), decl(ROWS[name])
        at = rows.index("da") + 1
        assert rows[at] == "flags" and len(names) == COUNT[name] == len(rows) + 5 and names == rows[:at] + FIVE + rows[at:]
        args, rargs = ext[name][1], ext[ROWS[name]][1]
        assert args[:at] == rargs[:at] and args[at + 5:] == rargs[at:] and args[at:at + 4] == [ctypes.c_void_p] * 4
        assert args[at + 4] is ctypes.POINTER(Reg)
        # the per-row declarations are what they were
        assert len(rows) == COUNT[name] - 5 and len(rargs) == len(rows)
    assert lsnf_amd._lib.extension_symbols() == sorted(ext)
    assert lib.lsnf_abi_version() == 5 and lsnf_amd._lib.ABI_VERSION == 5


def test_python_layers_exist_and_the_existing_ones_are_unchanged():
    F, L, M = lsnf_amd.flow, lsnf_amd.langevin, lsnf_amd.mcmc
    assert F.hmc_step_metric is M.hmc_step_metric and F.reverse_hmc_step_metric is M.reverse_hmc_step_metric
    assert F.HmcRowMetric is M.HmcRowMetric and F.new_hmc_row_metric is M.new_hmc_row_metric
    assert (F.HMC_METRIC_FOLD, F.HMC_METRIC_CLOSE) == (16, 32)
    for new, old in ((F.hmc_step_metric, F.hmc_step_rows), (F.reverse_hmc_step_metric, F.reverse_hmc_step_rows),
                     (lsnf_amd._netF.hmc_step_metric, lsnf_amd._netF.hmc_step_rows),
                     (lsnf_amd._netF.reverse_hmc_step_metric, lsnf_amd._netF.reverse_hmc_step_rows)):
        a, b = inspect.signature(new).parameters, inspect.signature(old).parameters
        want = []
        for n in b:
            want.append(n)
            if n == "steps":
                want.append("metric")
        assert [n for n in a] == want + ["window"]
        assert a["window"].kind is inspect.Parameter.KEYWORD_ONLY and a["window"].default is None
        for n in b:
            assert a[n].kind == b[n].kind and a[n].default == b[n].default
    assert [f for f in F.HmcRowMetric.__dataclass_fields__] == ["scale", "mean", "m2", "count", "n0", "var0", "scale_min", "scale_max"]
    assert [F.HmcRowMetric.__dataclass_fields__[f].default for f in ("n0", "var0", "scale_min", "scale_max")] == [5.0, 1e-3, 1e-3, 1e3]
    sig = inspect.signature(F.new_hmc_row_metric)
    assert list(sig.parameters) == ["plan", "B", "device", "scale"] and sig.parameters["scale"].default == 1.0
    for fn, old, first in ((L.sample_hmc_metric_post_z_with_flow, L.sample_hmc_adaptive_post_z_with_flow, "z"),
                           (L.sample_hmc_metric_post_eps_with_flow, L.sample_hmc_adaptive_post_eps_with_flow, "eps")):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == list(inspect.signature(old).parameters) + ["metric", "windows"] and list(sig.parameters)[0] == first
        for kw in list(sig.parameters)[4:]:
            assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
        assert sig.parameters["metric"].default is None and sig.parameters["windows"].default is None
    sig = inspect.signature(L.warmup_windows)
    assert list(sig.parameters) == ["W", "init_buffer", "term_buffer", "base_window"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == [75, 50, 25]
    # the existing layers keep their signatures and their fields
    assert [f for f in F.HmcRowSteps.__dataclass_fields__] == ["step", "adapt", "target_accept", "gamma", "t0", "kappa", "step_min", "step_max"]
    assert list(inspect.signature(M._check_chain).parameters) == ["plan", "point", "name", "grad_g", "energy_g", "state", "state_cls", "noise",
                                                                  "uniform", "stash"]
    assert len(lsnf_amd._lib._EXT_SIGNATURES["lsnf_hmc_step_rows"][1]) == 29 and len(lsnf_amd._lib._EXT_SIGNATURES["lsnf_reverse_hmc_step_rows"][1]) == 27


def _plan():
    F, lib = lsnf_amd.flow, lsnf_amd.load_library()
    return F.FlowPlan(8, 4, 2, 1, torch.zeros(lib.lsnf_plan_floats(8, 4, 2, 1)), torch.zeros(lib.lsnf_prepare_scratch_bytes(8, 4, 2) // 8, dtype=torch.float64))


def test_new_row_metric_fills_the_state():
    F, plan = lsnf_amd.flow, _plan()
    m = F.new_hmc_row_metric(plan, 5, "cpu")
    assert m.scale.shape == m.mean.shape == m.m2.shape == (5, 8) and m.count.shape == (5,)
    assert all(t.dtype == torch.float32 for t in (m.scale, m.mean, m.m2, m.count))
    assert bool((m.scale == 1.0).all()) and not m.mean.any() and not m.m2.any() and not m.count.any()
    assert (m.n0, m.var0, m.scale_min, m.scale_max) == (5.0, 1e-3, 1e-3, 1e3)
    assert bool((F.new_hmc_row_metric(plan, 3, "cpu", 0.25).scale == 0.25).all())
    sd = torch.rand(5, 8) + 0.5
    m = F.new_hmc_row_metric(plan, 5, "cpu", sd)
    assert torch.equal(m.scale, sd) and m.scale.data_ptr() != sd.data_ptr()
    with pytest.raises(lsnf_amd.LsnfError):
        F.new_hmc_row_metric(plan, 4, "cpu", sd)


# ---- the refusals of the two entry points ------------------------------------------------------------------------------------
Z_ARGS = ("plan", "point", "z_out", "saved", "act", "ll", "grad_g", "energy", "p_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")
E_ARGS = ("plan", "point", "saved", "act", "grad_g", "energy", "p_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")


def _caller(lib, name):
    Rng, Da, Reg = lsnf_amd._lib.LsnfRng, lsnf_amd._lib.LsnfDualAvg, lsnf_amd._lib.LsnfMetricReg
    order = Z_ARGS if name == "lsnf_hmc_step_metric" else E_ARGS
    ptrs = dict(zip(order + ("step_rows", "adapt", "scale", "mean", "m2", "count", "next", "accept", "la"), FAKE))
    base = dict(ptrs, nz=128, w=64, d=5, c=1, B=4, rng=None, da=None, adapt=None, mean=None, m2=None, count=None, reg=None, flags=0,
                accept=None, la=None)
    fn = getattr(lib, name)

    def call(**kw):
        a = dict(base, **kw)
        return fn(a["plan"], a["nz"], a["w"], a["d"], a["c"], a["B"], *(a[k] for k in order[1:]),
                  None if a["rng"] is None else ctypes.byref(a["rng"]), a["step_rows"], a["adapt"],
                  None if a["da"] is None else ctypes.byref(a["da"]), a["scale"], a["mean"], a["m2"], a["count"],
                  None if a["reg"] is None else ctypes.byref(a["reg"]), a["flags"], a["next"], a["accept"], a["la"], None)

    def said(code, text, **kw):
        rc = call(**kw)
        return rc == code and lib.lsnf_last_error().decode() == name + ": " + text
    return call, said, ptrs, Rng, Da, Reg


@pytest.mark.parametrize("name", NAMES)
def test_every_new_rule_refuses_before_any_hip_call(name):
    lib = lsnf_amd.load_library()
    call, said, P, Rng, Da, Reg = _caller(lib, name)
    z = name == "lsnf_hmc_step_metric"
    nxt, acc_name = ("z_next", "z_acc") if z else ("eps_next", "eps_acc")
    da = Da(target_accept=0.8, gamma=0.05, t0=10.0, kappa=0.75, step_min=1e-4, step_max=1e2)
    good = lambda **kw: Reg(**dict(dict(n0=5.0, var0=1e-3, scale_min=1e-3, scale_max=1e3), **kw))
    folding = dict(flags=FOLD, mean=P["mean"], m2=P["m2"], count=P["count"], reg=good())
    closing = dict(folding, flags=FOLD | CLOSE)
    adapting = dict(flags=ADAPT, adapt=P["adapt"], da=da)
    inner = dict(flags=INNER, noise=None, uniform=None)
    E = LSNF_E_ARG
    nan, inf = float("nan"), float("inf")
    for B in (0, 4):                                         # rules that precede the empty-batch return: the same answer for B = 0
        assert said(E, "unknown flag bits 0x40", B=B, flags=64) and said(E, "unknown flag bits 0x80000000", B=B, **dict(folding, flags=0x80000000 | FOLD))
        only_end = "flags: LSNF_HMC_METRIC_FOLD goes with an end call (neither LSNF_HMC_INIT nor LSNF_HMC_INNER)"
        assert said(E, only_end, B=B, **dict(folding, flags=FOLD | INIT)) and said(E, only_end, B=B, **dict(folding, **dict(inner, flags=FOLD | INNER)))
        assert said(E, only_end, B=B, **dict(closing, flags=FOLD | CLOSE | INIT))
        assert said(E, "flags: LSNF_HMC_METRIC_CLOSE goes with LSNF_HMC_METRIC_FOLD", B=B, flags=CLOSE)
        assert said(E, "flags: LSNF_HMC_METRIC_CLOSE goes with LSNF_HMC_METRIC_FOLD", B=B, **dict(adapting, flags=ADAPT | CLOSE))
        assert said(E, "reg is required with LSNF_HMC_METRIC_FOLD", B=B, **dict(folding, reg=None))
        none = "mean_rows, m2_rows, count_rows and reg must be NULL without LSNF_HMC_METRIC_FOLD"
        for k in ("mean", "m2", "count"):
            assert said(E, none, B=B, **{k: P[k]}) and said(E, none, B=B, **dict(inner, **{k: P[k]}))
        assert said(E, none, B=B, reg=good()) and said(E, none, B=B, **dict(adapting, reg=good()))
        for field in ("n0", "var0", "scale_min", "scale_max"):
            for bad, word in ((nan, "nan"), (inf, "inf"), (-inf, "-inf")):
                assert said(E, f"reg: every field must be finite (got {word})", B=B, **dict(folding, reg=good(**{field: bad})))
        assert said(E, "reg->n0 must not be negative (got -1)", B=B, **dict(folding, reg=good(n0=-1.0)))
        assert said(E, "reg->var0 must not be negative (got -0.5)", B=B, **dict(closing, reg=good(var0=-0.5)))
        for bad in (0.0, -0.25):
            assert said(E, f"reg->scale_min must be positive (got {bad:g})", B=B, **dict(folding, reg=good(scale_min=bad)))
        assert said(E, "reg->scale_max must not be below reg->scale_min (got 0.5 < 1)", B=B, **dict(folding, reg=good(scale_min=1.0, scale_max=0.5)))
        # the four arrays alias nothing else the call touches
        assert said(E, "scale_rows must not alias grad_g", B=B, scale=P["grad_g"]) and said(E, "scale_rows must not alias noise", B=B, scale=P["noise"])
        assert said(E, f"{acc_name} must not alias scale_rows", B=B, scale=P["p_acc"]) and said(E, "mom must not alias scale_rows", B=B, scale=P["mom"])
        assert said(E, f"{nxt} must not alias scale_rows", B=B, scale=P["next"]) and said(E, "step_rows must not alias scale_rows", B=B, scale=P["step_rows"])
        assert said(E, "scale_rows must not alias " + ("z_prop" if z else "eps_prop"), B=B, scale=P["point"])
        assert said(E, "mean_rows must not alias energy_g", B=B, **dict(folding, mean=P["energy"]))
        assert said(E, "scale_rows must not alias mean_rows", B=B, **dict(folding, mean=P["scale"]))
        assert said(E, "mean_rows must not alias m2_rows", B=B, **dict(folding, m2=P["mean"]))
        assert said(E, "kin0 must not alias count_rows", B=B, **dict(folding, count=P["kin0"]))
        assert said(E, "adapt must not alias m2_rows", B=B, **dict(adapting, **dict(folding, flags=ADAPT | FOLD, m2=P["adapt"])))
        # the per-row call's rules, word for word (a sample: the whole table is tests/test_hmc_rows_cpu.py's)
        assert said(E, "flags: LSNF_HMC_INIT and LSNF_HMC_INNER exclude each other", B=B, flags=INIT | INNER, noise=None, uniform=None)
        assert said(E, "flags: LSNF_HMC_ADAPT goes with an end call (neither LSNF_HMC_INIT nor LSNF_HMC_INNER)", B=B, **dict(adapting, flags=ADAPT | INIT))
        assert said(E, "flags: LSNF_HMC_ADAPT_LAST goes with LSNF_HMC_ADAPT", B=B, flags=LAST)
        assert said(E, "da is required with LSNF_HMC_ADAPT", B=B, flags=ADAPT, adapt=P["adapt"])
        assert said(E, "adapt and da must be NULL without LSNF_HMC_ADAPT", B=B, **dict(folding, da=da))
        assert said(E, "pass either a uniform tensor or an rng, not both", B=B, noise=None, rng=Rng(1, 0, None, 0))
        assert said(E, "noise is not taken with LSNF_HMC_INNER (an inner step draws nothing)", B=B, flags=INNER, uniform=None)
        assert said(E, f"{nxt} must not alias mom", B=B, mom=P["next"])
    assert call(nz=130) == LSNF_E_GEOMETRY and call(nz=130, B=0) == LSNF_E_GEOMETRY and said(E, "B=-1 out of range", B=-1)
    # an empty batch: nothing to launch, NULL pointers allowed, in every phase, folding and closing
    nulls = {k: None for k in P}
    assert call(B=0, **nulls) == LSNF_OK and call(B=0, **dict(nulls, flags=INNER)) == LSNF_OK and call(B=0, **dict(nulls, flags=INIT)) == LSNF_OK
    assert call(B=0, **dict(nulls, flags=FOLD, reg=good())) == LSNF_OK and call(B=0, **dict(nulls, flags=FOLD | CLOSE, reg=good())) == LSNF_OK
    assert call(B=0, **dict(nulls, flags=FOLD | CLOSE | ADAPT, reg=good(), da=da)) == LSNF_OK
    assert call(B=0, **folding) == LSNF_OK and call(B=0, **closing) == LSNF_OK and call(B=0, **{"next": P["point"]}) == LSNF_OK
    # the pointers of a non-empty call
    for extra in (dict(), inner, dict(flags=INIT), folding, closing):
        assert said(E, "scale_rows is required (NULL)", **dict(extra, scale=None))
        assert said(E, "step_rows is required (NULL)", **dict(extra, step_rows=None))
    for k in ("mean", "m2", "count"):
        for base in (folding, closing):
            assert said(E, "mean_rows, m2_rows and count_rows are required with LSNF_HMC_METRIC_FOLD", **dict(base, **{k: None}))
    odd = ctypes.c_void_p(0xF00002)
    assert said(E, "scale_rows must be 4-byte aligned", scale=odd) and said(E, "scale_rows must be 4-byte aligned", **dict(inner, scale=odd))
    assert said(E, "mean_rows must be 4-byte aligned", **dict(folding, mean=odd)) and said(E, "m2_rows must be 4-byte aligned", **dict(folding, m2=odd))
    assert said(E, "count_rows must be 4-byte aligned", **dict(closing, count=odd))
    assert said(E, "adapt is required with LSNF_HMC_ADAPT", **dict(folding, flags=FOLD | ADAPT, da=da))
    assert said(E, "uniform is required without an rng (unless LSNF_HMC_INIT or LSNF_HMC_INNER)", uniform=None)
    assert said(E, f"{nxt} is required (NULL) with LSNF_HMC_INNER", **dict(inner, **{"next": None}))
    # (the next rule -- a misaligned act_saved -- is what refuses a call that passed all others; 4 bytes off a 16-byte boundary is
    # allowed for the four arrays)
    bad_act = ctypes.c_void_p(0x50008)
    off4 = lambda k: ctypes.c_void_p(P[k].value + 4)
    both = dict(adapting, **dict(closing, flags=ADAPT | FOLD | CLOSE))
    for ok in (dict(), folding, closing, both, dict(both, flags=ADAPT | LAST | FOLD | CLOSE), dict(closing, noise=None, **{"next": None}), inner,
               dict(flags=INIT, uniform=None), dict(folding, noise=None, uniform=None, rng=Rng(1, 0, None, 0)),
               dict(closing, reg=good(n0=0.0, var0=0.0)), dict(closing, reg=good(scale_min=0.3, scale_max=0.3)),
               dict(closing, scale=off4("scale"), mean=off4("mean"), m2=off4("m2"), count=off4("count"))):
        assert said(E, "act_saved must be 16-byte aligned", **dict(ok, act=bad_act))


def test_the_per_row_entry_points_still_refuse_the_new_bits():
    """Nothing about lsnf_hmc_step_rows changed: bit 0x10 is unknown there (tests/test_hmc_rows_cpu.py pins it for both)."""
    lib = lsnf_amd.load_library()
    fn = lib.lsnf_hmc_step_rows
    rc = fn(FAKE[0], 128, 64, 5, 1, 4, *FAKE[1:15], None, FAKE[15], None, None, FOLD | CLOSE, FAKE[17], None, None, None)
    assert rc == LSNF_E_ARG and lib.lsnf_last_error().decode() == "lsnf_hmc_step_rows: unknown flag bits 0x30"


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
    zcall = lambda steps=steps, metric=metric, **kw: F.hmc_step_metric(plan, z, None, None, state, F.PhiloxNoise(3), steps, metric, **kw)
    ecall = lambda steps=steps, metric=metric, **kw: F.reverse_hmc_step_metric(plan, z, saved, act, None, None, state, F.PhiloxNoise(3), steps,
                                                                               metric, **kw)
    for call in (zcall, ecall):
        n = len(seen)
        with pytest.raises(lsnf_amd.LsnfError, match="phase must be one of"):
            call(phase="middle")
        with pytest.raises(lsnf_amd.LsnfError, match=r"steps must be a flow.HmcRowSteps \(new_hmc_row_steps\(\)\)"):
            call(steps=0.5)
        with pytest.raises(lsnf_amd.LsnfError, match=r"metric must be a flow.HmcRowMetric \(new_hmc_row_metric\(\)\)"):
            call(metric=torch.ones(5, 8))
        with pytest.raises(lsnf_amd.LsnfError, match="window must be None, 'fold' or 'close'"):
            call(window="open")
        with pytest.raises(lsnf_amd.LsnfError, match="adapt must be None, 'update' or 'last'"):
            call(adapt="yes", window="fold")
        for phase in ("init", "inner"):
            with pytest.raises(lsnf_amd.LsnfError, match="window goes with phase='end'"):
                call(phase=phase, window="fold")
        assert len(seen) == n                                # (refused before the tensors are looked at)
        for kw in (dict(), dict(window="fold"), dict(window="close", adapt="update"), dict(window="close", propose=False), dict(phase="init")):
            with pytest.raises(lsnf_amd.LsnfError, match="no CPU path"):
                call(**kw)
        assert len(seen) == n + 5                            # every such call went through _check_chain
    assert all(st is None for st in seen[:5]) and all(st is not None and st[0] is saved and st[1] is act for st in seen[5:])
    # the four arrays of `metric` go through the one checking path
    with pytest.raises(lsnf_amd.LsnfError, match="metric.scale must live on"):
        lsnf_amd.mcmc._row_metric_args(plan, metric, 5, torch.device("cuda:0"), None)
    names = []
    with monkeypatch.context() as m:
        m.setattr(lsnf_amd.mcmc, "_check_out", lambda t, name, need, dev, *a, **k: names.append((name, need)))
        for window, n_reg in ((None, 0), ("fold", 1), ("close", 1)):
            args = lsnf_amd.mcmc._row_metric_args(plan, metric, 5, torch.device("cpu"), window)
            assert len(args) == 5 and args[0] == metric.scale.data_ptr() and sum(a is not None for a in args[1:]) == 4 * n_reg
    assert names == [("metric.scale", 40), ("metric.mean", 40), ("metric.m2", 40), ("metric.count", 5)] * 3
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    with pytest.raises(lsnf_amd.LsnfError):
        net.hmc_step_metric(z, None, None, state, F.PhiloxNoise(1), steps, metric, phase="init")
    with pytest.raises(lsnf_amd.LsnfError):
        net.reverse_hmc_step_metric(z, saved, act, None, None, state, F.PhiloxNoise(1), steps, metric, phase="init")
    # the samplers: their own rules, then the wrappers'; nothing to do returns the input without a launch
    x, G = torch.zeros(5, 8), torch.nn.Flatten()
    kw = dict(g_l_step_size=0.5, g_llhd_sigma=0.3)
    for fn in (L.sample_hmc_metric_post_z_with_flow, L.sample_hmc_metric_post_eps_with_flow):
        with pytest.raises(ValueError, match="leapfrog_steps"):
            fn(z, x, G, net, g_l_steps=2, leapfrog_steps=0, warmup_steps=0, philox=F.PhiloxNoise(1), **kw)
        with pytest.raises(ValueError, match="warmup_steps"):
            fn(z, x, G, net, g_l_steps=2, leapfrog_steps=2, warmup_steps=3, philox=F.PhiloxNoise(1), **kw)
        with pytest.raises(lsnf_amd.LsnfError, match="metric must be a flow.HmcRowMetric"):
            fn(z, x, G, net, g_l_steps=2, leapfrog_steps=2, warmup_steps=1, philox=F.PhiloxNoise(1), metric=1.0, **kw)
        with pytest.raises(ValueError, match="windows"):
            fn(z, x, G, net, g_l_steps=40, leapfrog_steps=2, warmup_steps=30, philox=F.PhiloxNoise(1), windows=(5, [20, 10]), **kw)
        with pytest.raises(lsnf_amd.LsnfError):
            fn(z, x, G, net, g_l_steps=2, leapfrog_steps=2, warmup_steps=1, philox=F.PhiloxNoise(1), **kw)
        ph = F.PhiloxNoise(5, 100)
        none = fn(z.view(5, 8, 1, 1), x, G, net, g_l_steps=0, leapfrog_steps=2, warmup_steps=0, philox=ph, steps=steps, metric=metric, **kw)
        assert torch.equal(none[0].reshape(5, 8), z) and all(t is None for t in none[1:-2]) and none[-2] is steps and none[-1] is metric
        empty = fn(z[:0], x[:0], G, net, g_l_steps=4, leapfrog_steps=2, warmup_steps=2, philox=ph, **kw)
        assert empty[0].shape[0] == 0 and empty[-3] is None and empty[-2] is None and empty[-1] is None and ph.offset == 100
    assert stand.launching() == [], dict(stand.entered)


# ---- Stan's window schedule ----------------------------------------------------------------------------------------------------
def test_warmup_windows_are_stans():
    W = lsnf_amd.langevin.warmup_windows
    assert W(1000) == (76, [100, 150, 250, 450, 950]) and W(300) == (76, [100, 150, 250]) and W(150) == (76, [100]) and W(60) == (10, [54])
    assert W(19) == (None, []) and W(0) == (None, []) and W(20) == (4, [18])
    assert W(300) == MR.EXP_WINDOWS
    assert W(200, init_buffer=10, term_buffer=10, base_window=20) == (11, [30, 70, 190])
    for w in range(20, 400, 7):                              # the slow phase is covered by windows that at least double
        first, closes = W(w)
        sizes = [b - a for a, b in zip([first - 1] + closes, closes)]
        assert first >= 1 and closes[-1] <= w and all(b >= 2 * a for a, b in zip(sizes, sizes[1:])) and sorted(set(closes)) == closes
    modes, wins = MR.schedule(300, 60, *W(300))
    assert modes.count("update") == 299 and modes[299] == "last" and modes[300:] == [None] * 60
    assert [t + 1 for t, w in enumerate(wins) if w == "close"] == [100, 150, 250] and wins.count("fold") == 250 - 76 + 1 - 3
    assert wins[74] is None and wins[75] == "fold" and wins[250] is None


# ---- the restatement alone -------------------------------------------------------------------------------------------------
def same(a, b):
    """The same float64 bits (a row whose first adapted step overshoots may hold a NaN, which compares as bits)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _setup(B=24, seed=5, T=3, space="z"):
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
def test_a_unit_scale_is_the_per_row_chain(space):
    p, quad, z0, noises, uniforms, g = _setup(space=space)
    B, L = z0.shape[0], 3
    step = torch.where(torch.arange(B) % 2 == 0, torch.tensor(1.2), torch.tensor(0.6)).double()
    da = R.DualAvg()
    clone = lambda xs: [None if x is None else x.clone() for x in xs]
    for modes in (None, ["update", "update", "last"]):
        ref = R.chain(p, z0, quad, step, L, clone(noises), uniforms, da=da, modes=modes, space=space)
        got = MR.chain(MR.flow_potential(space, p, quad), z0, step, torch.ones(B, 8, dtype=torch.float64), L, clone(noises), uniforms, da=da, modes=modes)
        assert same(got.la, ref.la) and torch.equal(got.acc, ref.acc) and same(got.steps, ref.steps) and same(got.adapt, ref.adapt)
        assert all(same(a, b) for a, b in zip(got.state, ref.state)) and 0 < int(got.acc.sum()) < got.acc.numel()
        assert not got.mean.any() and not got.count.any() and bool((got.scale == 1.0).all())


@pytest.mark.parametrize("space", R.SPACES)
def test_a_scale_is_hmc_with_identity_mass_on_the_rescaled_target(space):
    """The chain with scale sd on U equals the unit-scale chain on y -> U(sd y), mapped back: HMC with mass diag(sd^-2)."""
    p, quad, z0, noises, uniforms, g = _setup(space=space)
    B, L = z0.shape[0], 3
    sd = torch.exp2(6.0 * torch.rand(B, 8, generator=g, dtype=torch.float64) - 3.0) * 0.3
    step = torch.full((B,), 0.5, dtype=torch.float64)
    pot = MR.flow_potential(space, p, quad)

    def pot_y(y):
        out = pot(sd * y)
        return out[0], sd * out[1]
    clone = lambda xs: [None if x is None else x.clone() for x in xs]
    a = MR.chain(pot, z0, step, sd, L, clone(noises), uniforms)
    b = MR.chain(pot_y, z0 / sd, step, torch.ones_like(sd), L, clone(noises), uniforms)
    scale = 1.0 + a.la.abs()
    assert bool(((a.la - b.la).abs() <= 1e-12 * scale).all()) and torch.equal(a.acc, b.acc) and 0 < int(a.acc.sum()) < a.acc.numel()
    assert bool(((a.states - sd * b.states).abs() <= 1e-12 * (1.0 + a.states.abs())).all())
    assert bool(((a.state[2] - b.state[2]).abs() <= 1e-12 * (1.0 + a.state[2].abs())).all())
    # and it is not the unit chain
    assert not torch.equal(a.acc, MR.chain(pot, z0, step, torch.ones_like(sd), L, clone(noises), uniforms).acc)


def test_a_windows_folds_are_the_sample_mean_and_variance():
    g = torch.Generator().manual_seed(3)
    B, nz, n = 7, 8, 40
    xs = 3.0 + 2.0 * torch.randn(n, B, nz, generator=g, dtype=torch.float64)
    mean, m2, count = torch.zeros(B, nz, dtype=torch.float64), torch.zeros(B, nz, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    for k in range(n):
        mean, m2, count = MR.fold(mean, m2, count, xs[k])
        if k == 0:
            assert torch.equal(mean, xs[0]) and not m2.any() and bool((count == 1).all())
    assert bool((count == n).all())
    assert bool(((mean - xs.mean(0)).abs() <= 1e-13).all()) and bool(((m2 / (n - 1) - torch.var(xs, 0, unbiased=True)).abs() <= 1e-12).all())
    # in fp32 the same to fp32 rounding of the magnitudes
    m32, q32, c32 = torch.zeros(B, nz), torch.zeros(B, nz), torch.zeros(B)
    for k in range(n):
        m32, q32, c32 = MR.fold(m32, q32, c32, xs[k].float())
    assert m32.dtype == torch.float32 and bool(((m32.double() - mean).abs() <= 1e-6 * (1 + mean.abs())).all())
    assert bool(((q32.double() - m2).abs() <= 1e-5 * m2).all())


def test_the_close_formula_the_single_sample_rule_and_the_restart():
    reg = MR.Reg()
    B, nz = 5, 8
    g = torch.Generator().manual_seed(4)
    sd = torch.rand(B, nz, generator=g, dtype=torch.float64) + 0.5
    m2 = torch.rand(B, nz, generator=g, dtype=torch.float64) * 30.0
    m2[2] = 1e12; m2[3] = 0.0
    n = torch.tensor([1.0, 2.0, 25.0, 25.0, 100.0], dtype=torch.float64)
    new = MR.close(sd, m2, n, reg)
    assert torch.equal(new[0], sd[0])                        # n < 2 keeps the scale
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    for b in (1, 4):
        v = (n[b] / (n[b] + 5.0)) * (m2[b] / (n[b] - 1.0)) + f32(1e-3) * (5.0 / (n[b] + 5.0))
        assert bool(((new[b] - torch.sqrt(v)).abs() <= 1e-15).all())
    assert bool((new[2] == f32(1e3)).all())                  # clamped above
    floor = (f32(1e-3) * 5.0 / 30.0) ** 0.5                  # no spread at all: the regulariser alone, sqrt(var0 n0 / (n + n0))
    assert bool(((new[3] - floor).abs() <= 1e-15).all()) and floor > f32(1e-3)
    assert bool((MR.close(sd, m2, n, MR.Reg(scale_min=0.7, scale_max=0.9)) [1:] >= f32(0.7)).all())
    assert bool((MR.close(sd, m2, n, MR.Reg(scale_min=0.7, scale_max=0.9))[1:] <= f32(0.9)).all())
    c32 = MR.close(sd.float(), m2.float(), n.float(), reg, dtype=torch.float32)
    assert c32.dtype == torch.float32 and bool(((c32.double() - new).abs() <= 1e-6 * new).all())
    # in a chain: a close zeroes the window, writes the scale and, with "update", restarts the dual averaging at log(10 s')
    p, quad, z0, noises, uniforms, g = _setup(T=4)
    B = z0.shape[0]
    step, ones = torch.full((B,), 0.9, dtype=torch.float64), torch.ones(B, 8, dtype=torch.float64)
    pot, da = MR.flow_potential("z", p, quad), R.DualAvg()
    clone = lambda xs: [None if x is None else x.clone() for x in xs]
    run = lambda modes, wins: MR.chain(pot, z0, step, ones, 3, clone(noises), uniforms, da=da, modes=modes, windows=wins)
    t = run(["update"] * 4, [None, "fold", "fold", "close"])
    assert not t.mean.any() and not t.m2.any() and not t.count.any()
    assert same(t.adapt, MR.restart(t.steps[-1])) and same(t.adapt[:, 3], torch.log(10.0 * t.steps[-1]))
    mean, m2, count = MR.fold(*MR.fold(*MR.fold(torch.zeros_like(ones), torch.zeros_like(ones), torch.zeros(B, dtype=torch.float64), t.states[1]),
                                       t.states[2]), t.states[3])
    assert same(t.scale, MR.close(ones, m2, count, MR.Reg())) and not same(t.scale, ones)
    # a fold leaves the decisions alone (the scale is unchanged until a close), "last" keeps the per-row call's quad
    plain, folded = run(["update"] * 4, None), run(["update"] * 4, [None, "fold", "fold", "fold"])
    assert same(plain.la, folded.la) and same(plain.adapt, folded.adapt) and bool((folded.count == 3).all())
    last = run(["update"] * 3 + ["last"], [None, "fold", "fold", "close"])
    assert same(last.adapt, run(["update"] * 3 + ["last"], None).adapt) and bool((last.adapt[:, 2] == 4).all())
    one = run(["update"] * 4, [None, None, None, "close"])   # a window of one state: the scale's bits are kept
    assert same(one.scale, ones) and not one.count.any()


@pytest.mark.parametrize("space", R.SPACES)
def test_the_windowed_metric_frees_the_step_from_the_stiffest_coordinate(space):
    seed = 11                                                # (a seed that is not one of those the bands were taken from)
    acc1, step1, dev1, rho1, tr = MR.experiment(seed, space, metric=True)
    acc0, step0, dev0, rho0, _ = MR.experiment(seed, space, metric=False)
    print(f"[hmc metric] {space}: warm-up {MR.EXP_W} + {MR.EXP_FROZEN} trajectories, B={MR.EXP_B}: with the metric frozen acceptance {acc1:.4f}, "
          f"median step {step1:.4f}, median |log(scale / closed form)| {dev1:.4f}, lag-1 autocorrelation of column 0 {rho1:+.3f}; step "
          f"adaptation alone: {acc0:.4f}, {step0:.4f}, (identity: {dev0:.4f}), {rho0:+.3f}")
    band = BAND[space]
    assert MR.BAND[space] == band
    assert band["accept"][0] <= acc1 <= band["accept"][1] and band["step"][0] <= step1 <= band["step"][1]
    assert band["scale"][0] <= dev1 <= band["scale"][1]
    assert step1 > step0                                     # a condition, not a measurement: the ratio is 16 - 17 in z, 5 - 6 in eps
    assert not tr.count.any() and bool((tr.adapt[:, 2] == MR.EXP_W - MR.EXP_WINDOWS[1][-1]).all())
    if space == "z":                                         # the closed form is z's: there the scales find it and the chain decorrelates
        assert dev1 < 0.25 * dev0 and step1 > 8.0 * step0 and rho1 < 0.2 < 0.7 < rho0


def test_cost_tool_is_a_driver_on_the_ab_harness():
    """tools/hmc_metric_vs_hmc_rows.py: its child's source is valid and importing the driver does not import torch."""
    import subprocess
    import sys
    tools = os.path.join(ROOT, "tools")
    code = ("import sys; sys.path.insert(0, %r)\nimport ab_harness, hmc_metric_vs_hmc_rows as t\n"
            "compile(ab_harness.PRELUDE + t.CHILD, 'child', 'exec')\nassert 'torch' not in sys.modules\n"
            "assert t.SIZES == (100, 16384)" % tools)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=60)

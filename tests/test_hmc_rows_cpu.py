"""CPU: the per-row step sizes of Hamiltonian Monte Carlo and their dual-averaging adaptation (`lsnf_hmc_step_rows`,
`lsnf_reverse_hmc_step_rows`, include/lsnf_flow_mcmc.h): the C declarations and the ctypes binding outside the core ABI, the Python
layers, every refusal the entry points make before any HIP call (fake 16-byte-aligned pointers that are never dereferenced, as
tests/test_rhmc_cpu.py), and the properties of the float64 restatement alone (tests/hmc_rows_restated.py).

The warm-up experiment (`hmc_rows_restated.warmup_run`: TINY flow prior plus the quadratic energy, 64 rows of which half start at
10 x and half at 0.1 x a sound step, L = 3, 60 adapting and 60 frozen trajectories) was run on the CPU at seeds 0 .. 7, for the chain
on z and for the one on eps (profiles/hmc_rows_cpu.txt).  z: frozen-phase mean acceptance 0.9247 .. 0.9339; one run's standard error
is sqrt(0.93 x 0.07 / 3840) = 0.0041, so BAND = (0.9247 - 3 SE, 0.9339 + 3 SE) = (0.912, 0.946); a half (1920 decisions, SE 0.0058,
observed 0.9177 .. 0.9391): BAND_HALF = (0.900, 0.957).  eps: 0.8872 .. 0.8997, SE 0.0050: (0.872, 0.915); a half 0.8844 .. 0.9036, SE
0.0071: (0.863, 0.925).  The bands lie ABOVE target_accept = 0.8 and say so: what a warm-up ends with is the AVERAGED log step, which
after 60 trajectories still carries the small early iterates (z, 150 trajectories: 0.91, 300: 0.87 -- the same file)."""
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
import hmc_rows_restated as R

import lsnf_amd

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2
INIT, INNER, ADAPT, LAST = 1, 2, 4, 8
NAMES = ("lsnf_hmc_step_rows", "lsnf_reverse_hmc_step_rows")
SCALAR = {"lsnf_hmc_step_rows": "lsnf_hmc_step", "lsnf_reverse_hmc_step_rows": "lsnf_reverse_hmc_step"}
COUNT = {"lsnf_hmc_step_rows": 29, "lsnf_reverse_hmc_step_rows": 27}      # (lsnf_hmc_step has 27 parameters, lsnf_reverse_hmc_step 25)
FAKE = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(24)]     # 16-byte aligned addresses that are never dereferenced on the host
BAND = {"z": (0.912, 0.946), "eps": (0.872, 0.915)}          # (the module docstring; hmc_rows_restated.BAND is held to it below)
BAND_HALF = {"z": (0.900, 0.957), "eps": (0.863, 0.925)}


def test_symbols_are_declared_exported_and_bound_outside_the_core_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow_mcmc.h")).read(), flags=re.S)
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    ext = lsnf_amd._lib._EXT_SIGNATURES
    assert len(re.findall(r"#define\s+LSNF_HMC_ADAPT\s+4u", hdr)) == 1 and len(re.findall(r"#define\s+LSNF_HMC_ADAPT_LAST\s+8u", hdr)) == 1
    assert re.search(r"typedef\s+struct\s+LsnfDualAvg\s*\{\s*float\s+target_accept,\s*gamma,\s*t0,\s*kappa,\s*step_min,\s*step_max;\s*\}\s*LsnfDualAvg;", hdr)
    assert [f for f, _ in lsnf_amd._lib.LsnfDualAvg._fields_] == ["target_accept", "gamma", "t0", "kappa", "step_min", "step_max"]
    assert ctypes.sizeof(lsnf_amd._lib.LsnfDualAvg) == 24
    decl = lambda name: [re.sub(r".*[\s*]", "", a.strip())
                         for a in re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1).split(",")]
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and name not in core and hasattr(lib, name)
        assert name in ext and len(ext[name][1]) == COUNT[name] and name not in lsnf_amd.exported_symbols() and name not in lsnf_amd._lib._SIGNATURES
        assert getattr(lib, name).argtypes == ext[name][1]               # attached in load()
        # the declaration's parameters: the scalar call's, `step_size` replaced by step_rows, adapt, da
        names, scalar = decl(name), decl(SCALAR[name])
        at = scalar.index("step_size")
        assert len(names) == COUNT[name] == len(scalar) + 2 and names == scalar[:at] + ["step_rows", "adapt", "da"] + scalar[at + 1:]
        args, sargs = ext[name][1], ext[SCALAR[name]][1]
        assert args[:at] == sargs[:at] and args[at + 3:] == sargs[at + 1:] and args[at:at + 2] == [ctypes.c_void_p, ctypes.c_void_p]
        assert args[at + 2] is ctypes.POINTER(lsnf_amd._lib.LsnfDualAvg)
    assert lsnf_amd._lib.extension_symbols() == sorted(ext)
    assert lib.lsnf_abi_version() == 5 and lsnf_amd._lib.ABI_VERSION == 5


def test_python_layers_exist_and_the_existing_ones_are_unchanged():
    F, L, M = lsnf_amd.flow, lsnf_amd.langevin, lsnf_amd.mcmc
    assert F.hmc_step_rows is M.hmc_step_rows and F.reverse_hmc_step_rows is M.reverse_hmc_step_rows
    assert F.HmcRowSteps is M.HmcRowSteps and F.new_hmc_row_steps is M.new_hmc_row_steps
    assert (F.HMC_ADAPT, F.HMC_ADAPT_LAST) == (4, 8)
    for new, old in ((F.hmc_step_rows, F.hmc_step), (F.reverse_hmc_step_rows, F.reverse_hmc_step),
                     (lsnf_amd._netF.hmc_step_rows, lsnf_amd._netF.hmc_step), (lsnf_amd._netF.reverse_hmc_step_rows, lsnf_amd._netF.reverse_hmc_step)):
        a, b = inspect.signature(new).parameters, inspect.signature(old).parameters
        assert [n for n in a] == [("steps" if n == "step_size" else n) for n in b] + ["adapt"]
        assert a["adapt"].kind is inspect.Parameter.KEYWORD_ONLY and a["adapt"].default is None
        for n in b:
            if n != "step_size":
                assert a[n].kind == b[n].kind and a[n].default == b[n].default
    assert [f for f in F.HmcRowSteps.__dataclass_fields__] == ["step", "adapt", "target_accept", "gamma", "t0", "kappa", "step_min", "step_max"]
    sig = inspect.signature(F.new_hmc_row_steps)
    assert list(sig.parameters) == ["B", "device", "step_size", "target_accept", "gamma", "t0", "kappa", "step_min", "step_max"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[3:]] == [0.8, 0.05, 10.0, 0.75, 1e-4, 1e2]
    for fn, first in ((L.sample_hmc_adaptive_post_z_with_flow, "z"), (L.sample_hmc_adaptive_post_eps_with_flow, "eps")):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == [first, "x", "netG", "netF", "g_l_steps", "leapfrog_steps", "warmup_steps", "g_l_step_size",
                                        "g_llhd_sigma", "philox", "target_accept", "steps"]
        for kw in list(sig.parameters)[4:]:
            assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
        assert sig.parameters["target_accept"].default == 0.8 and sig.parameters["steps"].default is None
    # the existing layers keep their signatures
    assert list(inspect.signature(F.hmc_step).parameters)[:7] == ["plan", "z_prop", "grad_g", "energy_g", "state", "noise", "step_size"]
    assert list(inspect.signature(F.reverse_hmc_step).parameters)[:9] == ["plan", "eps_prop", "z_saved", "act_saved", "grad_g", "energy_g", "state",
                                                                          "noise", "step_size"]
    assert list(inspect.signature(M._check_chain).parameters) == ["plan", "point", "name", "grad_g", "energy_g", "state", "state_cls", "noise",
                                                                  "uniform", "stash"]
    assert list(inspect.signature(L.sample_hmc_post_z_with_flow).parameters) == ["z", "x", "netG", "netF", "g_l_steps", "leapfrog_steps",
                                                                                "g_l_step_size", "g_llhd_sigma", "philox"]
    assert len(lsnf_amd._lib._EXT_SIGNATURES["lsnf_hmc_step"][1]) == 27 and len(lsnf_amd._lib._EXT_SIGNATURES["lsnf_reverse_hmc_step"][1]) == 25


def test_new_row_steps_fills_the_state():
    F = lsnf_amd.flow
    st = F.new_hmc_row_steps(5, "cpu", 0.25, target_accept=0.7)
    assert st.step.shape == (5,) and st.adapt.shape == (5, 4) and st.step.dtype == st.adapt.dtype == torch.float32
    assert bool((st.step == 0.25).all()) and bool((st.adapt[:, :3] == 0).all()) and torch.equal(st.adapt[:, 3], torch.log(10.0 * st.step))
    assert (st.target_accept, st.gamma, st.t0, st.kappa, st.step_min, st.step_max) == (0.7, 0.05, 10.0, 0.75, 1e-4, 1e2)
    rows = torch.tensor([0.1, 0.2, 0.4])
    st = F.new_hmc_row_steps(3, "cpu", rows)
    assert torch.equal(st.step, rows) and st.step.data_ptr() != rows.data_ptr() and torch.equal(st.adapt[:, 3], torch.log(10.0 * rows))
    with pytest.raises(lsnf_amd.LsnfError):
        F.new_hmc_row_steps(4, "cpu", rows)


# ---- the refusals of the two entry points ------------------------------------------------------------------------------------
Z_ARGS = ("plan", "point", "z_out", "saved", "act", "ll", "grad_g", "energy", "p_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")
E_ARGS = ("plan", "point", "saved", "act", "grad_g", "energy", "p_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")


def _caller(lib, name):
    Rng, Da = lsnf_amd._lib.LsnfRng, lsnf_amd._lib.LsnfDualAvg
    order = Z_ARGS if name == "lsnf_hmc_step_rows" else E_ARGS
    ptrs = dict(zip(order + ("step_rows", "adapt", "next", "accept", "la"), FAKE))
    base = dict(ptrs, nz=128, w=64, d=5, c=1, B=4, rng=None, da=None, adapt=None, flags=0, accept=None, la=None)
    fn = getattr(lib, name)

    def call(**kw):
        a = dict(base, **kw)
        return fn(a["plan"], a["nz"], a["w"], a["d"], a["c"], a["B"], *(a[k] for k in order[1:]),
                  None if a["rng"] is None else ctypes.byref(a["rng"]), a["step_rows"], a["adapt"],
                  None if a["da"] is None else ctypes.byref(a["da"]), a["flags"], a["next"], a["accept"], a["la"], None)

    def said(code, text, **kw):
        rc = call(**kw)
        return rc == code and lib.lsnf_last_error().decode() == name + ": " + text
    return call, said, ptrs, Rng, Da


@pytest.mark.parametrize("name", NAMES)
def test_every_new_rule_refuses_before_any_hip_call(name):
    lib = lsnf_amd.load_library()
    call, said, P, Rng, Da = _caller(lib, name)
    nxt = "z_next" if name == "lsnf_hmc_step_rows" else "eps_next"
    acc_name = "z_acc" if name == "lsnf_hmc_step_rows" else "eps_acc"
    good = lambda **kw: Da(**dict(dict(target_accept=0.8, gamma=0.05, t0=10.0, kappa=0.75, step_min=1e-4, step_max=1e2), **kw))
    adapting = dict(flags=ADAPT, adapt=P["adapt"], da=good())
    inner = dict(flags=INNER, noise=None, uniform=None)
    E = LSNF_E_ARG
    nan, inf = float("nan"), float("inf")
    for B in (0, 4):                                         # rules that precede the empty-batch return: the same answer for B = 0
        assert said(E, "unknown flag bits 0x10", B=B, flags=16) and said(E, "unknown flag bits 0x80000000", B=B, flags=0x80000000 | ADAPT)
        assert said(E, "flags: LSNF_HMC_INIT and LSNF_HMC_INNER exclude each other", B=B, flags=INIT | INNER, noise=None, uniform=None)
        only_end = "flags: LSNF_HMC_ADAPT goes with an end call (neither LSNF_HMC_INIT nor LSNF_HMC_INNER)"
        assert said(E, only_end, B=B, **dict(adapting, flags=ADAPT | INIT)) and said(E, only_end, B=B, **dict(adapting, **dict(inner, flags=ADAPT | INNER)))
        assert said(E, only_end, B=B, **dict(adapting, flags=ADAPT | LAST | INIT))
        assert said(E, "flags: LSNF_HMC_ADAPT_LAST goes with LSNF_HMC_ADAPT", B=B, flags=LAST)
        assert said(E, "flags: LSNF_HMC_ADAPT_LAST goes with LSNF_HMC_ADAPT", B=B, flags=LAST | INIT)
        assert said(E, "da is required with LSNF_HMC_ADAPT", B=B, flags=ADAPT, adapt=P["adapt"])
        assert said(E, "adapt and da must be NULL without LSNF_HMC_ADAPT", B=B, adapt=P["adapt"])
        assert said(E, "adapt and da must be NULL without LSNF_HMC_ADAPT", B=B, da=good())
        assert said(E, "adapt and da must be NULL without LSNF_HMC_ADAPT", B=B, da=good(), **inner)
        for field in ("target_accept", "gamma", "t0", "kappa", "step_min", "step_max"):
            for bad, word in ((nan, "nan"), (inf, "inf"), (-inf, "-inf")):
                assert said(E, f"da: every field must be finite (got {word})", B=B, **dict(adapting, da=good(**{field: bad})))
        for bad in (0.0, 1.0, -0.2, 1.5):
            assert said(E, f"da->target_accept must lie in (0, 1) (got {bad:g})", B=B, **dict(adapting, da=good(target_accept=bad)))
        for bad in (0.0, -0.05):
            assert said(E, f"da->gamma must be positive (got {bad:g})", B=B, **dict(adapting, da=good(gamma=bad)))
            assert said(E, f"da->step_min must be positive (got {bad:g})", B=B, **dict(adapting, da=good(step_min=bad)))
        for bad in (-1.0, -3.0):
            assert said(E, f"da->t0 + 1 must be positive (got t0 = {bad:g})", B=B, **dict(adapting, da=good(t0=bad)))
        assert said(E, "da->step_max must not be below da->step_min (got 0.5 < 1)", B=B, **dict(adapting, da=good(step_min=1.0, step_max=0.5)))
        # step_rows and adapt alias nothing else the call touches
        assert said(E, "step_rows must not alias grad_g", B=B, step_rows=P["grad_g"]) and said(E, "step_rows must not alias uniform", B=B, step_rows=P["uniform"])
        assert said(E, f"{acc_name} must not alias step_rows", B=B, step_rows=P["p_acc"]) and said(E, "kin0 must not alias step_rows", B=B, step_rows=P["kin0"])
        assert said(E, f"{nxt} must not alias step_rows", B=B, step_rows=P["next"])
        assert said(E, "adapt must not alias energy_g", B=B, **dict(adapting, adapt=P["energy"]))
        assert said(E, "mom must not alias adapt", B=B, **dict(adapting, adapt=P["mom"]))
        assert said(E, "step_rows must not alias adapt", B=B, **dict(adapting, adapt=P["step_rows"]))
        # the scalar call's rules, word for word (a sample: the whole table is tests/test_hmc_cpu.py's and tests/test_rhmc_cpu.py's)
        assert said(E, "pass either a uniform tensor or an rng, not both", B=B, noise=None, rng=Rng(1, 0, None, 0))
        assert said(E, "rng->row0 must be >= 0", B=B, noise=None, uniform=None, rng=Rng(1, 0, None, -1))
        assert said(E, "noise is not taken with LSNF_HMC_INNER (an inner step draws nothing)", B=B, flags=INNER, uniform=None)
        assert said(E, f"{nxt} must not alias mom", B=B, mom=P["next"])
    assert said(LSNF_E_GEOMETRY, "unsupported geometry nz=130 width=64 depth=5 coupling=1 (need nz even in [2,128], width in [1,128], "
                "depth in [1,16], coupling 0 or 1)", nz=130) or b"unsupported geometry" in lib.lsnf_last_error()
    assert call(nz=130) == LSNF_E_GEOMETRY and call(nz=130, B=0) == LSNF_E_GEOMETRY and said(E, "B=-1 out of range", B=-1)
    # an empty batch: nothing to launch, NULL pointers allowed, in every phase and with adaptation on
    nulls = {k: None for k in P}
    assert call(B=0, **nulls) == LSNF_OK and call(B=0, **dict(nulls, flags=INNER)) == LSNF_OK and call(B=0, **dict(nulls, flags=INIT)) == LSNF_OK
    assert call(B=0, **dict(nulls, flags=ADAPT, da=good())) == LSNF_OK and call(B=0, **dict(nulls, flags=ADAPT | LAST, da=good())) == LSNF_OK
    assert call(B=0, **adapting) == LSNF_OK and call(B=0, **{"next": P["point"]}) == LSNF_OK
    # the pointers of a non-empty call
    for extra in (dict(), inner, dict(flags=INIT), adapting):
        assert said(E, "step_rows is required (NULL)", **dict(extra, step_rows=None))
        assert said(E, "mom is required (NULL)", **dict(extra, mom=None))
    assert said(E, "adapt is required with LSNF_HMC_ADAPT", flags=ADAPT, da=good()) and said(E, "adapt is required with LSNF_HMC_ADAPT", flags=ADAPT | LAST, da=good())
    assert said(E, "adapt must be 16-byte aligned", **dict(adapting, adapt=ctypes.c_void_p(0xF00008)))
    assert said(E, "adapt must be 4-byte aligned", **dict(adapting, adapt=ctypes.c_void_p(0xF00002)))
    assert said(E, "step_rows must be 4-byte aligned", step_rows=ctypes.c_void_p(0xF00002))
    assert said(E, "step_rows must be 4-byte aligned", **dict(inner, step_rows=ctypes.c_void_p(0xF00002)))
    assert said(E, "plan must be 16-byte aligned", plan=ctypes.c_void_p(0x10004)) and said(E, "act_saved must be 16-byte aligned", act=ctypes.c_void_p(0x50008))
    assert said(E, "uniform is required without an rng (unless LSNF_HMC_INIT or LSNF_HMC_INNER)", uniform=None)
    assert said(E, f"noise is required with {nxt} when no rng is given", noise=None)
    assert said(E, f"{nxt} is required (NULL) with LSNF_HMC_INNER", **dict(inner, **{"next": None}))
    # (no step_size rule: the steps are device memory.  The next rule -- a misaligned act_saved -- is what refuses a call that passed all others)
    bad_act = ctypes.c_void_p(0x50008)
    for ok in (adapting, dict(adapting, flags=ADAPT | LAST), dict(adapting, noise=None, **{"next": None}), inner, dict(flags=INIT, uniform=None),
               dict(noise=None, uniform=None, rng=Rng(1, 0, None, 0)), dict(adapting, noise=None, uniform=None, rng=Rng(1, 0, None, 0)),
               dict(adapting, da=good(t0=-0.5)), dict(adapting, da=good(step_min=0.3, step_max=0.3)), dict(adapting, da=good(kappa=-1.0))):
        assert said(E, "act_saved must be 16-byte aligned", **dict(ok, act=bad_act))


def test_python_wrappers_speak_on_cpu_tensors(monkeypatch):
    from counting_lib import install
    F, L = lsnf_amd.flow, lsnf_amd.langevin
    lib = lsnf_amd.load_library()
    plan = F.FlowPlan(8, 4, 2, 1, torch.zeros(lib.lsnf_plan_floats(8, 4, 2, 1)), torch.zeros(lib.lsnf_prepare_scratch_bytes(8, 4, 2) // 8, dtype=torch.float64))
    stand = install(monkeypatch, lsnf_amd)
    seen = []
    real = lsnf_amd.mcmc._check_chain

    def spy(*a, **k):
        seen.append(k.get("stash"))
        return real(*a, **k)
    monkeypatch.setattr(lsnf_amd.mcmc, "_check_chain", spy)
    z, v, saved = torch.zeros(5, 8), torch.zeros(5), torch.zeros(1, 5, 8)
    act = torch.zeros(lib.lsnf_act_saved_floats(8, 4, 2, 5))
    steps, state = F.new_hmc_row_steps(5, "cpu", 0.5), F.new_hmc_state(plan, 5, "cpu")
    zcall = lambda steps=steps, **kw: F.hmc_step_rows(plan, z, None, None, state, F.PhiloxNoise(3), steps, **kw)
    ecall = lambda steps=steps, **kw: F.reverse_hmc_step_rows(plan, z, saved, act, None, None, state, F.PhiloxNoise(3), steps, **kw)
    for call in (zcall, ecall):
        n = len(seen)
        with pytest.raises(lsnf_amd.LsnfError, match="phase must be one of"):
            call(phase="middle")
        with pytest.raises(lsnf_amd.LsnfError, match=r"steps must be a flow.HmcRowSteps \(new_hmc_row_steps\(\)\)"):
            call(steps=0.5)
        with pytest.raises(lsnf_amd.LsnfError, match="adapt must be None, 'update' or 'last'"):
            call(adapt="yes")
        for phase in ("init", "inner"):
            with pytest.raises(lsnf_amd.LsnfError, match="adapt goes with phase='end'"):
                call(phase=phase, adapt="update")
        assert len(seen) == n                                # (refused before the tensors are looked at)
        for kw in (dict(), dict(adapt="update"), dict(adapt="last", propose=False), dict(phase="init")):
            with pytest.raises(lsnf_amd.LsnfError, match="no CPU path"):
                call(**kw)
        assert len(seen) == n + 4                            # every such call went through _check_chain
    assert all(st is None for st in seen[:4]) and all(st is not None and st[0] is saved and st[1] is act for st in seen[4:])
    # the two arrays of `steps` go through the one checking path
    with pytest.raises(lsnf_amd.LsnfError, match="steps.step must live on"):
        lsnf_amd.mcmc._row_step_args(steps, 5, torch.device("cuda:0"), None)
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    with pytest.raises(lsnf_amd.LsnfError):
        net.hmc_step_rows(z, None, None, state, F.PhiloxNoise(1), steps, phase="init")
    with pytest.raises(lsnf_amd.LsnfError):
        net.reverse_hmc_step_rows(z, saved, act, None, None, state, F.PhiloxNoise(1), steps, phase="init")
    # the samplers: their own rules, then the wrappers'; nothing to do returns the input without a launch
    x, G = torch.zeros(5, 8), torch.nn.Flatten()
    kw = dict(g_l_step_size=0.5, g_llhd_sigma=0.3)
    for fn in (L.sample_hmc_adaptive_post_z_with_flow, L.sample_hmc_adaptive_post_eps_with_flow):
        with pytest.raises(ValueError, match="leapfrog_steps"):
            fn(z, x, G, net, g_l_steps=2, leapfrog_steps=0, warmup_steps=0, philox=F.PhiloxNoise(1), **kw)
        for bad in (-1, 3):
            with pytest.raises(ValueError, match="warmup_steps"):
                fn(z, x, G, net, g_l_steps=2, leapfrog_steps=2, warmup_steps=bad, philox=F.PhiloxNoise(1), **kw)
        with pytest.raises(lsnf_amd.LsnfError, match="steps must be a flow.HmcRowSteps"):
            fn(z, x, G, net, g_l_steps=2, leapfrog_steps=2, warmup_steps=1, philox=F.PhiloxNoise(1), steps=0.5, **kw)
        with pytest.raises(lsnf_amd.LsnfError):
            fn(z, x, G, net, g_l_steps=2, leapfrog_steps=2, warmup_steps=1, philox=F.PhiloxNoise(1), **kw)
        ph = F.PhiloxNoise(5, 100)
        none = fn(z.view(5, 8, 1, 1), x, G, net, g_l_steps=0, leapfrog_steps=2, warmup_steps=0, philox=ph, steps=steps, **kw)
        assert torch.equal(none[0].reshape(5, 8), z) and all(t is None for t in none[1:-1]) and none[-1] is steps and ph.offset == 100
        empty = fn(z[:0], x[:0], G, net, g_l_steps=4, leapfrog_steps=2, warmup_steps=2, philox=ph, **kw)
        assert empty[0].shape[0] == 0 and empty[-2] is None and empty[-1] is None and ph.offset == 100
    assert stand.launching() == [], dict(stand.entered)


# ---- the restatement alone -------------------------------------------------------------------------------------------------
def _setup(nz=8, w=4, depth=5, B=24, seed=5, T=3):
    p = O.init_params(nz, w, depth, seed=3)
    quad = H.Quadratic(nz, 0.1, seed=7 + nz)
    g = torch.Generator().manual_seed(seed)
    z0, _ = O.smooth_batch(p, B, nz, seed=1000 + seed)
    noises = [torch.randn(B, nz, generator=g) for _ in range(T)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g).clamp_min(2.0 ** -25) for _ in range(T)]
    return p, quad, z0, noises, uniforms, g


def test_one_step_for_all_rows_is_the_scalar_chain():
    p, quad, z0, noises, uniforms, g = _setup()
    s, L = float(torch.tensor(1.2, dtype=torch.float32)), 3
    clone = lambda xs: [None if x is None else x.clone() for x in xs]
    n1, n2 = clone(noises), clone(noises)
    calls, state = H.chain(p, z0, quad, s, L, n1, uniforms, redraw=torch.Generator().manual_seed(9))
    tr = R.chain(p, z0, quad, torch.full((z0.shape[0],), s, dtype=torch.float64), L, n2, uniforms, redraw=torch.Generator().manual_seed(9))
    ends = [c for c in calls if c.phase == "end"]
    assert torch.equal(tr.la, torch.stack([c.la for c in ends])) and torch.equal(tr.acc, torch.stack([c.acc for c in ends]))
    assert all(torch.equal(a, b) for a, b in zip(tr.state, state)) and all(torch.equal(a, b) for a, b in zip(n1[:-1], n2[:-1]))
    assert bool((tr.steps == s).all()) and 0 < int(tr.acc.sum()) < tr.acc.numel()
    # a row's chain is its own: rows at another step leave the rows at s alone
    mixed = torch.full((z0.shape[0],), s, dtype=torch.float64)
    mixed[1::2] = 0.5 * s
    tr2 = R.chain(p, z0, quad, mixed, L, clone(noises), uniforms)
    tr1 = R.chain(p, z0, quad, torch.full_like(mixed, s), L, clone(noises), uniforms)
    assert torch.equal(tr2.la[:, 0::2], tr1.la[:, 0::2]) and not torch.equal(tr2.la[:, 1::2], tr1.la[:, 1::2])


def test_dual_averaging_update():
    da = R.DualAvg()
    B = 6
    step = torch.tensor([0.1, 0.5, 1.0, 2.0, 0.01, 30.0], dtype=torch.float64)
    la = torch.tensor([-0.3, 0.2, float("nan"), float("inf"), -float("inf"), -2.0], dtype=torch.float64)
    ad0 = R.new_adapt(step)
    assert bool((ad0[:, :3] == 0).all()) and torch.equal(ad0[:, 3], torch.log(10.0 * step))
    for last in (False, True):
        ad, s1 = R.dual_average(ad0, la, da, last)
        # count = 0: w = 1, so the average IS the first iterate, and "last" writes the same step
        assert torch.equal(ad[:, 0], torch.log(s1)) or bool(((ad[:, 0] - torch.log(s1)).abs() <= 1e-15).all())
        assert torch.equal(ad[:, 2], torch.ones(B, dtype=torch.float64)) and torch.equal(ad[:, 3], ad0[:, 3])
        a = torch.tensor([float(torch.exp(torch.tensor(-0.3, dtype=torch.float64))), 1.0, 0.0, 1.0, 0.0, float(torch.exp(torch.tensor(-2.0, dtype=torch.float64)))],
                         dtype=torch.float64)                # (a NaN log_alpha counts as a rejection, +inf as an acceptance)
        assert bool(((ad[:, 1] - (float(torch.tensor(0.8)) - a) / 11.0).abs() <= 1e-15).all())      # (target_accept: the fp32 value the kernel gets)
    # the float32 restatement follows the float64 one to fp32 rounding of the magnitudes involved
    ad64, s64 = R.dual_average(ad0, la, da, False)
    ad32, s32 = R.dual_average(ad0.float(), la.float(), da, False, dtype=torch.float32)
    assert ad32.dtype == torch.float32 and bool(((ad32.double() - ad64).abs() <= 1e-6 * R.update_scale(ad64, da)[:, None]).all())
    assert bool(((s32.double() - s64).abs() <= 1e-5 * s64).all())
    # a row that always accepts grows to step_max, one that never does shrinks to step_min; both stay finite, pinned there
    for la_const, pin in ((torch.full((B,), 5.0, dtype=torch.float64), da.step_max), (torch.full((B,), float("nan"), dtype=torch.float64), da.step_min)):
        ad = ad0
        for k in range(400):
            ad, s = R.dual_average(ad, la_const, da, False)
        assert bool(torch.isfinite(ad).all()) and bool(((s - pin).abs() <= 1e-6 * pin).all())
        ad, s = R.dual_average(ad, la_const, da, True)       # the averaged step lies between the first step's neighbourhood and the pin
        assert bool(torch.isfinite(s).all()) and bool((s >= da.step_min * (1 - 1e-6)).all()) and bool((s <= da.step_max * (1 + 1e-6)).all())
    # fp32 at the pins: finite too
    ad = ad0.float()
    for k in range(400):
        ad, s = R.dual_average(ad, torch.full((B,), float("nan")), da, False, dtype=torch.float32)
    assert bool(torch.isfinite(ad).all()) and bool(((s.double() - da.step_min).abs() <= 1e-5 * da.step_min).all())


def test_a_rows_update_uses_its_own_decision_and_comes_after_it():
    """An adapting end call decides with the step the trajectory ran at; the new step is what the NEXT trajectory runs at."""
    p, quad, z0, noises, uniforms, g = _setup(T=2)
    B = z0.shape[0]
    step = torch.full((B,), 1.2, dtype=torch.float64)
    clone = lambda xs: [None if x is None else x.clone() for x in xs]
    plain = R.chain(p, z0, quad, step, 3, clone(noises), uniforms)
    adapted = R.chain(p, z0, quad, step, 3, clone(noises), uniforms, da=R.DualAvg(), modes=["update", None])
    assert torch.equal(adapted.la[0], plain.la[0]) and torch.equal(adapted.acc[0], plain.acc[0])        # the first decision: the old step's
    ad, s1 = R.dual_average(R.new_adapt(step), plain.la[0], R.DualAvg(), False)
    assert torch.equal(adapted.steps[0], step) and torch.equal(adapted.steps[1], s1) and torch.equal(adapted.steps[2], s1)
    assert torch.equal(adapted.adapt, ad) and not torch.equal(adapted.la[1], plain.la[1])


@pytest.mark.parametrize("space", R.SPACES)
def test_warm_up_brings_rows_from_both_sides_into_the_band(space):
    # without adaptation the two halves sit at the two ends: 10 x the sound step accepts (almost) nothing, 0.1 x (almost) everything
    nz, B = R.WARMUP_GEO[0], R.WARMUP_B
    p, quad = R.warmup_target(space)
    g = torch.Generator().manual_seed(1)
    z0, _ = O.smooth_batch(p, B, nz, seed=2000)
    T = 6
    noises = [torch.randn(B, nz, generator=g, dtype=torch.float64) for _ in range(T)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g, dtype=torch.float64).clamp_min(2.0 ** -25) for _ in range(T)]
    fixed = R.chain(p, z0, quad, R.warmup_start(space), R.WARMUP_L, noises, uniforms, space=space).acc.double()
    assert fixed[:, 0::2].mean().item() < 0.05 and fixed[:, 1::2].mean().item() > 0.99
    rate, (big, small), steps = R.warmup_run(seed=11, space=space)      # (a seed that is not one of those the band was taken from)
    print(f"[hmc rows] {space}: warm-up {R.WARMUP_K} + {R.FROZEN_K} trajectories, B={B}: frozen-phase acceptance {rate:.4f} "
          f"(rows started at 10 x: {big:.4f}, at 0.1 x: {small:.4f}), frozen steps {steps.min():.3f} .. {steps.max():.3f}")
    band, half, sound = BAND[space], BAND_HALF[space], R.SOUND_STEP[space]
    assert R.BAND[space] == band and R.BAND_HALF[space] == half and band[0] <= rate <= band[1]
    assert half[0] <= big <= half[1] and half[0] <= small <= half[1]
    assert bool((steps > 0.1 * sound).all()) and bool((steps < 10.0 * sound).all())


def test_cost_tool_is_a_driver_on_the_ab_harness():
    """tools/hmc_rows_vs_hmc_step.py: its child's source is valid and importing the driver does not import torch."""
    import subprocess
    import sys
    tools = os.path.join(ROOT, "tools")
    code = ("import sys; sys.path.insert(0, %r)\nimport ab_harness, hmc_rows_vs_hmc_step as t\n"
            "compile(ab_harness.PRELUDE + t.CHILD, 'child', 'exec')\nassert 'torch' not in sys.modules\n"
            "assert t.SIZES == (100, 16384)" % tools)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=60)

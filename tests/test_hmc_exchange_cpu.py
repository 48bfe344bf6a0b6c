"""CPU: replica exchange (parallel tempering) for the tempered HMC steps (`lsnf_hmc_step_exchange`, `lsnf_reverse_hmc_step_exchange`,
include/lsnf_flow_mcmc.h): the C declarations and the ctypes binding outside the core ABI, the Python layers, every refusal the swap
adds pinned through the entry points' own check before any HIP call (fake aligned pointers that are never dereferenced, as
tests/test_hmc_tempered_cpu.py), the pairing's edges, the ladder's end points, and one statistical check of the float64 restatement
(tests/hmc_exchange_restated.py).

The statistical check: ais_restated's affine TINY flow is a Gaussian prior, `hmc_exchange_restated.TwoMode` a likelihood with two
quadratic wells 3.0 apart along the stiffest coordinate (a = 3.0: a well's posterior standard deviation there is 0.32), so the
posterior is a mixture of two Gaussians whose weights have a closed form, W_1 = Z_1 / (Z_1 + Z_2) = 0.156.  N = 32 ladders of R = 4
rungs (beta = 0.02 .. 1, geometric) start in well 1 and run K = 150 trajectories of L = 3 steps, every end call swapping, even / odd
alternating.  The beta = 1 rung's occupancy of well 1 over the last 4/5 of the run is compared with W_1.  The margin is a binomial
standard error of the n = N * (K - K / 5) = 3840 samples times FACTOR = 5: the factor stands for the samples' autocorrelation (a
ladder's successive states are not independent; 5 standard errors of independent samples are 2.5 of samples with an integrated
autocorrelation time of 4).  Chosen on the CPU: at generator seeds 0, 1, 2 the occupancy was off by -1.9, -0.1 and +3.7 of those
standard errors with swaps (seed 1 is the test's), and by more than +90 without: the chains never leave the well they start in."""
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
import hmc_exchange_restated as X
import hmc_tempered_restated as TR

import lsnf_amd

LSNF_OK, LSNF_E_ARG = 0, -1
INIT, INNER, ADAPT, LAST, FOLD, CLOSE, ANNEAL, SWAP, ODD = 1, 2, 4, 8, 16, 32, 64, 128, 256
NAMES = ("lsnf_hmc_step_exchange", "lsnf_reverse_hmc_step_exchange")
TEMPERED = {"lsnf_hmc_step_exchange": "lsnf_hmc_step_tempered", "lsnf_reverse_hmc_step_exchange": "lsnf_reverse_hmc_step_tempered"}
COUNT = {"lsnf_hmc_step_exchange": 43, "lsnf_reverse_hmc_step_exchange": 41}
FOUR = ["ladder", "swap_uniform", "swap_out", "log_swap_out"]
FAKE = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(40)]     # 16-byte aligned addresses that are never dereferenced on the host


def test_symbols_are_declared_exported_and_bound_outside_the_core_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow_mcmc.h")).read(), flags=re.S)
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    ext = lsnf_amd._lib._EXT_SIGNATURES
    assert len(re.findall(r"#define\s+LSNF_HMC_SWAP\s+128u", hdr)) == 1 and len(re.findall(r"#define\s+LSNF_HMC_SWAP_ODD\s+256u", hdr)) == 1
    decl = lambda name: [re.sub(r".*[\s*]", "", a.strip())
                         for a in re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1).split(",")]
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and name not in core and hasattr(lib, name)
        assert name in ext and len(ext[name][1]) == COUNT[name] and name not in lsnf_amd.exported_symbols() and name not in lsnf_amd._lib._SIGNATURES
        assert getattr(lib, name).argtypes == ext[name][1]               # attached in load()
        # the declaration's parameters: the tempered call's with the four inserted in front of stream
        names, tempered = decl(name), decl(TEMPERED[name])
        assert tempered[-1] == "stream" and names == tempered[:-1] + FOUR + ["stream"] and len(names) == COUNT[name]
        args, targs = ext[name][1], ext[TEMPERED[name]][1]
        assert args[:len(targs) - 1] == targs[:-1] and args[-1] == targs[-1]
        assert args[-5:-1] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        assert len(targs) == COUNT[name] - 4                 # the tempered declarations are what they were
    assert lsnf_amd._lib.extension_symbols() == sorted(ext)
    assert lib.lsnf_abi_version() == 5 and lsnf_amd._lib.ABI_VERSION == 5


def test_python_layers_exist():
    F, L, M = lsnf_amd.flow, lsnf_amd.langevin, lsnf_amd.mcmc
    assert F.hmc_step_exchange is M.hmc_step_exchange and F.reverse_hmc_step_exchange is M.reverse_hmc_step_exchange
    assert (F.HMC_SWAP, F.HMC_SWAP_ODD) == (M.HMC_SWAP, M.HMC_SWAP_ODD) == (128, 256)
    for new, old in ((F.hmc_step_exchange, F.hmc_step_tempered), (F.reverse_hmc_step_exchange, F.reverse_hmc_step_tempered),
                     (lsnf_amd._netF.hmc_step_exchange, lsnf_amd._netF.hmc_step_tempered),
                     (lsnf_amd._netF.reverse_hmc_step_exchange, lsnf_amd._netF.reverse_hmc_step_tempered)):
        a, b = inspect.signature(new).parameters, inspect.signature(old).parameters
        assert [n for n in a] == [n for n in b] + ["swap", "ladder", "swap_uniform"]
        for n in ("swap", "ladder", "swap_uniform"):
            assert a[n].kind is inspect.Parameter.KEYWORD_ONLY
        assert a["swap"].default is None and a["swap_uniform"].default is None
        for n in b:
            assert a[n].kind == b[n].kind and a[n].default == b[n].default
    for fn in (L.sample_hmc_pt_post_z_with_flow, L.sample_hmc_pt_post_eps_with_flow):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[1:] == ["x", "netG", "netF", "betas", "g_l_steps", "leapfrog_steps", "g_l_step_size", "g_llhd_sigma", "philox",
                                            "swap_every", "steps", "metric"]
        for kw in list(sig.parameters)[4:]:
            assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
        assert sig.parameters["swap_every"].default == 1 and sig.parameters["steps"].default is None and sig.parameters["metric"].default is None
        for said in ("philox.step(0)", "philox.step(t)", "K + 1", "counter field 3"):
            assert said in fn.__doc__
    assert list(inspect.signature(L.pt_ladder).parameters) == ["R", "beta_min"]
    # the tempered layers keep their signatures
    assert list(inspect.signature(F.hmc_step_tempered).parameters)[-1] == "anneal"
    assert len(lsnf_amd._lib._EXT_SIGNATURES["lsnf_hmc_step_tempered"][1]) == 39


def test_pairs_cover_the_edges():
    assert X.pairs(2, "even") == [(0, 1)] and X.pairs(2, "odd") == []
    assert X.pairs(4, "even") == [(0, 1), (2, 3)] and X.pairs(4, "odd") == [(1, 2)]
    assert X.pairs(16, "even") == [(a, a + 1) for a in range(0, 16, 2)] and X.pairs(16, "odd") == [(a, a + 1) for a in range(1, 14, 2)]
    for R in X.LADDERS:
        for parity in ("even", "odd"):
            ps = X.pairs(R, parity)
            used = [r for p in ps for r in p]
            assert len(set(used)) == len(used)               # a rung has at most one partner
            idle = sorted(set(range(R)) - set(used))
            assert idle == ([] if parity == "even" else sorted({0, R - 1}))
            prt = X.partner(3 * R, R, parity)
            rows = torch.arange(3 * R)
            assert torch.equal(prt[prt], rows) and bool((prt // R == rows // R).all())      # an involution inside the ladder
            assert bool(((prt - rows).abs() <= 1).all())
            assert sorted((rows[prt == rows] % R).unique().tolist()) == idle
    # B = 32, R = 16: no pair crosses rows 15 | 16
    for parity in ("even", "odd"):
        prt = X.partner(32, 16, parity)
        assert prt[15].item() in (14, 15) and prt[16].item() in (16, 17)


def test_exchange_lines_on_a_hand_made_pair():
    f64 = torch.float64
    beta = torch.tensor([0.25, 1.0, 0.5, 2.0], dtype=f64)
    z, g, gl = (torch.arange(8, dtype=f64).view(4, 2) + k for k in (0.0, 10.0, 20.0))
    u, el = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=f64), torch.tensor([5.0, 3.0, 1.0, 4.0], dtype=f64)
    prt = X.partner(4, 4, "even")
    lr = X.log_ratio(beta, el, prt)
    assert torch.equal(lr, torch.tensor([(0.25 - 1.0) * 2.0, (0.25 - 1.0) * 2.0, (0.5 - 2.0) * -3.0, (0.5 - 2.0) * -3.0], dtype=f64))
    sw = X.decide(lr, torch.tensor([0.5, 0.0, 0.5, 0.0], dtype=f64), prt)      # log 0.5 = -0.69: -1.5 rejects, +4.5 swaps
    assert sw.tolist() == [False, False, True, True]
    z2, g2, u2, gl2, el2 = X.exchange(beta, z, g, u, gl, el, prt, sw)
    assert torch.equal(z2[:2], z[:2]) and torch.equal(g2[:2], g[:2]) and torch.equal(u2[:2], u[:2])
    assert torch.equal(z2[2], z[3]) and torch.equal(z2[3], z[2]) and torch.equal(gl2[2], gl[3]) and el2.tolist() == [5.0, 3.0, 4.0, 1.0]
    assert torch.equal(g2[2], g[3] + (0.5 - 2.0) * gl[3]) and torch.equal(g2[3], g[2] + (2.0 - 0.5) * gl[2])
    assert u2[2].item() == 4.0 + (0.5 - 2.0) * 4.0 and u2[3].item() == 3.0 + (2.0 - 0.5) * 1.0
    # the potential at a row's own beta is what a fresh evaluation of the partner's state gives: u = prior + beta el
    prior = u - beta * el
    assert torch.allclose(u2[2:], prior[[3, 2]] + beta[2:] * el[[3, 2]], rtol=0, atol=1e-14)
    odd = X.partner(4, 4, "odd")
    assert X.log_ratio(beta, el, odd).tolist() == [0.0, (1.0 - 0.5) * (3.0 - 1.0), (1.0 - 0.5) * (3.0 - 1.0), 0.0]
    assert not X.decide(torch.full((4,), float("nan"), dtype=f64), torch.full((4,), 1e-9, dtype=f64), prt).any()


def test_pt_ladder_end_points_are_exact():
    L = lsnf_amd.langevin
    for R in (2, 4, 8, 16):
        for bmin in (0.02, 0.1, 1.0 / 3.0, 0.0):
            b = L.pt_ladder(R, bmin)
            assert b.dtype == torch.float64 and b.shape == (R,)
            assert b[0].item() == bmin and b[-1].item() == 1.0
            assert bool((b[1:] > b[:-1]).all())
            if bmin > 0.0 and R > 2:                         # geometric: a constant ratio
                ratio = b[1:] / b[:-1]
                assert bool(((ratio / ratio[0] - 1.0).abs() <= 1e-12).all())
    assert L.pt_ladder(4, 0.0).tolist() == [0.0, 0.25, 0.5, 1.0]
    for bad in (3, 1, 32):
        with pytest.raises(ValueError, match="R must be 2, 4, 8 or 16"):
            L.pt_ladder(bad, 0.1)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="beta_min must lie in"):
            L.pt_ladder(4, bad)


# ---- the refusals of the two entry points ------------------------------------------------------------------------------------
Z_ARGS = ("plan", "point", "z_out", "saved", "act", "ll", "grad_g", "energy", "p_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")
E_ARGS = ("plan", "point", "saved", "act", "grad_g", "energy", "p_acc", "g_acc", "u_acc", "mom", "kin0", "noise", "uniform")


def _caller(lib, name):
    Rng, Da, Reg = lsnf_amd._lib.LsnfRng, lsnf_amd._lib.LsnfDualAvg, lsnf_amd._lib.LsnfMetricReg
    order = Z_ARGS if name == "lsnf_hmc_step_exchange" else E_ARGS
    ptrs = dict(zip(order + ("step_rows", "adapt", "scale", "mean", "m2", "count", "beta", "beta_next", "like_grad", "like_u", "log_w", "next",
                             "accept", "la", "swap_uniform", "swap_out", "log_swap_out"), FAKE))
    base = dict(ptrs, nz=128, w=64, d=5, c=1, B=16, rng=None, da=None, adapt=None, mean=None, m2=None, count=None, reg=None, beta_next=None,
                log_w=None, flags=0, accept=None, la=None, ladder=0, swap_uniform=None, swap_out=None, log_swap_out=None)
    fn = getattr(lib, name)

    def call(**kw):
        a = dict(base, **kw)
        return fn(a["plan"], a["nz"], a["w"], a["d"], a["c"], a["B"], *(a[k] for k in order[1:]),
                  None if a["rng"] is None else ctypes.byref(a["rng"]), a["step_rows"], a["adapt"],
                  None if a["da"] is None else ctypes.byref(a["da"]), a["scale"], a["mean"], a["m2"], a["count"],
                  None if a["reg"] is None else ctypes.byref(a["reg"]), a["beta"], a["beta_next"], a["like_grad"], a["like_u"], a["log_w"],
                  a["flags"], a["next"], a["accept"], a["la"], a["ladder"], a["swap_uniform"], a["swap_out"], a["log_swap_out"], None)

    def said(code, text, **kw):
        rc = call(**kw)
        return rc == code and lib.lsnf_last_error().decode() == name + ": " + text
    return call, said, ptrs, Rng, Da, Reg


@pytest.mark.parametrize("name", NAMES)
def test_every_new_rule_refuses_before_any_hip_call(name):
    lib = lsnf_amd.load_library()
    call, said, P, Rng, Da, Reg = _caller(lib, name)
    z = name == "lsnf_hmc_step_exchange"
    nxt, point = ("z_next", "z_prop") if z else ("eps_next", "eps_prop")
    da = Da(target_accept=0.8, gamma=0.05, t0=10.0, kappa=0.75, step_min=1e-4, step_max=1e2)
    reg = Reg(n0=5.0, var0=1e-3, scale_min=1e-3, scale_max=1e3)
    swapping = dict(flags=SWAP, ladder=4, swap_uniform=P["swap_uniform"], swap_out=P["swap_out"], log_swap_out=P["log_swap_out"])
    annealing = dict(beta_next=P["beta_next"], log_w=P["log_w"])
    folding = dict(mean=P["mean"], m2=P["m2"], count=P["count"], reg=reg)
    adapting = dict(adapt=P["adapt"], da=da)
    philox = dict(noise=None, uniform=None, rng=Rng(1, 0, None, 0))
    E = LSNF_E_ARG
    for B in (0, 16):                                        # rules that precede the empty-batch return: the same answer for B = 0
        assert said(E, "unknown flag bits 0x200", B=B, **dict(swapping, flags=SWAP | 0x200))
        assert said(E, "flags: LSNF_HMC_SWAP_ODD goes with LSNF_HMC_SWAP", B=B, flags=ODD)
        assert said(E, "flags: LSNF_HMC_SWAP_ODD goes with LSNF_HMC_SWAP", B=B, flags=ODD | INIT, uniform=None)
        end_only = "flags: LSNF_HMC_SWAP goes with an end call (neither LSNF_HMC_INIT nor LSNF_HMC_INNER)"
        assert said(E, end_only, B=B, **dict(swapping, flags=SWAP | INIT, uniform=None))
        assert said(E, end_only, B=B, **dict(swapping, flags=SWAP | ODD | INNER, noise=None, uniform=None))
        frozen = "flags: LSNF_HMC_SWAP excludes LSNF_HMC_ADAPT, LSNF_HMC_METRIC_FOLD, LSNF_HMC_METRIC_CLOSE and LSNF_HMC_ANNEAL"
        assert said(E, frozen, B=B, **dict(swapping, flags=SWAP | ADAPT, **adapting))
        assert said(E, frozen, B=B, **dict(swapping, flags=SWAP | ADAPT | LAST, **adapting))
        assert said(E, frozen, B=B, **dict(swapping, flags=SWAP | FOLD, **folding))
        assert said(E, frozen, B=B, **dict(swapping, flags=SWAP | FOLD | CLOSE, **folding))
        assert said(E, frozen, B=B, **dict(swapping, flags=SWAP | ODD | ANNEAL, **annealing))
        for bad in (0, 1, 3, 5, 6, 12, 32, -4):
            assert said(E, f"ladder must be 2, 4, 8 or 16 with LSNF_HMC_SWAP (got {bad})", B=B, **dict(swapping, ladder=bad))
        none = "swap_uniform, swap_out and log_swap_out must be NULL without LSNF_HMC_SWAP"
        for k in ("swap_uniform", "swap_out", "log_swap_out"):
            assert said(E, none, B=B, **{k: P[k]}) and said(E, none, B=B, flags=INIT, uniform=None, **{k: P[k]})
            assert said(E, none, B=B, ladder=4, **{k: P[k]})
        assert said(E, "swap_uniform goes with a noise tensor, not with an rng (the pair's uniform is drawn in-kernel)", B=B,
                    **dict(swapping, **philox))
        # the move's arrays alias nothing else the call touches
        assert said(E, "swap_out must not alias uniform", B=B, **dict(swapping, swap_out=P["uniform"]))
        assert said(E, "swap_out must not alias swap_uniform", B=B, **dict(swapping, swap_out=P["swap_uniform"]))
        assert said(E, "u_acc must not alias swap_uniform", B=B, **dict(swapping, swap_uniform=P["u_acc"]))
        assert said(E, "like_u_acc must not alias log_swap_out", B=B, **dict(swapping, log_swap_out=P["like_u"]))
        assert said(E, "swap_out must not alias log_swap_out", B=B, **dict(swapping, log_swap_out=P["swap_out"]))
        assert said(E, "accept_out must not alias swap_out", B=B, **dict(swapping, accept=P["swap_out"]))
        # the tempered call's rules, word for word (a sample: the whole table is tests/test_hmc_tempered_cpu.py's)
        assert said(E, "beta_next and log_w must be NULL without LSNF_HMC_ANNEAL", B=B, **dict(swapping, beta_next=P["beta_next"]))
        assert said(E, "flags: LSNF_HMC_INIT and LSNF_HMC_INNER exclude each other", B=B, flags=INIT | INNER, noise=None, uniform=None)
        assert said(E, f"like_grad_acc must not alias {point}", B=B, **dict(swapping, like_grad=P["point"]))
    for B, R in ((15, 2), (18, 4), (20, 8), (24, 16), (8, 16), (1, 2)):
        assert said(E, f"B={B} is not a multiple of ladder={R}", B=B, **dict(swapping, ladder=R))
    # an empty batch: nothing to launch, NULL pointers allowed, swapping or not
    nulls = {k: None for k in P}
    assert call(B=0, **nulls) == LSNF_OK and call(B=0, **dict(nulls, flags=SWAP, ladder=8)) == LSNF_OK
    assert call(B=0, **dict(nulls, flags=SWAP | ODD, ladder=16)) == LSNF_OK and call(B=0, **swapping) == LSNF_OK
    # the pointers of a non-empty call
    assert said(E, "swap_uniform is required with LSNF_HMC_SWAP when no rng is given", **dict(swapping, swap_uniform=None))
    assert said(E, "swap_uniform is required with LSNF_HMC_SWAP when no rng is given", **dict(swapping, flags=SWAP | ODD, swap_uniform=None))
    odd = ctypes.c_void_p(0xF00002)
    for k, said_name in (("swap_uniform", "swap_uniform"), ("swap_out", "swap_out"), ("log_swap_out", "log_swap_out")):
        assert said(E, f"{said_name} must be 4-byte aligned", **dict(swapping, **{k: odd}))
    assert said(E, "beta_rows is required (NULL)", **dict(swapping, beta=None))
    assert said(E, "uniform is required without an rng (unless LSNF_HMC_INIT or LSNF_HMC_INNER)", **dict(swapping, uniform=None))
    # (the next rule -- a misaligned act_saved -- is what refuses a call that passed all others: swap_out and log_swap_out are optional,
    # the uniforms come from a tensor or from the rng, every ladder and both parities pass, a call without SWAP ignores ladder)
    bad_act = ctypes.c_void_p(0x50008)
    off4 = lambda k: ctypes.c_void_p(P[k].value + 4)
    for ok in (dict(), dict(ladder=3), swapping, dict(swapping, flags=SWAP | ODD), dict(swapping, swap_out=None), dict(swapping, log_swap_out=None),
               dict(swapping, swap_out=None, log_swap_out=None), dict(swapping, swap_uniform=None, **philox),
               dict(swapping, noise=None, **{"next": None}),
               dict(swapping, swap_uniform=off4("swap_uniform"), swap_out=off4("swap_out"), log_swap_out=off4("log_swap_out")),
               dict(flags=ANNEAL, **annealing), dict(flags=INNER, noise=None, uniform=None)) + \
            tuple(dict(swapping, ladder=R) for R in (2, 4, 8, 16)):
        assert said(E, "act_saved must be 16-byte aligned", **dict(ok, act=bad_act))


def test_the_tempered_entry_points_still_refuse_the_new_bits():
    """Nothing about lsnf_hmc_step_tempered / lsnf_reverse_hmc_step_tempered changed: bits 0x80 and 0x100 are unknown there."""
    import test_hmc_tempered_cpu as T
    lib = lsnf_amd.load_library()
    for name in T.NAMES:
        _, said, _, _, _, _ = T._caller(lib, name)
        assert said(LSNF_E_ARG, "unknown flag bits 0x80", flags=SWAP) and said(LSNF_E_ARG, "unknown flag bits 0x180", flags=SWAP | ODD)


# ---- the Python wrappers and the samplers on CPU tensors ----------------------------------------------------------------------------
def _plan():
    F, lib = lsnf_amd.flow, lsnf_amd.load_library()
    return F.FlowPlan(8, 4, 2, 1, torch.zeros(lib.lsnf_plan_floats(8, 4, 2, 1)), torch.zeros(lib.lsnf_prepare_scratch_bytes(8, 4, 2) // 8, dtype=torch.float64))


def test_python_wrappers_speak_on_cpu_tensors(monkeypatch):
    from counting_lib import install
    F, L, M = lsnf_amd.flow, lsnf_amd.langevin, lsnf_amd.mcmc
    lib = lsnf_amd.load_library()
    plan = _plan()
    stand = install(monkeypatch, lsnf_amd)
    seen = []
    real = M._check_chain

    def spy(*a, **k):
        seen.append(k.get("stash"))
        return real(*a, **k)
    monkeypatch.setattr(M, "_check_chain", spy)
    B = 8
    z, saved = torch.zeros(B, 8), torch.zeros(1, B, 8)
    act = torch.zeros(lib.lsnf_act_saved_floats(8, 4, 2, B))
    steps, state, metric = F.new_hmc_row_steps(B, "cpu", 0.5), F.new_hmc_state(plan, B, "cpu"), F.new_hmc_row_metric(plan, B, "cpu")
    temper, nxt = F.new_hmc_row_temper(plan, B, "cpu"), torch.full((B,), 0.25)
    zcall = lambda **kw: F.hmc_step_exchange(plan, z, None, None, state, F.PhiloxNoise(3), steps, metric, temper, **kw)
    ecall = lambda **kw: F.reverse_hmc_step_exchange(plan, z, saved, act, None, None, state, F.PhiloxNoise(3), steps, metric, temper, **kw)
    for call in (zcall, ecall):
        n = len(seen)
        with pytest.raises(lsnf_amd.LsnfError, match="swap must be None, 'even' or 'odd'"):
            call(swap="both", ladder=4)
        for kw in (dict(phase="init"), dict(phase="inner"), dict(adapt="update"), dict(window="fold"), dict(anneal=nxt)):
            with pytest.raises(lsnf_amd.LsnfError, match="swap goes with phase='end', without adapt, window and anneal"):
                call(swap="even", ladder=4, **kw)
        for bad in (0, 3, 32, None):
            with pytest.raises(lsnf_amd.LsnfError, match="ladder must be 2, 4, 8 or 16"):
                call(swap="odd", ladder=bad)
        assert len(seen) == n                                # (refused before the tensors are looked at)
        for kw in (dict(), dict(swap="even", ladder=4), dict(swap="odd", ladder=8, propose=False), dict(phase="init"), dict(anneal=nxt)):
            with pytest.raises(lsnf_amd.LsnfError, match="no CPU path"):
                call(**kw)
        assert len(seen) == n + 5                            # every such call went through _check_chain
    assert all(st is None for st in seen[:5]) and all(st is not None and st[0] is saved and st[1] is act for st in seen[5:])
    # the swap's uniforms go through the one checking path; its own rules come after it
    cpu, su, rng = torch.device("cpu"), torch.zeros(B), object()
    with pytest.raises(lsnf_amd.LsnfError, match="swap_uniform must live on"):
        M._row_exchange_args(plan, "even", 4, su, None, B, torch.device("cuda:0"), False)
    names = []
    with monkeypatch.context() as m:
        m.setattr(M, "_check_in", lambda t, name, need, dev, *a, **k: names.append((name, need)))
        assert M._row_exchange_args(plan, None, 0, None, rng, B, cpu, False) == ((0, None, None, None), None, None)
        with pytest.raises(lsnf_amd.LsnfError, match="swap_uniform goes with swap="):
            M._row_exchange_args(plan, None, 0, su, None, B, cpu, False)
        with pytest.raises(lsnf_amd.LsnfError, match="are not a multiple of ladder=16"):
            M._row_exchange_args(plan, "even", 16, None, rng, B, cpu, False)
        for bad in ((su, rng), (None, None)):
            with pytest.raises(lsnf_amd.LsnfError, match="the swap draws as the trajectory does"):
                M._row_exchange_args(plan, "odd", 4, bad[0], bad[1], B, cpu, False)
        args, swapped, log_swap = M._row_exchange_args(plan, "odd", 4, su, None, B, cpu, False)
        assert args == (4, su.data_ptr(), swapped.data_ptr(), log_swap.data_ptr()) and swapped.shape == log_swap.shape == (B,)
        args, swapped, log_swap = M._row_exchange_args(plan, "even", 8, None, rng, B, cpu, False)
        assert args == (8, None, swapped.data_ptr(), log_swap.data_ptr()) and swapped.dtype == log_swap.dtype == torch.float32
    assert names == [("swap_uniform", B)] * 7
    flags = lambda swap: M._row_exchange_mode(swap, 4, "end", None, None, None)
    assert (flags(None), flags("even"), flags("odd")) == (0, SWAP, SWAP | ODD)
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    with pytest.raises(lsnf_amd.LsnfError):
        net.hmc_step_exchange(z, None, None, state, F.PhiloxNoise(1), steps, metric, temper, swap="even", ladder=4)
    with pytest.raises(lsnf_amd.LsnfError):
        net.reverse_hmc_step_exchange(z, saved, act, None, None, state, F.PhiloxNoise(1), steps, metric, temper, swap="even", ladder=4)
    # the samplers: their own rules, then the wrappers'; nothing to do returns without a launch
    x, G = torch.zeros(2, 8), torch.nn.Flatten()
    kw = dict(g_l_step_size=0.5, g_llhd_sigma=0.3, leapfrog_steps=2)
    for fn in (L.sample_hmc_pt_post_z_with_flow, L.sample_hmc_pt_post_eps_with_flow):
        start = torch.zeros(2, 8)
        with pytest.raises(ValueError, match="betas must hold 2, 4, 8 or 16 temperatures"):
            fn(start, x, G, net, betas=[0.1, 0.5, 1.0], g_l_steps=2, philox=F.PhiloxNoise(1), **kw)
        with pytest.raises(ValueError, match="leapfrog_steps"):
            fn(start, x, G, net, betas=L.pt_ladder(4, 0.1), g_l_steps=2, philox=F.PhiloxNoise(1), **dict(kw, leapfrog_steps=0))
        with pytest.raises(ValueError, match="swap_every"):
            fn(start, x, G, net, betas=L.pt_ladder(4, 0.1), g_l_steps=2, philox=F.PhiloxNoise(1), swap_every=0, **kw)
        with pytest.raises(lsnf_amd.LsnfError, match="metric must be a flow.HmcRowMetric"):
            fn(start, x, G, net, betas=L.pt_ladder(4, 0.1), g_l_steps=2, philox=F.PhiloxNoise(1), metric=1.0, **kw)
        with pytest.raises(lsnf_amd.LsnfError, match="steps must be a flow.HmcRowSteps"):
            fn(start, x, G, net, betas=L.pt_ladder(4, 0.1), g_l_steps=2, philox=F.PhiloxNoise(1), steps=0.5, **kw)
        with pytest.raises(lsnf_amd.LsnfError):              # (the first launch is refused: the tensors live on the CPU)
            fn(start, x, G, net, betas=L.pt_ladder(4, 0.1), g_l_steps=2, philox=F.PhiloxNoise(1), **kw)
        ph = F.PhiloxNoise(5, 100)
        out = fn(start, x, G, net, betas=L.pt_ladder(4, 0.1), g_l_steps=0, philox=ph, **kw)
        assert out[0].shape == (2, 8, 1, 1) and out[1:] == (None,) * 5
        out = fn(start[:0], x[:0], G, net, betas=L.pt_ladder(4, 0.1), g_l_steps=3, philox=ph, **kw)
        assert out[0].shape == (0, 8, 1, 1) and out[1:] == (None,) * 5 and ph.offset == 100
    assert stand.launching() == [], dict(stand.entered)
    # the swap schedule and the rate's bookkeeping
    _, R, K, Ls, swap = L._pt_plan(F, L.pt_ladder(4, 0.1), 7, 2, 2, None, None)
    assert (R, K, Ls) == (4, 7, 2) and [swap(t) for t in range(1, 8)] == [None, "even", None, "odd", None, "even", None]
    swap = L._pt_plan(F, L.pt_ladder(2, 0.1), 4, 1, 1, None, None)[4]
    assert [swap(t) for t in range(1, 5)] == ["even", "odd", "even", "odd"]
    sums = {"even": torch.arange(8.0), "odd": 10.0 * torch.arange(8.0)}
    rate = L._pt_swap_rate(sums, {"even": 2, "odd": 5}, 2, 4)
    assert rate.tolist() == [[0.0, 2.0, 1.0], [2.0, 10.0, 3.0]]
    assert L._pt_swap_rate(sums, {"even": 2, "odd": 0}, 2, 4).tolist() == [[0.0, 0.0, 1.0], [2.0, 0.0, 3.0]]


# ---- the float64 restatement: swaps make the beta = 1 rung visit both wells in their closed-form proportion ----------------------
EXP_GAP, EXP_R, EXP_BETA_MIN, EXP_N, EXP_K, EXP_L, EXP_STEP, EXP_SEED, FACTOR = 3.0, 4, 0.02, 32, 150, 3, 0.28, 1, 5.0


def _occupancy(swap):
    f64 = torch.float64
    p, nz = A.affine_flow(), A.GEO[0]
    target = X.TwoMode(nz, EXP_GAP)
    logz = torch.tensor([A.closed_form(p, q) for q in target.quads], dtype=f64)
    W1 = torch.softmax(logz, 0)[0].item()
    R, N, K = EXP_R, EXP_N, EXP_K
    B = N * R
    g = torch.Generator().manual_seed(EXP_SEED)
    beta = lsnf_amd.langevin.pt_ladder(R, EXP_BETA_MIN).repeat(N)
    x0 = target.quads[0].t.clone()[None, :].repeat(B, 1)     # every replica starts at the centre of well 1
    noises = [torch.randn(B, nz, generator=g, dtype=f64) for _ in range(K)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g, dtype=f64).clamp_min(2.0 ** -25) for _ in range(K)]
    swap_uniforms = [torch.rand(B, generator=g, dtype=f64).clamp_min(2.0 ** -25) for _ in range(K)]
    swaps = [("even", "odd")[k % 2] if swap else None for k in range(K)]
    step = torch.full((B,), EXP_STEP, dtype=f64) / torch.sqrt(beta).clamp_min(0.3)      # a hot rung's wells are wider
    tr = X.chain(TR.flow_parts("z", p, target), x0, step, torch.ones(B, nz, dtype=f64), EXP_L, noises, uniforms, beta, R, swaps, swap_uniforms)
    burn = K // 5
    top = tr.states.view(K, N, R, nz)[burn:, :, R - 1]
    n = (K - burn) * N
    return W1, target.in_mode_1(top).double().mean().item(), FACTOR * math.sqrt(W1 * (1.0 - W1) / n), tr


def test_swaps_bring_the_cold_rung_to_the_closed_form_mode_weights():
    W1, occ, margin, tr = _occupancy(True)
    W1b, stuck, _, plain = _occupancy(False)
    rate = tr.swapped.double().mean().item()
    print(f"two wells, closed-form weight of well 1 {W1:.4f}; beta = 1 rung's occupancy with swaps {occ:.4f}, without {stuck:.4f}; margin "
          f"{FACTOR:g} x binomial SE = {margin:.4f}; rows swapped per call {rate:.3f}, acceptance {tr.acc.double().mean().item():.3f}")
    assert W1 == W1b and 0.05 < W1 < 0.95
    assert abs(occ - W1) <= margin, "with swaps the cold rung's occupancy is not the closed-form weight"
    assert abs(stuck - W1) > margin, "without swaps the cold rung was expected to stay in the well it started in"
    assert not plain.swapped.any() and 0.1 < rate < 0.9
    # both rows of a pair report the same decision and ratio; idle rungs report nothing
    for k in (0, 1):
        prt = X.partner(EXP_N * EXP_R, EXP_R, ("even", "odd")[k])
        assert torch.equal(tr.swapped[k], tr.swapped[k][prt]) and torch.equal(tr.log_swap[k], tr.log_swap[k][prt])
        idle = prt == torch.arange(EXP_N * EXP_R)
        assert not tr.swapped[k][idle].any() and not tr.log_swap[k][idle].any()


def test_cost_tool_is_a_driver_on_the_ab_harness():
    """tools/hmc_exchange_vs_hmc_tempered.py: its child's source is valid and importing the driver does not import torch."""
    import subprocess
    import sys
    tools = os.path.join(ROOT, "tools")
    code = ("import sys; sys.path.insert(0, %r)\nimport ab_harness, hmc_exchange_vs_hmc_tempered as t\n"
            "compile(ab_harness.PRELUDE + t.CHILD, 'child', 'exec')\nassert 'torch' not in sys.modules\n"
            "assert t.SIZES == (100, 16384) and t.LADDER == 4 and all(B %% t.LADDER == 0 for B in t.SIZES)" % tools)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=60)

"""GPU: Hamiltonian Monte Carlo in the flow's base space (lsnf_reverse_hmc_step, lsnf_small3_rhmc_kernel: the latency bf16x3
reverse-backward with the leapfrog tail as its output section), `flow.reverse_hmc_step`, `_netF.reverse_hmc_step` and
`langevin.sample_hmc_post_eps_with_flow`.

Against float64 every call is TEACHER-FORCED: the device is given the fp32 casts of the float64 restatement's inputs of that call
(tests/rhmc_restated.py: state, momentum, kin0, the point eps_prop, grad_g / energy_g of the closed-form quadratic at the float64
x = f^-1(eps_prop), noise, uniform), so a decision that differs on one row cannot move a later call's inputs; the device runs its
own reverse at the point for the stash.  Momentum draws of which any point of the trajectory would put x within 2e-5 of a ReLU kink
are redrawn on the CPU.  L = 3; two trajectories (7 calls) for B <= 100, above that one init, one inner and one end call (the CPU
computes the whole trajectory; the device is not given its second inner call).  Per row of an end call
    gate = max(1e-5 * (|u_acc| + |U_prop| + kin0 + kinL), 3 * |fp32 restatement - fp64 restatement|);
rows whose float64 log_alpha is within the gate of ln u, and rows with oracle.relu_margin <= 2e-5 at x, are set aside (at most 10 %
of a case, 2 rows for B <= 33: asserted on the CPU, and again for the set formed from the device's own log_alpha and the kink rows).  u_acc: tests/test_gpu_rmala.py's bound
1e-5 (|e| + |eps|^2 / 2) (Case asserts that the fp32 restatement meets a third of it on accepted rows); grad_acc and eps_next rel-L2
<= 1e-5 per row, |mom - fp64| <= 1e-5 (|mom_in or xi| + s |t|), kin0 relative <= 1e-5 per row, each widened to 3 x the fp32
restatement's own error where that exceeds a third of it (the number of rows widened is printed).  Everything else is bit identity
between call forms, or the device against itself.

Step sizes are chosen on the CPU from the float64 restatement alone -- Case.rate of the two-trajectory case of 33 rows (L = 3,
quadratic scale 0.1, the kink redraw on), scanned in steps of 0.01 -- so that the two-trajectory cases accept between 15 % and 85 %
of their decisions (asserted).  The window is narrow at large nz: at C3 the rate falls from 0.79 to 0.20 between s = 0.45 and 0.48.  The
scan and the rates found are in profiles/rhmc.txt; the rate at the step chosen is beside each entry below."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import flow_oracle as O
import chain_geometries as G
import rhmc_restated as RH
import rmala_restated as RM
import trained_weights as T
import test_gpu_reverse_keep as K
from test_gpu_langevin import ToyG

pytestmark = pytest.mark.gpu

C3, C5, TINY = K.C3, K.C5, K.TINY
CASES = [C3 + (B,) for B in (1, 17, 33, 100, 4100, 8200, 16400)] + \
        [TINY + (33,), C5 + (33,), (126, 127, 2, 1, 33), (2, 1, 3, 1, 33), (64, 32, 1, 1, 33), (20, 12, 16, 1, 33), (20, 12, 5, 0, 33)]
CASES += G.CASES + G.LARGE                                   # the geometry classes of tests/chain_geometries.py
RUNS = [c + ("default",) for c in CASES] + [C3 + (100, "fp32")]
L_STEPS = 3
# Step size per geometry, keyed whole (nz 20, 66 and 128 occur with two flows): `Case(*geo, 33, s=s, light=True).rate` scanned in steps of
# 0.05 from 0.5 to 1.6 times the geometry's base-space MALA step (tests/test_gpu_rmala.py), then in steps of 0.01 across +-0.05 of the
# coarse step nearest one half; the step whose rate is nearest one half (the smaller of two).  Beside each entry: the rate found.  The
# whole scan: profiles/rhmc.txt.
STEP_GEO = {
    (128, 64, 5, 1): 0.47,       # 0.47
    (8, 4, 5, 1): 1.13,          # 0.50
    (100, 128, 5, 1): 0.51,      # 0.48
    (126, 127, 2, 1): 0.65,      # 0.44
    (2, 1, 3, 1): 1.81,          # 0.45
    (64, 32, 1, 1): 0.95,        # 0.50
    (20, 12, 16, 1): 0.43,       # 0.58
    (20, 12, 5, 0): 1.17,        # 0.50
    (62, 31, 2, 1): 0.84,        # 0.52
    (66, 33, 2, 1): 0.80,        # 0.47
    (124, 63, 3, 1): 0.58,       # 0.39
    (66, 33, 3, 0): 0.85,        # 0.45
    (10, 40, 2, 1): 1.24,        # 0.50
    (70, 8, 2, 1): 0.84,         # 0.48
    (12, 100, 2, 1): 1.20,       # 0.50
    (66, 65, 2, 1): 0.81,        # 0.55
    (128, 128, 2, 1): 0.63,      # 0.56
}
# seed offset of a case's generator, chosen on the CPU (the float64 restatement alone) where the default draws leave a two-trajectory
# case outside 15 % .. 85 % (B = 1 has two decisions: exactly one must accept) or set aside more rows than allowed
SEED = {C3 + (1,): 1}                                        # (offsets 1, 3, 5 accept one of the two; 2, 4 both; 0 none)
STEP_L1 = {128: 0.5, 8: 1.0}                                 # L = 1 against reverse_mala_step: tests/test_gpu_rmala.py's steps


def step_of(geo, weights=T.INIT):
    return float(np.float32(STEP_GEO[geo] if weights == T.INIT else T.step_of("hmc eps", geo)))     # the fp32 step the kernel sees


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


def rel_rows(got, ref):
    return (got.double() - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)


def widened(bound, own):
    """The bound per row, widened to 3 x the fp32 restatement's own error where that exceeds a third of it; how many rows were."""
    wide = own > bound / 3.0
    return torch.where(wide, 3.0 * own, bound), int(wide.sum())


class Case:
    """One geometry and batch on the CPU: the float64 chain's call records, each with its fp32 restatement, gates and row sets.
    s / seed: the overrides of the step-size scan; light: the chain and its rate alone."""

    def __init__(self, nz, w, depth, coupling, B, s=None, seed=None, light=False, weights=T.INIT):
        self.geo, self.B, self.nz, self.depth, self.weights = (nz, w, depth, coupling), B, nz, depth, weights
        p = T.params_for(O, self.geo, weights)
        self.p = K.additive(p) if coupling == 0 else p
        self.s, self.L = step_of(self.geo, weights) if s is None else float(np.float32(s)), L_STEPS
        self.n_traj = 2 if B <= 100 else 1
        self.quad = RH.Quadratic(nz, 0.1, seed=7 + nz)        # (U >= |eps|^2 / 2 is of order nz / 2: no row's bound falls below fp32)
        g = torch.Generator().manual_seed(7 + B + (SEED.get(self.geo + (B,), 0) if seed is None else seed))
        x0, _ = O.smooth_batch(self.p, B, nz, seed=1007 + B)  # (the chain's start is clear of a ReLU kink too)
        self.eps0 = K.R.forward64(self.p, x0)[0].float()
        noises = [torch.randn(B, nz, generator=g) for _ in range(self.n_traj)] + [None]
        uniforms = [None] + [torch.rand(B, generator=g).clamp_min(2.0 ** -25) for _ in range(self.n_traj)]
        self.calls, _ = RH.chain(self.p, self.eps0, self.quad, self.s, self.L, noises, uniforms, redraw=g)
        ends = [c for c in self.calls if c.phase == "end"]
        self.rate = torch.stack([c.acc for c in ends]).double().mean().item()
        self.allowed = 2 if B <= 33 else B // 10
        if light:
            return
        s = self.s
        for c in self.calls:
            c.o32 = o = RH.call32(self.p, c, s)
            c.margin = O.relu_margin(self.p, c.x.float())
            c.smooth = c.margin > 2e-5
            c.decided = c.smooth
            if c.phase != "inner":                           # the u_acc bound can be met in fp32 on these inputs (tests/test_gpu_rmala.py)
                c.u_scale = c.e.abs() + 0.5 * (c.e_prop ** 2).sum(1)
                c.u_own = (o.U_prop.double() - c.U_prop).abs()
                assert bool((c.u_own <= 1e-5 * c.u_scale / 3.0)[c.acc].all()), "the u_acc bound is below fp32 on these inputs"
                c.g_bound, c.g_wide = widened(torch.full((B,), 1e-5, dtype=torch.float64), rel_rows(o.g, c.g))
            if c.phase == "end":
                c.scale = c.u_acc.abs() + c.U_prop.abs() + c.kin_in + c.kinL
                c.gate = torch.maximum(1e-5 * c.scale, 3.0 * (o.la.double() - c.la).abs())
                c.decided = c.smooth & ((c.la - torch.log(c.u.double())).abs() > c.gate)
                assert int((~c.decided).sum()) <= self.allowed, "too many rows set aside: choose another seed"
            # the bounds of a call that proposes / leaves a momentum, from float64 and the fp32 restatement alone
            if c.mom_out is not None and c.phase != "init" or c.e_next is not None:
                src = c.noise.double() if c.noise is not None else c.mom_in
                gg = c.g_after if c.noise is not None else c.g
                c.mom_bound, c.mom_wide = widened(1e-5 * (src.norm(dim=1) + s * gg.norm(dim=1)), (o.mom_out.double() - c.mom_out).norm(dim=1))
            if c.e_next is not None:
                c.e_bound, c.e_wide = widened(torch.full((B,), 1e-5, dtype=torch.float64), rel_rows(o.e_next, c.e_next))
            if c.noise is not None:
                c.kin_bound, c.kin_wide = widened(1e-5 * c.kin_out, (o.kin_out.double() - c.kin_out).abs())
        # what the device is given: every call for B <= 100, else init, the first inner call and the end call
        self.device_calls = self.calls if B <= 100 else [self.calls[0], self.calls[1], self.calls[self.L]]


@functools.lru_cache(maxsize=None)
def case(nz, w, depth, coupling, B, weights=T.INIT):
    return Case(nz, w, depth, coupling, B, weights=weights)


class Setup:
    """A case's plan on the device (made under the run's math mode, as its stash will be)."""

    def __init__(self, lsnf, dev, nz, w, depth, coupling, B, mode, weights=T.INIT):
        self.c, self.dev, self.mode = case(nz, w, depth, coupling, B, weights), dev, mode
        self.plan = K.make_plan(lsnf, self.c, dev)


@functools.lru_cache(maxsize=None)
def setup_of(lsnf, dev, nz, w, depth, coupling, B, mode="default", weights=T.INIT):
    return Setup(lsnf, dev, nz, w, depth, coupling, B, mode, weights)


@pytest.fixture
def math(request, lsnf):
    def enter(mode):
        if mode == "fp32":
            F = lsnf.flow
            prev = F.set_math_mode(F.MATH_FP32)
            request.addfinalizer(lambda: F.set_math_mode(prev))
    return enter


def bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


FIELDS = ("z", "grad", "energy", "mom", "kin")


def clone_state(lsnf, st):
    return lsnf.flow.HmcState(*(getattr(st, f).clone() for f in FIELDS))


def stash_at(lsnf, plan, eps, how="auto"):
    """(saved, act) of the forward at x = reverse(eps): kept by the reverse launch itself ("reverse"; "auto": where supported), or by
    a forward at the reverse's x ("forward").  The stash is NaN-filled first: every word read of a live row must have been written."""
    F, B, dev = lsnf.flow, eps.shape[0], eps.device
    act = F.new_act_saved(plan, B, dev)
    act.fill_(float("nan"))
    if how == "reverse" or (how == "auto" and F.reverse_keep_supported(plan, B)):
        return F.reverse(plan, eps, None, save_for_backward=True, act_saved=act)[2], act
    x = F.reverse(plan, eps, None)[0]
    return F.forward(plan, x, None, want_ll=False, save_for_backward=True, act_saved=act)[3], act


def state_for(lsnf, s, c, rows=slice(None)):
    """The HmcState a recorded call is given: the fp32 casts of the float64 state, momentum and kin0 before it.  What the call must
    not read is NaN: the whole state for init, z / grad / energy / kin for an inner call."""
    B, nz, dev = c.e_prop[rows].shape[0], s.c.nz, s.dev
    nan_rows, nan_one = (lambda: torch.full((B, nz), float("nan"), device=dev)), (lambda: torch.full((B,), float("nan"), device=dev))
    cut = lambda t: t[rows].float().to(dev).contiguous()
    if c.phase == "init":
        return lsnf.flow.HmcState(nan_rows(), nan_rows(), nan_one(), nan_rows(), nan_one())
    if c.phase == "inner":
        return lsnf.flow.HmcState(nan_rows(), nan_rows(), nan_one(), cut(c.mom_in), nan_one())
    return lsnf.flow.HmcState(cut(c.e_acc), cut(c.g_acc), cut(c.u_acc), cut(c.mom_in), cut(c.kin_in))


def run(lsnf, s, c, noise="record", uniform="record", rows=slice(None), state=None, grad_g="record", **kw):
    """The recorded call c on its rows `rows` from its inputs' casts: (state after, outputs).  noise / uniform / grad_g "record": the
    record's."""
    cut = lambda t: None if t is None else t[rows].float().to(s.dev).contiguous()
    state = state_for(lsnf, s, c, rows) if state is None else state
    noise = cut(c.noise) if isinstance(noise, str) else noise
    uniform = cut(c.u) if isinstance(uniform, str) else uniform
    grad_g = cut(c.ge) if isinstance(grad_g, str) else grad_g
    kw.setdefault("propose", c.e_next is not None)
    eps = cut(c.e_prop)
    saved, act = stash_at(lsnf, s.plan, eps)
    out = lsnf.flow.reverse_hmc_step(s.plan, eps, saved, act, grad_g, cut(c.e), state, noise, s.c.s, phase=c.phase, uniform=uniform, **kw)
    return state, out


def same(a, b):
    """Two (state, outputs) results hold the same bits."""
    (sa, oa), (sb, ob) = a, b
    xs = [getattr(sa, f) for f in FIELDS] + list(oa)
    ys = [getattr(sb, f) for f in FIELDS] + list(ob)
    return all((x is None and y is None) or (x is not None and y is not None and bits(x, y)) for x, y in zip(xs, ys))


fig = lambda t: t.max().item() if t.numel() else 0.0


# ---------------------------------------------------------------------------------------------
# 1. against float64, teacher-forced
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B,mode", RUNS)
def test_every_call_follows_float64(lsnf, gpu_device, math, nz, w, depth, coupling, B, mode, weights=T.INIT):
    math(mode)
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, mode, weights)
    c = s.c
    tag = f"[rhmc] {mode} {c.geo} B{B}" + ("" if weights == T.INIT else f" {weights}")
    print(f"{tag} s={c.s:.3f} L={c.L}: float64 accepts {100 * c.rate:.0f} % of {c.n_traj} x {B} decisions")
    if c.n_traj > 1:
        assert 0.15 <= c.rate <= 0.85
    for j, r in enumerate(c.device_calls):
        state = state_for(lsnf, s, r)
        before = clone_state(lsnf, state)
        state, (e_next, acc, la) = run(lsnf, s, r, state=state)
        torch.cuda.synchronize()
        ea, ga, ua, mom, kin = (getattr(state, f).cpu() for f in FIELDS)
        name = f"{tag} call {j} {r.phase}"
        if r.phase == "inner":
            assert acc is None and la is None
            for f in ("z", "grad", "energy", "kin"):
                assert bits(getattr(state, f), getattr(before, f))            # neither read nor written: the NaN sentinels are there
        else:
            d, a64 = r.decided, r.acc
            acc_c = acc.cpu()
            assert bool(((acc_c == 1.0) | (acc_c == 0.0)).all())
            if r.phase == "init":
                assert bool((acc_c == 1.0).all()) and bits(la, torch.zeros_like(la))
            else:
                aside = int((~d).sum())
                err = (la.cpu().double() - r.la).abs()
                # At trained weights a few rows of the larger batches leave the window in which the float64 trajectory is stable
                # (C3 in eps at s = 0.025: 1 row of 100, 11 of 4100, 15 of 8200): the float64 record or its fp32 restatement is not
                # finite there, so neither is the gate.  Such a row is among those set aside (it counts against the cap), no bound
                # can be held on it, and where float64 itself has no finite log_alpha the device must reject it.  A row whose
                # float64 log_alpha is finite while its fp32 restatement is not (x = f^-1(eps) overflows in fp32 alone: 3 of the 11
                # at 4100 rows) is held to NOTHING but that count: plain fp32 arithmetic has no finite answer on those inputs, so
                # none is asked of an fp32 kernel; the device's figure against the unwidened 1e-5 x scale is printed.  At the init
                # weights there is no such row of either kind.
                held = torch.isfinite(r.gate)
                fp32_only = ~held & torch.isfinite(r.la) & torch.isfinite(r.scale)
                if bool(fp32_only.any()):
                    print(f"{name}: {int(fp32_only.sum())} rows finite in float64 alone (held to nothing): device |log_alpha - fp64| / (1e-5 scale) = "
                          f"{(err / (1e-5 * r.scale))[fp32_only].tolist()}")
                assert weights != T.INIT or bool(held.all())
                assert not bool((~held & d).any()) and bool((acc_c[~torch.isfinite(r.la)] == 0.0).all())
                worst = fig((err / r.gate)[r.smooth & held])
                # the same share from the device's figures: its own log_alpha within the gate of ln u, together with the kink rows
                aside_dev = int((~r.smooth | ((la.cpu().double() - torch.log(r.u.double())).abs() <= r.gate)).sum())
                print(f"{name}: accepted {int(a64.sum())}/{B}, set aside {aside} (allowed {c.allowed}; {int((~r.smooth).sum())} near a kink; "
                      f"{aside_dev} by the device's log_alpha), "
                      f"worst |log_alpha - fp64| / gate = {worst:.3f}, fp32 restatement worst "
                      f"{fig(((r.o32.la.double() - r.la).abs() / r.gate)[held]):.3f}, {int((~held).sum())} rows without a finite gate")
                assert aside <= c.allowed and aside_dev <= c.allowed
                assert bool((err <= r.gate)[r.smooth & held].all())
                assert torch.equal(acc_c[d] == 1.0, a64[d])
            yes, no = d & a64, d & ~a64
            ub = torch.maximum(1e-5 * r.u_scale, 3.0 * r.u_own)
            g_err = rel_rows(ga, r.g)
            print(f"{name}: worst u_acc error / bound = {fig(((ua.double() - r.U_prop).abs() / ub)[yes]):.3f}, "
                  f"worst grad_acc rel-L2 / bound = {fig((g_err / r.g_bound)[yes]):.3f} ({r.g_wide} rows widened by the fp32 restatement)")
            assert bits(ea[yes], r.e_prop.float()[yes])
            assert bool(((ua.double() - r.U_prop).abs() <= ub)[yes].all())
            assert bool((g_err <= r.g_bound)[yes].all())
            if r.phase == "end":
                bz, bg, bu = before.z.cpu(), before.grad.cpu(), before.energy.cpu()
                assert bits(ea[no], bz[no]) and bits(ga[no], bg[no]) and bits(ua[no], bu[no])
        d = r.decided
        if hasattr(r, "mom_bound"):
            e = (mom.double() - r.mom_out).norm(dim=1)
            print(f"{name}: worst |mom - fp64| / bound = {fig((e / r.mom_bound)[d]):.3f} ({r.mom_wide} rows widened by the fp32 restatement)")
            assert bool((e <= r.mom_bound)[d].all())
        if r.e_next is not None:
            e = rel_rows(e_next.cpu(), r.e_next)
            print(f"{name}: worst eps_next rel-L2 / bound = {fig((e / r.e_bound)[d]):.3f} ({r.e_wide} rows widened)")
            assert bool((e <= r.e_bound)[d].all())
        else:
            assert e_next is None
        if r.noise is not None:
            e = (kin.double() - r.kin_out).abs()
            print(f"{name}: worst kin0 error / bound = {fig(e / r.kin_bound):.3f} ({r.kin_wide} rows widened)")
            assert bool((e <= r.kin_bound).all())
        elif r.phase != "init":
            assert bits(state.kin, before.kin)                                    # no trajectory begun: kin0 is left as it is


@pytest.mark.parametrize("nz,w,depth,coupling,B", T.CASES)
def test_every_call_follows_float64_at_trained_weights(lsnf, gpu_device, math, nz, w, depth, coupling, B):
    """The same calls, gates and caps on the golden trained weights (tests/trained_weights.py): a saturating sigmoid, |3 logs| up to 2,
    steps from the narrow window in which the float64 leapfrog is stable there."""
    test_every_call_follows_float64(lsnf, gpu_device, math, nz, w, depth, coupling, B, "default", weights=T.TRAINED)


SMALL = [C3 + (33,), C3 + (4100,), C3 + (8200,), TINY + (33,)]
FORMS = SMALL + G.FORMS                                      # the cases of the bit identities


def end_call(c):
    """The first end call of a case (B <= 100: it begins the next trajectory; above: it proposes nothing)."""
    return next(r for r in c.calls if r.phase == "end")


# ---------------------------------------------------------------------------------------------
# 2. bit identities on the device
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", FORMS)
def test_init_state_is_the_mala_init_state(lsnf, gpu_device, nz, w, depth, coupling, B):
    """(a) after an INIT call state.z / grad / energy are `reverse_mala_step(init=True)`'s on the same inputs, bit for bit, and
    state.grad is eps_prop + reverse_backward_z(...), one torch fp32 add; without a proposal the state alone is written."""
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c = lsnf.flow, gpu_device, s.c
    r = c.calls[0]
    cut = lambda t: t.float().to(dev).contiguous()
    eps, ge, e = cut(r.e_prop), cut(r.ge), cut(r.e)
    saved, act = stash_at(lsnf, s.plan, eps)
    g = F.reverse_backward_z(s.plan, eps, saved, act, ge, None)
    for xi in (cut(r.noise), F.PhiloxNoise(1234, 40, 3)):
        hs = state_for(lsnf, s, r)                                                # NaN: never read
        ms = F.MalaState(*(torch.full_like(t, float("nan")) for t in (eps, eps, e)))
        e_next, acc, la = F.reverse_hmc_step(s.plan, eps, saved, act, ge, e, hs, xi, c.s, phase="init")
        F.reverse_mala_step(s.plan, eps, saved, act, ge, e, ms, xi, c.s, init=True)
        assert bits(hs.z, ms.z) and bits(hs.grad, ms.grad) and bits(hs.energy, ms.energy)
        assert bits(hs.z, eps) and bits(hs.grad, eps + g)
        assert bool((acc == 1.0).all()) and bits(la, torch.zeros_like(la))
        # the first trajectory's begin, each op a launch of its own
        draw = xi if isinstance(xi, torch.Tensor) else F.sample(s.plan, B, xi, want_eps=True)[2]
        ph = draw - (0.5 * c.s) * hs.grad
        assert bits(hs.mom, ph) and bits(e_next, eps + c.s * ph)
    hs2 = F.new_hmc_state(s.plan, B, dev)
    hs2.mom.fill_(3.0); hs2.kin.fill_(4.0)
    none = F.reverse_hmc_step(s.plan, eps, saved, act, ge, e, hs2, F.PhiloxNoise(1234, 40, 3), c.s, phase="init", propose=False)
    assert none[0] is None and bits(hs2.z, hs.z) and bits(hs2.grad, hs.grad) and bits(hs2.energy, hs.energy)
    assert bool((hs2.mom == 3.0).all()) and bool((hs2.kin == 4.0).all())           # mom and kin0 are left as they are


@pytest.mark.parametrize("nz,w,depth,coupling,B", FORMS)
def test_inner_call_is_the_elementwise_recomputation(lsnf, gpu_device, nz, w, depth, coupling, B):
    """(b) mom and eps_next of an inner call against torch fp32 ops, each a launch of its own: t = eps + g, ph = mom - (s t),
    next = eps + (s ph); state.z / grad / energy / kin are untouched."""
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c = lsnf.flow, gpu_device, s.c
    r = c.calls[1]
    assert r.phase == "inner"
    cut = lambda t: t.float().to(dev).contiguous()
    eps, ge = cut(r.e_prop), cut(r.ge)
    saved, act = stash_at(lsnf, s.plan, eps)
    g = F.reverse_backward_z(s.plan, eps, saved, act, ge, None)
    state = state_for(lsnf, s, r)
    before = clone_state(lsnf, state)
    e_next, acc, la = F.reverse_hmc_step(s.plan, eps, saved, act, ge, None, state, None, c.s, phase="inner")
    t = eps + g
    st = t * c.s
    ph = before.mom - st
    sp = ph * c.s
    assert acc is None and la is None
    assert bits(state.mom, ph) and bits(e_next, eps + sp)
    for f in ("z", "grad", "energy", "kin"):
        assert bits(getattr(state, f), getattr(before, f))


@pytest.mark.parametrize("nz,w,depth,coupling,B", FORMS)
def test_philox_is_the_tensors_of_the_same_draws(lsnf, gpu_device, nz, w, depth, coupling, B):
    """(c) xi is `flow.sample(..., want_eps=True)`'s eps at the same generator, u rmala_restated.uniform_draws."""
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c = lsnf.flow, gpu_device, s.c
    for r in (c.calls[0], end_call(c)):
        for row0 in (0, 2 ** 32 - 5):
            rng = F.PhiloxNoise(1234, 40, row0)
            xi = F.sample(s.plan, B, rng, want_eps=True)[2]
            u = None if r.phase == "init" else torch.from_numpy(RH.uniform_draws(B, 1234, 40, row0)).to(dev)
            got, ref = run(lsnf, s, r, rng, None, propose=True), run(lsnf, s, r, xi, u, propose=True)
            # kin0 is 1/2 sum xi^2 over the nz real columns: the draw of a padding column (a half that is no multiple of 4) is not in it
            x64 = xi.cpu().double()
            kin64, kin32 = 0.5 * (x64 ** 2).sum(1), 0.5 * (xi.cpu() ** 2).sum(1)
            bound, _ = widened(1e-5 * kin64, (kin32.double() - kin64).abs())              # Case's kin_bound, at these draws
            kin_err = (got[0].kin.cpu().double() - kin64).abs()
            print(f"[rhmc] {c.geo} B{B} {r.phase} row0 {row0}: in-kernel draw, worst kin0 error / bound = {fig(kin_err / bound):.3f}")
            assert same(got, ref)
            assert xi.shape == (B, nz) and bool((kin_err <= bound).all())
            assert r.phase == "init" or 0 < int(got[1][1].sum()) < B or B < 8      # both outcomes occur
        assert rng.offset == 40                                             # the call does not advance the generator
        ctr = torch.full((1,), 3, dtype=torch.int64, device=dev)
        a = run(lsnf, s, r, F.PhiloxNoise(1234, 37, 0, offset_dev=ctr), None, propose=True)
        b = run(lsnf, s, r, F.PhiloxNoise(1234, 40, 0), None, propose=True)
        assert same(a, b) and not bits(a[1][0], run(lsnf, s, r, F.PhiloxNoise(1234, 37, 0), None, propose=True)[1][0])
    with pytest.raises(lsnf.LsnfError):
        run(lsnf, s, r, rng, u, propose=True)                               # a generator and a tensor exclude each other
    with pytest.raises(lsnf.LsnfError):
        run(lsnf, s, r, xi, None, propose=True)                             # tensors: the uniform is required
    with pytest.raises(lsnf.LsnfError):
        run(lsnf, s, c.calls[1], rng, None)                                 # an inner call takes no generator


# (64 rows per workgroup; the <1, 1> geometry at 32 and at 64 rows; f_width > 64 at 32 rows, its largest shape: with the cases above,
# every instantiation of lsnf_small3_rhmc_kernel that the default dispatch can reach)
@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (8200,), TINY + (4100,), TINY + (8200,), C5 + (4100,)] + G.LARGE)
def test_rows_do_not_depend_on_the_batch_or_the_sharding(lsnf, gpu_device, nz, w, depth, coupling, B):
    """(d) sub-batches against the full batch, in every phase."""
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, c = lsnf.flow, s.c
    flat = lambda r: [getattr(r[0], f) for f in FIELDS] + [t for t in r[1] if t is not None]
    for r in (c.calls[0], c.calls[1], end_call(c)):
        inner = r.phase == "inner"
        gen = lambda row0: None if inner else F.PhiloxNoise(99, 7, row0)
        kw = dict(propose=True)
        whole = run(lsnf, s, r, gen(0), None, **kw)
        part = run(lsnf, s, r, gen(0), None, rows=slice(0, 100), **kw)        # 16 rows per workgroup
        alone = run(lsnf, s, r, gen(57), None, rows=slice(57, 58), **kw)
        for a, b, x in zip(flat(whole), flat(part), flat(alone)):
            assert bits(a[:100], b) and bits(b[57:58], x)
        lo = run(lsnf, s, r, gen(0), None, rows=slice(0, 40), **kw)
        hi = run(lsnf, s, r, gen(40), None, rows=slice(40, 100), **kw)
        for a, x, y in zip(flat(part), flat(lo), flat(hi)):
            assert bits(a, torch.cat([x, y]))
        if not inner:
            wrong = run(lsnf, s, r, gen(0), None, rows=slice(40, 100), **kw)
            assert not bits(wrong[1][0], part[1][0][40:100])


@pytest.mark.parametrize("nz,w,depth,coupling,B", FORMS)
def test_in_place_and_four_bytes_off_a_16_byte_boundary(lsnf, gpu_device, nz, w, depth, coupling, B):
    """(e) eps_next over eps_prop, and every tensor 4 bytes off a 16-byte boundary, equal the plain call."""
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c = lsnf.flow, gpu_device, s.c

    def off4(t):
        if t is None:
            return None
        t = t.float().to(dev)
        b = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
        v = b[1: 1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    for r in (c.calls[0], c.calls[1], end_call(c)):
        inner = r.phase == "inner"
        noise = None if inner else (r.noise if r.noise is not None else c.calls[0].noise).to(dev)
        ref = run(lsnf, s, r, noise, "record", propose=True)
        u = None if r.u is None else r.u.to(dev)
        # in place: the next point over the point
        state, ep = state_for(lsnf, s, r), r.e_prop.float().to(dev)
        saved, act = stash_at(lsnf, s.plan, ep)
        ge, e = r.ge.float().to(dev), r.e.float().to(dev)
        out = F.reverse_hmc_step(s.plan, ep, saved, act, ge, e, state, noise, c.s, phase=r.phase, uniform=u, inplace=True)
        assert out[0].data_ptr() == ep.data_ptr() and same((state, out), ref)
        # the Philox form in place as well
        if not inner:
            rng = F.PhiloxNoise(5, 6, 7)
            ref2 = run(lsnf, s, r, rng, None, propose=True)
            state, ep = state_for(lsnf, s, r), r.e_prop.float().to(dev)
            out = F.reverse_hmc_step(s.plan, ep, saved, act, ge, e, state, rng, c.s, phase=r.phase, inplace=True)
            assert same((state, out), ref2)
        # every tensor 4 bytes off a 16-byte boundary
        st = state_for(lsnf, s, r)
        state = F.HmcState(*(off4(getattr(st, f)) for f in FIELDS))
        out = F.reverse_hmc_step(s.plan, off4(r.e_prop), off4(saved), act, off4(r.ge), off4(r.e), state, off4(noise), c.s, phase=r.phase,
                                 uniform=off4(u), inplace=True)
        assert same((state, out), ref)
    with pytest.raises(lsnf.LsnfError):                                 # no other output may be an input
        st = state_for(lsnf, s, r)
        ep = r.e_prop.float().to(dev)
        F.reverse_hmc_step(s.plan, ep, saved, act, ge, e, F.HmcState(ep, st.grad, st.energy, st.mom, st.kin), noise, c.s, uniform=u)


@pytest.mark.parametrize("nz,w,depth,coupling,B", FORMS)
def test_prior_alone(lsnf, gpu_device, nz, w, depth, coupling, B):
    """(f) grad_g = energy_g = None equals zeros passed explicitly; the chain is then the prior alone, N(0, I) whatever the flow: two
    plans of one geometry with different weights give identical bits for every output."""
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c = lsnf.flow, gpu_device, s.c
    other = O.init_params(nz, w, depth, seed=11)
    other = K.additive(other) if coupling == 0 else other
    plan2 = lsnf.prepare(lsnf.params_from_state_dict(other, depth, dev), nz, w, depth, coupling)
    for r in (c.calls[0], c.calls[1], end_call(c)):
        ep = r.e_prop.float().to(dev)
        rng = None if r.phase == "inner" else F.PhiloxNoise(8, 9, 0)
        res = []
        for plan, gg, e in ((s.plan, None, None), (s.plan, torch.zeros_like(ep), torch.zeros(B, device=dev)), (plan2, None, None)):
            saved, act = stash_at(lsnf, plan, ep)
            state = state_for(lsnf, s, r)
            res.append((state, F.reverse_hmc_step(plan, ep, saved, act, gg, e, state, rng, c.s, phase=r.phase)))
        assert same(res[0], res[1]) and same(res[0], res[2])
        if r.phase == "init":
            assert bits(res[0][0].grad, ep)                              # g = 0: grad U is eps itself


# ---------------------------------------------------------------------------------------------
# 3. L = 1 against flow.reverse_mala_step, no oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", SMALL)
def test_one_leapfrog_step_is_the_reverse_mala_step(lsnf, gpu_device, nz, w, depth, coupling, B):
    """Both chains start at eps0 with the same noise; both then decide the SAME point (MALA's proposal, which is HMC's up to fp32
    rounding) with the same uniform and propose again with the same noise.  The state is the same bits, and so is U_prop (the same
    sum in the same order); the two log_alpha differ by the rounding of kin0 - kinL against (A - Bq) / (2 s^2), held to ONE end-call
    gate of (1) with kinL >= 0 left out of the scale, which only tightens it: 1e-5 (|u_acc| + |U_prop| + kin0)."""
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c, step = lsnf.flow, gpu_device, s.c, float(np.float32(STEP_L1[nz]))
    g = torch.Generator().manual_seed(5)
    eps0, xi = c.eps0.to(dev), [torch.randn(B, nz, generator=g).to(dev) for _ in range(2)]
    u = torch.rand(B, generator=g).clamp_min(2.0 ** -25).to(dev)

    def pot(eps):                                                          # (energy, gradient) of the quadratic at the float64 x
        return tuple(t.float().to(dev) for t in c.quad(RM.reverse_of(c.p, eps.cpu(), torch.float64)))
    e0, g0 = pot(eps0)
    hs, ms = F.new_hmc_state(s.plan, B, dev), F.new_mala_state(s.plan, B, dev)
    saved, act = stash_at(lsnf, s.plan, eps0)
    eh = F.reverse_hmc_step(s.plan, eps0, saved, act, g0, e0, hs, xi[0], step, phase="init")[0]
    em = F.reverse_mala_step(s.plan, eps0, saved, act, g0, e0, ms, xi[0], step, init=True)[0]
    assert bits(hs.z, ms.z) and bits(hs.grad, ms.grad) and bits(hs.energy, ms.energy)
    assert bool((rel_rows(eh.cpu(), em.cpu().double()) <= 2e-5).all())                       # the same proposal in exact arithmetic
    e1, g1 = pot(em)
    u_acc, kin0 = hs.energy.cpu().double(), hs.kin.cpu().double()
    assert bool(((kin0 - 0.5 * (xi[0].cpu().double() ** 2).sum(1)).abs() <= 1e-5 * kin0).all())
    saved, act = stash_at(lsnf, s.plan, em)
    eh2, acc_h, la_h = F.reverse_hmc_step(s.plan, em, saved, act, g1, e1, hs, xi[1], step, uniform=u)
    em2, acc_m, la_m = F.reverse_mala_step(s.plan, em, saved, act, g1, e1, ms, xi[1], step, uniform=u)
    la_h, la_m, lnu = la_h.cpu().double(), la_m.cpu().double(), torch.log(u.cpu().double())
    U_prop = e1.cpu().double() + 0.5 * (em.cpu().double() ** 2).sum(1)
    gate = 1e-5 * (u_acc.abs() + U_prop.abs() + kin0)
    decided = ((la_m - lnu).abs() > gate) & ((la_h - lnu).abs() > gate)
    print(f"[rhmc] {c.geo} B{B} L=1 against reverse_mala_step: worst |log_alpha difference| / gate = {fig((la_h - la_m).abs() / gate):.3f}, "
          f"{int((~decided).sum())} rows within the gate of ln u, {int(acc_m.sum())}/{B} accepted")
    assert bool(((la_h - la_m).abs() <= gate).all())
    assert torch.equal(acc_h.cpu()[decided], acc_m.cpu()[decided]) and int((~decided).sum()) <= max(2, B // 10)
    assert bool((rel_rows(eh2.cpu()[decided], em2.cpu().double()[decided]) <= 2e-5).all())
    assert 0 < int(acc_m.sum()) < B


# ---------------------------------------------------------------------------------------------
# 4. reversibility on the device
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", SMALL)
def test_a_trajectory_is_reversible_on_the_device(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c, step, L = lsnf.flow, gpu_device, s.c, s.c.s, s.c.L
    f32, f64 = torch.float32, torch.float64

    def ge64(eps):
        return c.quad(RM.reverse_of(c.p, eps.cpu(), f64))
    pot = lambda eps: tuple(t.float().to(dev) for t in ge64(eps))
    u = torch.full((B,), 0.5, device=dev)

    def there(e_start, p0):
        """init with noise = p0, L - 1 inner calls, an end call that proposes nothing: (eps_L, pL, log_alpha)."""
        st, ep = F.new_hmc_state(s.plan, B, dev), e_start
        for i in range(L + 1):
            e, gg = pot(ep)
            phase = "init" if i == 0 else "inner" if i < L else "end"
            saved, act = stash_at(lsnf, s.plan, ep)
            en, _, la = F.reverse_hmc_step(s.plan, ep, saved, act, gg, e, st, p0 if i == 0 else None, step, phase=phase,
                                           uniform=u if phase == "end" else None, propose=i < L)
            ep = en if en is not None else ep
        return ep, st.mom.clone(), la.cpu().double()
    eps0, p0 = c.eps0.to(dev), c.calls[0].noise.to(dev)
    eL, pL, la1 = there(eps0, p0)
    e_back, _, la2 = there(eL, -pL)

    # the fp32 restatement's own return error, from the same start
    def gradU32(eps):
        return eps + RM.pull_back(c.p, eps, ge64(eps)[1].to(f32), f32)

    def there32(ep, p):
        ph, ep, _ = RH.begin(ep, gradU32(ep), p, step)
        for _ in range(L - 1):
            ph, ep = RH.inner(ep, ph, gradU32(ep), step)
        return ep, RH.end(ph, gradU32(ep), step)[0]
    eL32, pL32 = there32(c.eps0.to(f32), c.calls[0].noise.to(f32))
    own = (there32(eL32, -pL32)[0].double() - c.eps0.double()).norm(dim=1)
    bound = torch.maximum(1e-5 * L * c.eps0.double().norm(dim=1), 3.0 * own)
    err = (e_back.cpu().double() - c.eps0.double()).norm(dim=1)
    # two gates of the end calls' log_alpha: the two directions have the same terms (U at the two ends in float64, the kinetic
    # energies of the two momenta the chains were given)
    kin0, kinL = 0.5 * (p0.cpu().double() ** 2).sum(1), 0.5 * (pL.cpu().double() ** 2).sum(1)
    U0, UL = c.calls[0].U_prop, RH.potential(c.p, eL.cpu().double(), c.quad, f64)[0]
    scale = U0.abs() + UL.abs() + kin0 + kinL
    print(f"[rhmc] {c.geo} B{B} reversibility: worst return error / bound = {fig(err / bound):.3f}, worst |la1 + la2| / (two gates) = "
          f"{fig((la1 + la2).abs() / (2e-5 * scale)):.3f}, largest |log_alpha| {fig(la1.abs()):.2f}")
    assert bool((err <= bound).all())
    assert bool(((la1 + la2).abs() <= 2e-5 * scale).all()) and fig(la1.abs()) > 1e-2


# ---------------------------------------------------------------------------------------------
# 5. a non-finite row stays alone
# ---------------------------------------------------------------------------------------------
def test_a_nan_row_is_rejected_and_alone(lsnf, gpu_device):
    s = setup_of(lsnf, gpu_device, *C3, 33)
    F, dev, c = lsnf.flow, gpu_device, s.c
    end = c.calls[c.L]
    bad, keep = 18, torch.arange(33, device=dev) != 18
    rng = F.PhiloxNoise(3, 4, 0)
    clean = run(lsnf, s, end, rng, None, propose=True)
    ge = end.ge.float().to(dev)
    ge[bad, 5] = float("nan")
    state = state_for(lsnf, s, end)
    before = clone_state(lsnf, state)
    _, (e_next, acc, la) = run(lsnf, s, end, rng, None, state=state, grad_g=ge, propose=True)
    assert acc[bad].item() == 0.0 and bool(torch.isnan(la[bad]))
    for f in ("z", "grad", "energy"):
        assert bits(getattr(state, f)[bad], getattr(before, f)[bad])
    assert bool(torch.isfinite(e_next[bad]).all()) and bool(torch.isfinite(state.mom[bad]).all()) and bool(torch.isfinite(state.kin[bad]))
    # ... and that restart is the begin of a rejected row: from (eps_acc, grad_acc), whatever the proposal was
    xi = F.sample(s.plan, 33, rng, want_eps=True)[2]
    ph = xi[bad] - (0.5 * c.s) * before.grad[bad]
    assert bits(state.mom[bad], ph) and bits(e_next[bad], before.z[bad] + c.s * ph)
    for got, ref in zip([getattr(state, f) for f in FIELDS] + [e_next, acc, la], [getattr(clean[0], f) for f in FIELDS] + list(clean[1])):
        assert bits(got[keep], ref[keep])
    assert 0 < int(acc[keep].sum()) < 32


def diverged_rows(c):
    """The first end call of a diverging case, and the rows whose float64 log_alpha is NaN, -inf or below -100."""
    r = c.calls[c.L]
    return r, torch.isnan(r.la) | (r.la < -100.0)


def diverging_call(c):
    """That end call with the rows T.GRAFTED given the inputs of the same case at its stable step, and the diverged rows of it."""
    stable = case(*c.geo, c.B, T.TRAINED)
    r = T.graft(c.calls[c.L], stable.calls[stable.L])
    return r, torch.isnan(r.la) | (r.la < -100.0)


def test_a_diverging_trajectory_is_rejected_and_alone(lsnf, gpu_device):
    """C3 at trained weights, step 0.1 (the smallest multiple of 0.05 at which the float64 gradient is NaN from the second inner call
    on: tests/trained_weights.py): the end call is given NaN points and momenta on 30 rows (three rows carry the stable case's
    inputs: GRAFTED).  Every diverged row is rejected with its state kept to the bit, and no other row's output differs from the call on
    those rows alone."""
    c = Case(*C3, 33, s=T.DIVERGING_STEP["hmc eps"], light=True, weights=T.TRAINED)
    r, bad = diverging_call(c)
    assert int(bad.sum()) >= T.DIVERGING_ROWS and not bool(bad[list(T.GRAFTED)].any())
    dev = gpu_device
    s = types.SimpleNamespace(c=c, dev=dev, plan=K.make_plan(lsnf, c, dev))
    state = state_for(lsnf, s, r)
    before = clone_state(lsnf, state)
    state, out = run(lsnf, s, r, state=state, propose=True)
    torch.cuda.synchronize()
    acc, la = out[1], out[2]
    bad_d = bad.to(dev)
    print(f"[rhmc] {c.geo} B33 trained s={c.s:.2f} diverging: {int(bad.sum())} rows diverged in float64, the device accepts "
          f"{int(acc[bad_d].sum())} of them; its log_alpha there: {int(torch.isnan(la[bad_d]).sum())} NaN, {int(torch.isinf(la[bad_d]).sum())} inf; "
          f"the {int((~bad).sum())} other rows: accepted {int(acc[~bad_d].sum())}")
    assert bool((acc[bad_d] == 0.0).all())
    for f in ("z", "grad", "energy"):
        assert bits(getattr(state, f)[bad_d], getattr(before, f)[bad_d])
    keep = torch.nonzero(~bad).flatten()                     # the rows that did not diverge, as a batch of their own
    assert keep.numel() == len(T.GRAFTED)
    alone_state, alone = run(lsnf, s, r, rows=keep, propose=True)
    whole = [getattr(state, f) for f in FIELDS] + list(out)
    for got, ref in zip(whole, [getattr(alone_state, f) for f in FIELDS] + list(alone)):
        assert (got is None) == (ref is None)
        if got is not None:
            assert bits(got[keep.to(dev)], ref) and bool(torch.isfinite(ref).all())


# ---------------------------------------------------------------------------------------------
# 6. a chain replayed from captured graphs
# ---------------------------------------------------------------------------------------------
def test_graphed_chain_is_the_eager_chain(lsnf, gpu_device):
    """The stash-keeping reverse, ToyG's energy and gradient and `reverse_hmc_step` in place on static buffers, captured once per
    call form (init; inner; end that begins the next trajectory; end that proposes nothing) on one stream, the draws from a
    device-side counter the graphs advance themselves; K L + 1 replays against the eager loop of the same calls."""
    nz, w, depth, B, Kt, L, s, sigma = 20, 12, 5, 37, 2, 3, 0.4, 0.3
    p = O.init_params(nz, w, depth, seed=8)
    dev, F = gpu_device, lsnf.flow
    net = K.module_of(lsnf, p, dev, False)
    plan = net._plan()
    assert F.reverse_keep_supported(plan, B)
    torch.manual_seed(0)
    netG = ToyG(nz).to(dev)
    for q in netG.parameters():
        q.requires_grad_(False)
    x = torch.tanh(torch.randn(B, 3, 4, 4)).to(dev)
    eps0 = torch.randn(B, nz).to(dev)
    f32 = dict(dtype=torch.float32, device=dev)

    class Buffers:
        def __init__(self):
            self.eps, self.z, self.obj = torch.zeros(B, nz, **f32), torch.zeros(B, nz, **f32), torch.zeros(B, **f32)
            self.saved, self.act = torch.zeros(depth - 1, B, nz, **f32), F.new_act_saved(plan, B, dev)
            self.state = F.new_hmc_state(plan, B, dev)

    def step(b, phase, propose, noise):
        with torch.no_grad():
            F.reverse(plan, b.eps, None, out=(b.z, b.obj), act_saved=b.act, z_saved_out=b.saved)
        zr = b.z.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = 1.0 / (2.0 * sigma * sigma) * ((netG(zr) - x) ** 2).flatten(1).sum(1)
        gg = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()
        with torch.no_grad():
            _, acc, la = F.reverse_hmc_step(plan, b.eps, b.saved, b.act, gg, energy.detach(), b.state, noise, s, phase=phase,
                                            propose=propose, inplace=True)
        return acc, la
    forms = [("init", True) if j == 0 else ("inner", True) if j % L else ("end", j < Kt * L) for j in range(Kt * L + 1)]
    # eager
    be = Buffers()
    be.eps.copy_(eps0)
    eager = []
    for j, (phase, propose) in enumerate(forms):
        acc, la = step(be, phase, propose, None if phase == "inner" else F.PhiloxNoise(21, 300 + j // L, 0))
        if phase != "inner":
            eager.append((acc.clone(), la.clone()))
    # graphed: one capture per call form
    bg = Buffers()
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    rng = F.PhiloxNoise(21, 0, 0, offset_dev=ctr)

    def graphed_step(form):
        phase, propose = form
        out = step(bg, phase, propose, None if phase == "inner" else rng)
        if phase != "inner":
            ctr.add_(1)
        return out
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                            # warm-up off the capture stream
        bg.eps.copy_(eps0)
        for form in forms:
            graphed_step(form)
    torch.cuda.current_stream(dev).wait_stream(side)
    graphs, outs = {}, {}
    for form in dict.fromkeys(forms):
        graphs[form] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[form]):
            outs[form] = graphed_step(form)
    assert len(graphs) == 4
    bg.eps.copy_(eps0); ctr.fill_(300)
    got = []
    for form in forms:
        graphs[form].replay()
        if form[0] != "inner":
            got.append(tuple(t.clone() for t in outs[form]))
    torch.cuda.synchronize()
    assert int(ctr.item()) == 300 + Kt + 1
    for (a_g, l_g), (a_e, l_e) in zip(got, eager):
        assert bits(a_g, a_e) and bits(l_g, l_e)
    assert bits(bg.eps, be.eps) and all(bits(getattr(bg.state, f), getattr(be.state, f)) for f in FIELDS)
    assert 0 < int(sum(a.sum() for a, _ in eager[1:])) < Kt * B


# ---------------------------------------------------------------------------------------------
# 7. the sampler
# ---------------------------------------------------------------------------------------------
def test_sampler_is_the_hand_written_loop(lsnf, gpu_device):
    nz, w, B, Ks, L, s, sigma = 20, 12, 37, 3, 2, 0.6, 0.3
    p = O.init_params(nz, w, 5, seed=8)
    dev, F, Lv = gpu_device, lsnf.flow, lsnf.langevin
    net = K.module_of(lsnf, p, dev, False)
    torch.manual_seed(0)
    netG = ToyG(nz).to(dev)
    x = torch.tanh(torch.randn(B, 3, 4, 4)).to(dev)
    eps0 = torch.randn(B, nz, 1, 1).to(dev)
    ph = F.PhiloxNoise(77, 1000, 0)
    kw = dict(leapfrog_steps=L, g_l_step_size=s, g_llhd_sigma=sigma)
    eps_k, z_k, rate, u_k = Lv.sample_hmc_post_eps_with_flow(eps0, x, netG, net, g_l_steps=Ks, philox=ph, **kw)
    torch.cuda.synchronize()
    assert ph.offset == 1000 + Ks + 1 and eps_k.shape == (B, nz) and z_k.shape == (B, nz, 1, 1) and rate.shape == (B,) and u_k.shape == (B,)
    assert all(bool(torch.isfinite(t).all()) for t in (eps_k, z_k, rate, u_k))
    plan = net._plan()
    assert bits(z_k.view(B, nz), F.reverse(plan, eps_k, None)[0])
    # by hand: K L + 1 calls, the call that starts trajectory t + 1 at offset + t
    state, ep, flags = F.new_hmc_state(plan, B, dev), eps0.view(B, nz).clone(), []
    for j in range(Ks * L + 1):
        act = F.new_act_saved(plan, B, dev)
        z, _, saved = F.reverse(plan, ep, None, save_for_backward=True, act_saved=act)
        zr = z.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = 1.0 / (2.0 * sigma * sigma) * ((netG(zr) - x) ** 2).flatten(1).sum(1)
        gg = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()
        inner = j % L != 0
        ep, acc, _ = F.reverse_hmc_step(plan, ep, saved, act, gg, energy.detach(), state, None if inner else F.PhiloxNoise(77, 1000 + j // L, 0), s,
                                        phase="inner" if inner else "end" if j else "init", propose=j < Ks * L)
        if j and not inner:
            flags.append(acc.clone())
    assert ep is None and len(flags) == Ks
    flags = torch.stack(flags)
    assert bits(eps_k, state.z) and bits(u_k, state.energy) and bits(rate, flags.sum(0) / Ks)
    assert 0.0 < rate.mean().item() < 1.0
    print(f"[rhmc] sampler nz={nz} B={B} s={s} L={L}: mean acceptance {rate.mean().item():.2f}")
    # no trajectory, or no rows: the input, without a launch
    ph = F.PhiloxNoise(77, 1000, 0)
    none = Lv.sample_hmc_post_eps_with_flow(eps0, x, netG, net, g_l_steps=0, philox=ph, **kw)
    assert torch.equal(none[0], eps0.view(B, nz)) and none[2] is None and none[3] is None and ph.offset == 1000
    empty = Lv.sample_hmc_post_eps_with_flow(eps0[:0], x[:0], netG, net, g_l_steps=Ks, philox=ph, **kw)
    assert empty[0].shape == (0, nz) and empty[2] is None and ph.offset == 1000

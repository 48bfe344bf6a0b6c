"""GPU: Hamiltonian Monte Carlo in z (lsnf_hmc_step, lsnf_small3_hmc_kernel: the latency bf16x3 backward with the leapfrog tail as its
output section), `flow.hmc_step`, `_netF.hmc_step` and `langevin.sample_hmc_post_z_with_flow`.

Against float64 every call is TEACHER-FORCED: the device is given the fp32 casts of the float64 restatement's inputs of that call
(tests/hmc_restated.py: state, momentum, kin0, the point, grad_g / energy_g of the closed-form quadratic, noise, uniform), so a
decision that differs on one row cannot move a later call's inputs.  Momentum draws of which any point of the trajectory would land
within 2e-5 of a ReLU kink are redrawn on the CPU.  L = 3; two trajectories (7 calls) for B <= 100, above that one init, one inner
and one end call (the CPU computes the whole trajectory; the device is not given its second inner call).  Per row of an end call
    gate = max(1e-5 * (|u_acc| + |U_prop| + kin0 + kinL), 3 * |fp32 restatement - fp64 restatement|);
rows whose float64 log_alpha is within the gate of ln u, and rows with oracle.relu_margin <= 2e-5 at the call's point, are set aside
(at most 10 % of a case, 2 rows for B <= 33: asserted on the CPU and again with the device's figures).  Every call that proposes:
z_next rel-L2 <= 1e-5, |mom - fp64| <= 1e-5 (|mom_in or xi| + s |g|), kin0 relative <= 1e-5 per row, each widened to 3 x the fp32
restatement's own error where that exceeds a third of it (printed).  Step sizes are chosen per nz (per geometry for the entries of
tests/chain_geometries.py -- ragged halves, whole tiles of padding -- which CASES, PHILOX_CASES and FORMS append) on the CPU from the float64
restatement alone so that the two-trajectory cases accept between 15 % and 85 % of their decisions (asserted).  Everything else is
bit identity between call forms, or the device against itself."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import flow_oracle as O
import chain_geometries as G
import hmc_restated as H
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
# step size by nz, chosen on the CPU from the float64 restatement alone (tests/hmc_restated.py, L = 3)
STEP = {128: 0.8, 126: 0.84, 100: 0.9, 64: 1.0, 20: 1.0, 8: 1.2, 2: 0.48}
# The geometries of tests/chain_geometries.py are keyed whole (nz 66 and 128 occur with two widths), chosen the same way: Case.rate of
# the two-trajectory case of 33 rows scanned over s = 0.30, 0.35, ... 1.50; the step whose rate is nearest one half (the smaller of
# two).  At nz >= 124 the rate falls from 0.9 to nothing within 0.2 of step size.  Rates found, in the table's order: 0.39 / 0.36 /
# 0.64 / 0.62 / 0.61 / 0.38 / 0.50 / 0.62 / 0.68 (profiles/chain_geometries.txt).
STEP_GEO = {(62, 31, 2, 1): 1.05, (66, 33, 2, 1): 1.05, (124, 63, 3, 1): 0.8, (66, 33, 3, 0): 0.95, (10, 40, 2, 1): 1.25, (70, 8, 2, 1): 1.05,
            (12, 100, 2, 1): 1.2, (66, 65, 2, 1): 1.0, (128, 128, 2, 1): 0.8}
# seed offset of a case's generator, to be chosen on the CPU (float64 / float32 restatements alone) should the default draws leave a
# two-trajectory case outside 15 % .. 85 % (B = 1 has two decisions: exactly one must accept) or set aside more rows than allowed
# (Case asserts the latter): none needed with the steps above
SEED = {}
STEP_L1 = {128: 0.9, 8: 1.2}                                 # L = 1 against mala_step: tests/test_gpu_mala.py's steps
QUAD_SCALE = {2: 2.0}                                        # (tests/test_gpu_mala.py: at nz = 2 the u_acc bound needs an energy of order 1)


def step_of(nz, geo=None, weights=T.INIT):
    if weights != T.INIT:
        return float(np.float32(T.step_of("hmc z", geo)))                          # tests/trained_weights.py
    return float(np.float32(STEP_GEO[geo] if geo in STEP_GEO else STEP[nz]))      # the fp32 step the kernel sees


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
    """One geometry and batch on the CPU: the float64 chain's call records, each with its fp32 restatement, gates and row sets."""

    def __init__(self, nz, w, depth, coupling, B, weights=T.INIT, s=None, diverging=False):
        self.geo, self.B, self.nz, self.depth, self.weights = (nz, w, depth, coupling), B, nz, depth, weights
        p = T.params_for(O, self.geo, weights)
        self.p = K.additive(p) if coupling == 0 else p
        self.s, self.L = step_of(nz, self.geo, weights) if s is None else float(np.float32(s)), L_STEPS
        self.n_traj = 2 if B <= 100 else 1
        self.quad = H.Quadratic(nz, QUAD_SCALE.get(nz, 0.1), seed=7 + nz)
        g = torch.Generator().manual_seed(7 + B + SEED.get(self.geo + (B,), 0))
        self.z0, _ = O.smooth_batch(self.p, B, nz, seed=1007 + B)
        noises = [torch.randn(B, nz, generator=g) for _ in range(self.n_traj)] + [None]
        uniforms = [None] + [torch.rand(B, generator=g).clamp_min(2.0 ** -25) for _ in range(self.n_traj)]
        self.calls, _ = H.chain(self.p, self.z0, self.quad, self.s, self.L, noises, uniforms, redraw=g)
        self.allowed = 2 if B <= 33 else B // 10
        if diverging:                                        # the records alone: no rate, gate or row set holds on a diverged trajectory
            return
        s = self.s
        for c in self.calls:
            c.o32 = o = H.call32(self.p, c, self.quad, s)
            c.margin = O.relu_margin(self.p, c.z_prop.float())
            c.smooth = c.margin > 2e-5
            c.decided = c.smooth
            if c.phase != "inner":                           # the u_acc bound can be met in fp32 on these inputs (tests/test_gpu_mala.py)
                own = (o.U_prop.double() - c.U_prop).abs()
                assert bool((own <= 1e-5 * (c.e.abs() + c.ll.abs()) / 3.0)[c.acc].all()), "the u_acc bound is below fp32 on these inputs"
            if c.phase == "end":
                c.scale = c.u_acc.abs() + c.U_prop.abs() + c.kin_in + c.kinL
                c.gate = torch.maximum(1e-5 * c.scale, 3.0 * (o.la.double() - c.la).abs())
                c.decided = c.smooth & ((c.la - torch.log(c.u.double())).abs() > c.gate)
                assert int((~c.decided).sum()) <= self.allowed, "too many rows set aside: choose another seed"
            # the bounds of a call that proposes / leaves a momentum, from float64 and the fp32 restatement alone
            if c.mom_out is not None and c.phase != "init" or c.z_next is not None:
                src = c.noise.double() if c.noise is not None else c.mom_in
                gg = c.g_after if c.noise is not None else c.g
                c.mom_bound, c.mom_wide = widened(1e-5 * (src.norm(dim=1) + s * gg.norm(dim=1)), (o.mom_out.double() - c.mom_out).norm(dim=1))
            if c.z_next is not None:
                c.z_bound, c.z_wide = widened(torch.full((B,), 1e-5, dtype=torch.float64), rel_rows(o.z_next, c.z_next))
            if c.noise is not None:
                c.kin_bound, c.kin_wide = widened(1e-5 * c.kin_out, (o.kin_out.double() - c.kin_out).abs())
        ends = [c for c in self.calls if c.phase == "end"]
        self.rate = torch.stack([c.acc for c in ends]).double().mean().item()
        # what the device is given: every call for B <= 100, else init, the first inner call and the end call
        self.device_calls = self.calls if B <= 100 else [self.calls[0], self.calls[1], self.calls[self.L]]


@functools.lru_cache(maxsize=None)
def case(nz, w, depth, coupling, B, weights=T.INIT):
    return Case(nz, w, depth, coupling, B, weights)


class Setup:
    """A case's plan on the device (made under the run's math mode, as its forward's stash will be)."""

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


def state_for(lsnf, s, c, rows=slice(None)):
    """The HmcState a recorded call is given: the fp32 casts of the float64 state, momentum and kin0 before it.  What the call must
    not read is NaN: the whole state for init, z / grad / energy / kin for an inner call."""
    B, nz, dev = c.z_prop[rows].shape[0], s.c.nz, s.dev
    nan_rows, nan_one = (lambda: torch.full((B, nz), float("nan"), device=dev)), (lambda: torch.full((B,), float("nan"), device=dev))
    cut = lambda t: t[rows].float().to(dev).contiguous()
    if c.phase == "init":
        return lsnf.flow.HmcState(nan_rows(), nan_rows(), nan_one(), nan_rows(), nan_one())
    if c.phase == "inner":
        return lsnf.flow.HmcState(nan_rows(), nan_rows(), nan_one(), cut(c.mom_in), nan_one())
    return lsnf.flow.HmcState(cut(c.z_acc), cut(c.g_acc), cut(c.u_acc), cut(c.mom_in), cut(c.kin_in))


def run(lsnf, s, c, noise="record", uniform="record", rows=slice(None), state=None, **kw):
    """The recorded call c on its rows `rows` from its inputs' casts: (state after, outputs).  noise / uniform "record": the record's."""
    dev, cut = s.dev, (lambda t: None if t is None else t[rows].float().to(s.dev).contiguous())
    state = state_for(lsnf, s, c, rows) if state is None else state
    noise = cut(c.noise) if isinstance(noise, str) else noise
    uniform = cut(c.u) if isinstance(uniform, str) else uniform
    kw.setdefault("propose", c.z_next is not None)
    out = lsnf.flow.hmc_step(s.plan, cut(c.z_prop), cut(c.ge), cut(c.e), state, noise, s.c.s, phase=c.phase, uniform=uniform, **kw)
    return state, out


def same(a, b):
    """Two (state, outputs) results hold the same bits."""
    (sa, oa), (sb, ob) = a, b
    xs = [getattr(sa, f) for f in FIELDS] + list(oa)
    ys = [getattr(sb, f) for f in FIELDS] + list(ob)
    return all((x is None and y is None) or bits(x, y) for x, y in zip(xs, ys))


fig = lambda t: t.max().item() if t.numel() else 0.0


# ---------------------------------------------------------------------------------------------
# 1. against float64, teacher-forced
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B,mode", RUNS)
def test_every_call_follows_float64(lsnf, gpu_device, math, nz, w, depth, coupling, B, mode, weights=T.INIT):
    math(mode)
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, mode, weights)
    c = s.c
    tag = f"[hmc] {mode} {c.geo} B{B}" + ("" if weights == T.INIT else f" {weights}")
    print(f"{tag} s={c.s:.3f} L={c.L}: float64 accepts {100 * c.rate:.0f} % of {c.n_traj} x {B} decisions")
    if c.n_traj > 1:
        assert 0.15 <= c.rate <= 0.85
    for j, r in enumerate(c.device_calls):
        state = state_for(lsnf, s, r)
        before = clone_state(lsnf, state)
        state, (z_next, acc, la, ll) = run(lsnf, s, r, state=state)
        torch.cuda.synchronize()
        za, ga, ua, mom, kin = (getattr(state, f).cpu() for f in FIELDS)
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
                worst = fig((err / r.gate)[r.smooth])
                print(f"{name}: accepted {int(a64.sum())}/{B}, set aside {aside} (allowed {c.allowed}; {int((~r.smooth).sum())} near a kink), "
                      f"worst |log_alpha - fp64| / gate = {worst:.3f}, fp32 restatement worst {fig((r.o32.la.double() - r.la).abs() / r.gate):.3f}")
                assert aside <= c.allowed
                if weights != T.INIT:                        # the same share from the device's own log_alpha, together with the kink rows
                    aside_dev = int((~r.smooth | ((la.cpu().double() - torch.log(r.u.double())).abs() <= r.gate)).sum())
                    print(f"{name}: set aside by the device's log_alpha {aside_dev}")
                    assert aside_dev <= c.allowed
                assert bool((err <= r.gate)[r.smooth].all())
                assert torch.equal(acc_c[d] == 1.0, a64[d])
            yes, no = d & a64, d & ~a64
            ub = 1e-5 * (r.e.abs() + r.ll.abs())
            print(f"{name}: worst u_acc error / (1e-5 (|e| + |ll|)) = {fig(((ua.double() - r.U_prop).abs() / ub)[yes]):.3f}, "
                  f"grad_acc rel-L2 {fig(rel_rows(ga[yes], r.g[yes])):.2e} (allowed 1e-5)")
            assert bits(za[yes], r.z_prop.float()[yes])
            assert bool(((ua.double() - r.U_prop).abs() <= ub)[yes].all())
            assert bool((rel_rows(ga[yes], r.g[yes]) <= 1e-5).all())
            if r.phase == "end":
                bz, bg, bu = before.z.cpu(), before.grad.cpu(), before.energy.cpu()
                assert bits(za[no], bz[no]) and bits(ga[no], bg[no]) and bits(ua[no], bu[no])
        d = r.decided
        if hasattr(r, "mom_bound"):
            e = (mom.double() - r.mom_out).norm(dim=1)
            print(f"{name}: worst |mom - fp64| / bound = {fig((e / r.mom_bound)[d]):.3f} ({r.mom_wide} rows widened by the fp32 restatement)")
            assert bool((e <= r.mom_bound)[d].all())
        if r.z_next is not None:
            e = rel_rows(z_next.cpu(), r.z_next)
            print(f"{name}: worst z_next rel-L2 / bound = {fig((e / r.z_bound)[d]):.3f} ({r.z_wide} rows widened)")
            assert bool((e <= r.z_bound)[d].all())
        else:
            assert z_next is None
        if r.noise is not None:
            e = (kin.double() - r.kin_out).abs()
            print(f"{name}: worst kin0 error / bound = {fig(e / r.kin_bound):.3f} ({r.kin_wide} rows widened)")
            assert bool((e <= r.kin_bound).all())
        elif r.phase != "init":
            assert bits(state.kin, before.kin)                                    # no trajectory begun: kin0 is left as it is


@pytest.mark.parametrize("nz,w,depth,coupling,B", T.CASES)
def test_every_call_follows_float64_at_trained_weights(lsnf, gpu_device, math, nz, w, depth, coupling, B):
    """The same calls, gates and caps on the golden trained weights (tests/trained_weights.py): a saturating sigmoid, |3 logs| up to 2,
    |grad log p| of order 1e3, steps from the narrow window in which the float64 leapfrog is stable there."""
    test_every_call_follows_float64(lsnf, gpu_device, math, nz, w, depth, coupling, B, "default", weights=T.TRAINED)


SMALL = [C3 + (33,), C3 + (4100,), C3 + (8200,), TINY + (33,)]
PHILOX_CASES = SMALL + G.CASES                               # the in-kernel draw against the tensor form
FORMS = SMALL + G.FORMS                                      # in place, 4 bytes off, NULL optionals


def end_call(c):
    """The first end call of a case (B <= 100: it begins the next trajectory; above: it proposes nothing)."""
    return next(r for r in c.calls if r.phase == "end")


# ---------------------------------------------------------------------------------------------
# 2. L = 1 against flow.mala_step, no oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", SMALL)
def test_one_leapfrog_step_is_the_mala_step(lsnf, gpu_device, nz, w, depth, coupling, B):
    """Both chains start at z0 with the same noise; both then decide the SAME point (MALA's proposal, which is HMC's up to fp32
    rounding) with the same uniform and propose again with the same noise.  The state is the same bits, so |u_acc| and |U_prop| are;
    kinL >= 0 is left out of the scale, which only tightens the bound: two gates >= 2e-5 (|u_acc| + |U_prop| + kin0)."""
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c, step = lsnf.flow, gpu_device, s.c, float(np.float32(STEP_L1[nz]))
    g = torch.Generator().manual_seed(5)
    z0, xi = c.z0.to(dev), [torch.randn(B, nz, generator=g).to(dev) for _ in range(2)]
    u = torch.rand(B, generator=g).clamp_min(2.0 ** -25).to(dev)
    pot = lambda z: tuple(t.float().to(dev) for t in c.quad(z.cpu().double()))               # (energy, gradient) of the quadratic
    e0, g0 = pot(z0)
    hs, ms = F.new_hmc_state(s.plan, B, dev), F.new_mala_state(s.plan, B, dev)
    zh = F.hmc_step(s.plan, z0, g0, e0, hs, xi[0], step, phase="init")[0]
    zm = F.mala_step(s.plan, z0, g0, e0, ms, xi[0], step, init=True)[0]
    assert bits(hs.z, ms.z) and bits(hs.grad, ms.grad) and bits(hs.energy, ms.energy)
    assert bool((rel_rows(zh.cpu(), zm.cpu().double()) <= 2e-5).all())                       # the same proposal in exact arithmetic
    e1, g1 = pot(zm)
    u_acc, kin0 = hs.energy.cpu().double(), hs.kin.cpu().double()
    assert bool(((kin0 - 0.5 * (xi[0].cpu().double() ** 2).sum(1)).abs() <= 1e-5 * kin0).all())
    zh2, acc_h, la_h, ll_h = F.hmc_step(s.plan, zm, g1, e1, hs, xi[1], step, uniform=u)
    zm2, acc_m, la_m, ll_m = F.mala_step(s.plan, zm, g1, e1, ms, xi[1], step, uniform=u)
    assert bits(ll_h, ll_m)
    la_h, la_m, lnu = la_h.cpu().double(), la_m.cpu().double(), torch.log(u.cpu().double())
    gate = 2e-5 * (u_acc.abs() + (e1.cpu().double() - ll_m.cpu().double()).abs() + kin0)
    decided = ((la_m - lnu).abs() > gate) & ((la_h - lnu).abs() > gate)
    print(f"[hmc] {c.geo} B{B} L=1 against mala_step: worst |log_alpha difference| / (two gates) = {fig((la_h - la_m).abs() / gate):.3f}, "
          f"{int((~decided).sum())} rows within the gates of ln u, {int(acc_m.sum())}/{B} accepted")
    assert bool(((la_h - la_m).abs() <= gate).all())
    assert torch.equal(acc_h.cpu()[decided], acc_m.cpu()[decided]) and int((~decided).sum()) <= max(2, B // 10)
    assert bool((rel_rows(zh2.cpu()[decided], zm2.cpu().double()[decided]) <= 2e-5).all())
    assert 0 < int(acc_m.sum()) < B


# ---------------------------------------------------------------------------------------------
# 3. reversibility on the device
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", SMALL)
def test_a_trajectory_is_reversible_on_the_device(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c, step, L = lsnf.flow, gpu_device, s.c, s.c.s, s.c.L
    pot = lambda z: tuple(t.float().to(dev) for t in c.quad(z.cpu().double()))
    u = torch.full((B,), 0.5, device=dev)

    def there(z_start, p0):
        """init with noise = p0, L - 1 inner calls, an end call that proposes nothing: (z_L, pL, log_alpha)."""
        st, z = F.new_hmc_state(s.plan, B, dev), z_start
        for i in range(L + 1):
            e, gg = pot(z)
            phase = "init" if i == 0 else "inner" if i < L else "end"
            zn, _, la, _ = F.hmc_step(s.plan, z, gg, e, st, p0 if i == 0 else None, step, phase=phase,
                                      uniform=u if phase == "end" else None, propose=i < L)
            z = zn if zn is not None else z
        return z, st.mom.clone(), la.cpu().double()
    z0, p0 = c.z0.to(dev), c.calls[0].noise.to(dev)
    zL, pL, la1 = there(z0, p0)
    z_back, _, la2 = there(zL, -pL)
    # the fp32 restatement's own return error, from the same start
    f32 = torch.float32
    q = O.to_dtype(c.p, f32)

    def gradU32(z):
        return c.quad(z.double())[1].to(f32) + O.grad_neg_sum_ll_wrt_z(q, z)

    def there32(z, p):
        ph, z, _ = H.begin(z, gradU32(z), p, step)
        for _ in range(L - 1):
            ph, z = H.inner(z, ph, gradU32(z), step)
        return z, H.end(ph, gradU32(z), step)[0]
    zL32, pL32 = there32(c.z0.to(f32), c.calls[0].noise.to(f32))
    own = (there32(zL32, -pL32)[0].double() - c.z0.double()).norm(dim=1)
    bound = torch.maximum(1e-5 * L * c.z0.double().norm(dim=1), 3.0 * own)
    err = (z_back.cpu().double() - c.z0.double()).norm(dim=1)
    # two gates of the end calls' log_alpha: the two directions have the same terms (U at the two ends in float64, the kinetic
    # energies of the two momenta the chains were given)
    kin0, kinL = 0.5 * (p0.cpu().double() ** 2).sum(1), 0.5 * (pL.cpu().double() ** 2).sum(1)
    U0, UL = c.calls[0].U_prop, H.potential(c.p, zL.cpu().double(), c.quad, torch.float64)[0]
    scale = U0.abs() + UL.abs() + kin0 + kinL
    print(f"[hmc] {c.geo} B{B} reversibility: worst return error / bound = {fig(err / bound):.3f}, worst |la1 + la2| / (two gates) = "
          f"{fig((la1 + la2).abs() / (2e-5 * scale)):.3f}, largest |log_alpha| {fig(la1.abs()):.2f}")
    assert bool((err <= bound).all())
    assert bool(((la1 + la2).abs() <= 2e-5 * scale).all()) and fig(la1.abs()) > 1e-2


# ---------------------------------------------------------------------------------------------
# 4. bit identities
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", PHILOX_CASES)
def test_philox_is_the_tensors_of_the_same_draws(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c = lsnf.flow, gpu_device, s.c
    for r in (c.calls[0], end_call(c)):
        for row0 in (0, 2 ** 32 - 5):
            rng = F.PhiloxNoise(1234, 40, row0)
            xi = F.sample(s.plan, B, rng, want_eps=True)[2]
            u = None if r.phase == "init" else torch.from_numpy(H.uniform_draws(B, 1234, 40, row0)).to(dev)
            got, ref = run(lsnf, s, r, rng, None, propose=True), run(lsnf, s, r, xi, u, propose=True)
            # kin0 is 1/2 sum xi^2 over the nz real columns: the draw of a padding column (a half that is no multiple of 4) is not in it
            x64 = xi.cpu().double()
            kin64, kin32 = 0.5 * (x64 ** 2).sum(1), 0.5 * (xi.cpu() ** 2).sum(1)
            bound, _ = widened(1e-5 * kin64, (kin32.double() - kin64).abs())              # Case's kin_bound, at these draws
            kin_err = (got[0].kin.cpu().double() - kin64).abs()
            print(f"[hmc] {c.geo} B{B} {r.phase} row0 {row0}: in-kernel draw, worst kin0 error / bound = {fig(kin_err / bound):.3f}, "
                  f"kin0 the tensor form's bits: {bits(got[0].kin, ref[0].kin)}")
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
# every instantiation of lsnf_small3_hmc_kernel that the default dispatch can reach)
@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (8200,), TINY + (4100,), TINY + (8200,), C5 + (4100,)] + G.LARGE)
def test_rows_do_not_depend_on_the_batch_or_the_sharding(lsnf, gpu_device, nz, w, depth, coupling, B):
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
        state, zp = state_for(lsnf, s, r), r.z_prop.float().to(dev)
        out = F.hmc_step(s.plan, zp, r.ge.float().to(dev), r.e.float().to(dev), state, noise, c.s, phase=r.phase, uniform=u, inplace=True)
        assert out[0].data_ptr() == zp.data_ptr() and same((state, out), ref)
        # the Philox form in place as well
        if not inner:
            rng = F.PhiloxNoise(5, 6, 7)
            ref2 = run(lsnf, s, r, rng, None, propose=True)
            state, zp = state_for(lsnf, s, r), r.z_prop.float().to(dev)
            out = F.hmc_step(s.plan, zp, r.ge.float().to(dev), r.e.float().to(dev), state, rng, c.s, phase=r.phase, inplace=True)
            assert same((state, out), ref2)
        # every tensor 4 bytes off a 16-byte boundary
        st = state_for(lsnf, s, r)
        state = F.HmcState(*(off4(getattr(st, f)) for f in FIELDS))
        out = F.hmc_step(s.plan, off4(r.z_prop), off4(r.ge), off4(r.e), state, off4(noise), c.s, phase=r.phase, uniform=off4(u), inplace=True)
        assert same((state, out), ref)
    with pytest.raises(lsnf.LsnfError):                                 # no other output may be an input
        st = state_for(lsnf, s, r)
        F.hmc_step(s.plan, zp, r.ge.float().to(dev), r.e.float().to(dev), F.HmcState(zp, st.grad, st.energy, st.mom, st.kin), noise, c.s, uniform=u)


@pytest.mark.parametrize("nz,w,depth,coupling,B", FORMS)
def test_null_gradient_and_energy_are_zeros(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c = lsnf.flow, gpu_device, s.c
    for r in (c.calls[0], c.calls[1], end_call(c)):
        zp = r.z_prop.float().to(dev)
        rng = None if r.phase == "inner" else F.PhiloxNoise(8, 9, 0)
        res = []
        for gg, e in ((None, None), (torch.zeros_like(zp), torch.zeros(B, device=dev))):
            state = state_for(lsnf, s, r)
            res.append((state, F.hmc_step(s.plan, zp, gg, e, state, rng, c.s, phase=r.phase)))
        assert same(res[0], res[1])


# ---------------------------------------------------------------------------------------------
# 5. a non-finite row stays alone
# ---------------------------------------------------------------------------------------------
def test_a_nan_row_is_rejected_and_alone(lsnf, gpu_device):
    s = setup_of(lsnf, gpu_device, *C3, 33)
    F, dev, c = lsnf.flow, gpu_device, s.c
    inner, end = c.calls[1], c.calls[c.L]
    bad, keep = 18, torch.arange(33, device=dev) != 18
    # the inner call: the row is NaN in mom and z_next, no other row changes a bit
    clean = run(lsnf, s, inner)
    zp = inner.z_prop.float().to(dev)
    zp[bad, 5] = float("nan")
    state = state_for(lsnf, s, inner)
    z_next = F.hmc_step(s.plan, zp, inner.ge.float().to(dev), inner.e.float().to(dev), state, None, c.s, phase="inner")[0]
    assert bool(torch.isnan(z_next[bad]).all()) and bool(torch.isnan(state.mom[bad]).all())
    assert bits(z_next[keep], clean[1][0][keep]) and bits(state.mom[keep], clean[0].mom[keep])
    # the end call with that row's NaN momentum: rejected with a NaN log_alpha, its state kept, the next trajectory begun from its state
    rng = F.PhiloxNoise(3, 4, 0)
    clean = run(lsnf, s, end, rng, None, propose=True)
    state = state_for(lsnf, s, end)
    state.mom[bad] = float("nan")
    before = clone_state(lsnf, state)
    z_next, acc, la, ll = F.hmc_step(s.plan, end.z_prop.float().to(dev), end.ge.float().to(dev), end.e.float().to(dev), state, rng, c.s)
    assert acc[bad].item() == 0.0 and bool(torch.isnan(la[bad]))
    for f in ("z", "grad", "energy"):
        assert bits(getattr(state, f)[bad], getattr(before, f)[bad])
    assert bool(torch.isfinite(z_next[bad]).all()) and bool(torch.isfinite(state.mom[bad]).all()) and bool(torch.isfinite(state.kin[bad]))
    # ... and that restart is the begin of a rejected row: from (z_acc, grad_acc), whatever the proposal was
    xi = F.sample(s.plan, 33, rng, want_eps=True)[2]
    ph = xi[bad] - (0.5 * c.s) * before.grad[bad]
    assert bits(state.mom[bad], ph) and bits(z_next[bad], before.z[bad] + c.s * ph)
    for got, ref in zip([getattr(state, f) for f in FIELDS] + [z_next, acc, la, ll], [getattr(clean[0], f) for f in FIELDS] + list(clean[1])):
        assert bits(got[keep], ref[keep])


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
    """C3 at trained weights, step 0.2: in float64 |z| grows 13 -> 79 -> 2.9e3 over the three leapfrog steps, ll = -inf and the gradient
    is NaN from the second inner call on, so the end call is given NaN points, infinite energies and momenta of order 1e5 on 30 rows
    (three rows carry the stable case's inputs: tests/trained_weights.py GRAFTED).  Every diverged row is rejected with its state kept
    to the bit, and no other row's output differs from the call on those rows alone."""
    c = Case(*C3, 33, weights=T.TRAINED, s=T.DIVERGING_STEP["hmc z"], diverging=True)
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
    print(f"[hmc] {c.geo} B33 trained s={c.s:.2f} diverging: {int(bad.sum())} rows diverged in float64, the device accepts "
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
# 6. a chain captured in a graph
# ---------------------------------------------------------------------------------------------
def test_graphed_chain_is_the_eager_chain(lsnf, gpu_device):
    nz, w, depth, coupling, B = C3 + (100,)
    c = case(nz, w, depth, coupling, B)
    dev, F = gpu_device, lsnf.flow
    net = K.module_of(lsnf, c.p, dev, False)
    z0, s, L, Kt = c.z0.to(dev), c.s, 3, 2

    def chain(z, state, noise_of, after=lambda: None):
        """init + 2 trajectories of 3 steps, prior-only, in place on z; returns the end calls' acceptance flags and log_alpha."""
        acc, la = [], []
        for j in range(Kt * L + 1):
            inner = j % L != 0
            _, a, l, _ = net.hmc_step(z, None, None, state, None if inner else noise_of(j // L), s,
                                      phase="inner" if inner else "end" if j else "init", propose=j < Kt * L, inplace=True)
            if not inner:
                acc.append(a.clone()); la.append(l.clone())
                after()
        return torch.stack(acc), torch.stack(la)

    z_e, st_e = z0.clone(), F.new_hmc_state(net._plan(), B, dev)
    acc_e, la_e = chain(z_e, st_e, lambda t: F.PhiloxNoise(21, 300 + t, 0))
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    z_g, st_g = z0.clone(), F.new_hmc_state(net._plan(), B, dev)
    rng = F.PhiloxNoise(21, 0, 0, offset_dev=ctr)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                            # warm-up off the capture stream
        chain(z_g, st_g, lambda t: rng, lambda: ctr.add_(1))
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc_g, la_g = chain(z_g, st_g, lambda t: rng, lambda: ctr.add_(1))
    z_g.copy_(z0); ctr.fill_(300)
    graph.replay()
    torch.cuda.synchronize()
    assert bits(acc_g, acc_e) and bits(la_g, la_e) and bits(z_g, z_e)
    assert all(bits(getattr(st_g, f), getattr(st_e, f)) for f in FIELDS)
    assert 0 < int(acc_e[1:].sum()) < Kt * B


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
    z0 = torch.randn(B, nz, 1, 1).to(dev)
    ph = F.PhiloxNoise(77, 1000, 0)
    kw = dict(leapfrog_steps=L, g_l_step_size=s, g_llhd_sigma=sigma)
    z_k, rate, u_k = Lv.sample_hmc_post_z_with_flow(z0, x, netG, net, g_l_steps=Ks, philox=ph, **kw)
    assert ph.offset == 1000 + Ks + 1 and z_k.shape == (B, nz, 1, 1) and rate.shape == (B,) and u_k.shape == (B,)
    # by hand: K L + 1 calls, the call that starts trajectory t + 1 at offset + t
    state, zp, flags = F.new_hmc_state(net._plan(), B, dev), z0.view(B, nz).clone(), []
    for j in range(Ks * L + 1):
        zr = zp.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = 1.0 / (2.0 * sigma * sigma) * ((netG(zr) - x) ** 2).flatten(1).sum(1)
        gg = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()
        inner = j % L != 0
        zp, acc, _, _ = net.hmc_step(zr.detach().view(B, nz), gg, energy.detach(), state, None if inner else F.PhiloxNoise(77, 1000 + j // L, 0), s,
                                     phase="inner" if inner else "end" if j else "init", propose=j < Ks * L)
        if j and not inner:
            flags.append(acc.clone())
    assert zp is None and len(flags) == Ks
    flags = torch.stack(flags)
    assert bits(z_k.view(B, nz), state.z) and bits(u_k, state.energy) and bits(rate, flags.sum(0) / Ks)
    assert 0.0 < rate.mean().item() < 1.0
    print(f"[hmc] sampler nz={nz} B={B} s={s} L={L}: mean acceptance {rate.mean().item():.2f}")
    # no trajectory, or no rows: the input
    ph = F.PhiloxNoise(77, 1000, 0)
    none = Lv.sample_hmc_post_z_with_flow(z0, x, netG, net, g_l_steps=0, philox=ph, **kw)
    assert torch.equal(none[0], z0) and none[1] is None and none[2] is None and ph.offset == 1000
    empty = Lv.sample_hmc_post_z_with_flow(z0[:0], x[:0], netG, net, g_l_steps=Ks, philox=ph, **kw)
    assert empty[0].shape == (0, nz, 1, 1) and ph.offset == 1000

"""GPU: the base-space Metropolis-adjusted Langevin step (lsnf_reverse_mala_step, lsnf_small3_rmala_kernel: the latency bf16x3
reverse-backward with the accept / reject tail as its output section), `flow.reverse_mala_step`, `_netF.reverse_mala_step` and
`langevin.sample_mala_post_eps_with_flow`.

Against float64 the chain is TEACHER-FORCED (the scheme of tests/test_gpu_mala.py): at each step the device is given the fp32 casts of
the float64 restatement's state (tests/rmala_restated.py), proposal, grad_g / energy_g (the closed-form quadratic of
tests/mala_restated.py, evaluated at the float64 x = f^-1(eps_prop)), noise and uniform, so a decision that differs on one row
cannot move the next step's inputs; the device runs its own reverse at the proposal for the stash.  Noise rows whose proposal would
put x within 2e-5 of a ReLU kink are redrawn on the CPU.  Per row, scale = |u_acc| + |U_prop| + (A + Bq) / (2 s^2) and
    gate = max(1e-5 * scale, 3 * |fp32 restatement - fp64 restatement|)
(the project's existing rule).  Rows whose float64 log_alpha is within the gate of ln u, and rows with oracle.relu_margin(p, x) <= 2e-5,
are set aside (at most 10 % of a case, 2 rows for B <= 33: asserted).  Accepted rows: eps_acc holds the bits of eps_prop; grad_acc is
held under the reverse-autograd gate max(1e-5 rel-L2, 3 x the oracle's own fp32-vs-fp64 error on that input); u_acc to
max(1e-5 (|e| + |eps|^2 / 2), 3 x the fp32 restatement's own error), and Case asserts that the fp32 restatement meets a third of the
first term on the inputs used.  Rejected rows keep their bits.  Everything else is bit identity between call forms."""
import functools

import numpy as np
import pytest
import torch

from oracle import flow_oracle as O
import chain_geometries as G
import mala_restated as M
import rmala_restated as RM
import trained_weights as T
import test_gpu_mala as ZM
import test_gpu_reverse_keep as K
from test_gpu_langevin import ToyG

pytestmark = pytest.mark.gpu

C3, C5, TINY = K.C3, K.C5, K.TINY
RUNS = [c + ("default",) for c in ZM.CASES] + [C3 + (100, "fp32")]            # (with the geometry classes of tests/chain_geometries.py)
PHILOX_CASES = [C3 + (33,), C3 + (4100,), C3 + (8200,), TINY + (33,)] + G.CASES   # the in-kernel draw against the tensor form
# Step size by nz, chosen on the CPU from the float64 restatement alone: tests/rmala_restated.py's 3-step chain of 33 rows (Case.rate)
# scanned over s = 0.3, 0.4, ... 2.1 and then in steps of 0.05 around the step at which about half of the decisions are accepted.  The
# z-space table of tests/test_gpu_mala.py does not carry over: there 0.9 serves nz 128, here 0.9 accepts nothing at nz >= 100 and the
# rate falls from 0.8 to 0.2 between s = 0.4 and 0.6 (N(0, I) in 128 dimensions times the quadratic likelihood pulled back through the
# flow), while nz 8 and 2 take larger steps than in z.  Rates found (B = 33): 0.48 / 0.47 / 0.70 / 0.66 / 0.51 / 0.58 / 0.47 in the
# table's order; C3 at B = 1: one of its three decisions accepted.
STEP = {128: 0.5, 100: 0.55, 126: 0.65, 64: 0.9, 20: 0.4, 8: 1.0, 2: 1.7}
# nz = 20 comes in two flows, and no one step serves both: depth 16 accepts 0.51 at s = 0.4 and 0.10 at 0.55, the additive depth-5
# flow still 0.90 at 0.5 and 0.82 at 0.7.  The additive geometry gets its own entry.
STEP_GEO = {(20, 12, 5, 0): 0.7}
# The geometries of tests/chain_geometries.py are keyed whole (nz 66 and 128 occur with two widths): Case.rate at 33 rows scanned over
# s = 0.30, 0.35, ... 1.50; the step whose rate is nearest one half (the smaller of two), no step setting aside more than its 2 rows.
# Rates found, in the table's order: 0.52 / 0.49 / 0.57 / 0.51 / 0.51 / 0.60 / 0.54 / 0.56 / 0.34 (at (128, 128) 0.65 still accepts
# 0.66; profiles/chain_geometries.txt).
STEP_GEO.update({(62, 31, 2, 1): 0.8, (66, 33, 2, 1): 0.8, (124, 63, 3, 1): 0.6, (66, 33, 3, 0): 0.85, (10, 40, 2, 1): 1.25, (70, 8, 2, 1): 0.85,
                 (12, 100, 2, 1): 1.1, (66, 65, 2, 1): 0.8, (128, 128, 2, 1): 0.7})


def step_of(nz, geo=None, weights=T.INIT):
    if weights != T.INIT:
        return float(np.float32(T.step_of("mala eps", geo)))                       # tests/trained_weights.py
    return float(np.float32(STEP_GEO[geo] if geo in STEP_GEO else STEP[nz]))      # the fp32 step the kernel sees


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


class Case:
    """One geometry and batch on the CPU: the float64 chain (teacher-forcing records) and the fp32 restatement's figures."""

    def __init__(self, nz, w, depth, coupling, B, s=None, weights=T.INIT):
        self.geo, self.B, self.nz, self.depth, self.weights = (nz, w, depth, coupling), B, nz, depth, weights
        p = T.params_for(O, self.geo, weights)
        self.p = K.additive(p) if coupling == 0 else p
        self.s = step_of(nz, (nz, w, depth, coupling), weights) if s is None else s
        self.n_steps = 3 if B <= 100 else 1
        self.quad = M.Quadratic(nz, 0.1, seed=7 + nz)                       # (U >= |eps|^2 / 2 is of order nz / 2: no row's bound falls below fp32)
        g = torch.Generator().manual_seed(7 + B)
        x0, _ = O.smooth_batch(self.p, B, nz, seed=1007 + B)                # (the chain's start is clear of a ReLU kink too)
        self.eps0 = K.R.forward64(self.p, x0)[0].float()
        self.noises = [torch.randn(B, nz, generator=g) for _ in range(self.n_steps + 1)]
        self.uniforms = [None] + [torch.rand(B, generator=g).clamp_min(2.0 ** -25) for _ in range(self.n_steps)]
        self.steps, _ = RM.chain(self.p, self.eps0, self.quad, self.s, self.noises, self.uniforms, redraw=g)
        for st in self.steps:
            U32, st.t32 = RM.potential32(self.p, st)
            st.la32 = RM.decide(st.e_acc.float(), st.t_acc.float(), st.u_acc.float(), st.e_prop.float(), st.t32, U32, st.u, self.s)[0]
            st.u_scale = st.e.abs() + 0.5 * (st.e_prop ** 2).sum(1)
            st.u_own = (U32.double() - st.U_prop).abs()
            assert bool((st.u_own <= 1e-5 * st.u_scale / 3.0)[st.acc].all()), "the u_acc bound is below fp32 on these inputs"
            st.margin = O.relu_margin(self.p, st.x.float())
            scale = st.u_acc.abs() + st.U_prop.abs() + (st.A + st.Bq) / (2.0 * self.s * self.s)
            st.gate = torch.maximum(1e-5 * scale, 3.0 * (st.la32.double() - st.la).abs())
            st.smooth = st.margin > 2e-5
            st.decided = st.smooth & ((st.la - torch.log(st.u.double())).abs() > st.gate)
        self.rate = torch.stack([st.acc for st in self.steps]).double().mean().item()


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


bits = ZM.bits


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


def run(lsnf, s, st, noise, uniform=None, rows=slice(None), how="auto", **kw):
    """The call of record st on its rows `rows`, from the float64 state's casts: (state after, the state before, outputs)."""
    cut = lambda t: t[rows].float().to(s.dev).contiguous()
    F = lsnf.flow
    state = F.MalaState(cut(st.e_acc), cut(st.t_acc), cut(st.u_acc))
    before = F.MalaState(state.z.clone(), state.grad.clone(), state.energy.clone())
    eps = cut(st.e_prop)
    saved, act = stash_at(lsnf, s.plan, eps, how)
    out = F.reverse_mala_step(s.plan, eps, saved, act, cut(st.ge), cut(st.e), state, noise, s.c.s, uniform=uniform, **kw)
    return state, before, out


def same(a, b):
    """Two (state, before, outputs) results hold the same bits."""
    (sa, _, oa), (sb, _, ob) = a, b
    return all(bits(x, y) for x, y in zip((sa.z, sa.grad, sa.energy) + tuple(oa), (sb.z, sb.grad, sb.energy) + tuple(ob)))


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


# ---------------------------------------------------------------------------------------------
# 1. against float64, teacher-forced
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B,mode", RUNS)
def test_decisions_and_state_follow_float64(lsnf, gpu_device, math, nz, w, depth, coupling, B, mode, weights=T.INIT):
    math(mode)
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, mode, weights)
    c = s.c
    mode = mode if weights == T.INIT else f"{mode} {weights}"
    print(f"[rmala] {mode} {c.geo} B{B} s={c.s:.3f}: float64 accepts {100 * c.rate:.0f} % of {len(c.steps)} x {B} decisions")
    if c.n_steps == 3:
        assert 0.15 <= c.rate <= 0.85
    for j, st in enumerate(c.steps):
        state, before, (e_next, acc, la) = run(lsnf, s, st, st.noise.to(s.dev), st.u.to(s.dev))
        torch.cuda.synchronize()
        aside = int((~st.decided).sum())
        allowed = 2 if B <= 33 else B // 10
        err = (la.cpu().double() - st.la).abs()
        worst = (err / st.gate)[st.smooth].max().item() if bool(st.smooth.any()) else 0.0
        print(f"[rmala] {mode} {c.geo} B{B} step {j + 1}: accepted {int(st.acc.sum())}/{B}, set aside {aside} (allowed {allowed}; "
              f"{int((~st.smooth).sum())} near a kink), worst |log_alpha - fp64| / gate = {worst:.3f}, "
              f"oracle-fp32 worst {((st.la32.double() - st.la).abs() / st.gate).max().item():.3f}")
        assert aside <= allowed
        if weights != T.INIT:                                # the same share from the device's own log_alpha, together with the kink rows
            aside_dev = int((~st.smooth | ((la.cpu().double() - torch.log(st.u.double())).abs() <= st.gate)).sum())
            print(f"[rmala] {mode} {c.geo} B{B} step {j + 1}: set aside by the device's log_alpha {aside_dev}")
            assert aside_dev <= allowed
        assert bool((err <= st.gate)[st.smooth].all())
        d, a64 = st.decided, st.acc
        acc_c, ea, ga, ua = acc.cpu(), state.z.cpu(), state.grad.cpu(), state.energy.cpu()
        assert bool(((acc_c == 1.0) | (acc_c == 0.0)).all()) and torch.equal(acc_c[d] == 1.0, a64[d])
        yes, no = d & a64, d & ~a64
        assert bits(ea[yes], st.e_prop.float()[yes])
        assert bits(ea[no], before.z.cpu()[no]) and bits(ga[no], before.grad.cpu()[no]) and bits(ua[no], before.energy.cpu()[no])
        if bool(yes.any()):
            u_bound = torch.maximum(1e-5 * st.u_scale, 3.0 * st.u_own)[yes]
            u_err = (ua[yes].double() - st.U_prop[yes]).abs()
            g_own = rel_l2(st.t32[yes], st.t_prop[yes])
            g_tol, g_err = max(1e-5, 3.0 * g_own), rel_l2(ga[yes], st.t_prop[yes])
            print(f"[rmala] {mode} {c.geo} B{B} step {j + 1}: worst u_acc error / bound = {(u_err / u_bound).max().item():.3f}, grad_acc "
                  f"rel-L2 measured {g_err:.3e} allowed {g_tol:.3e} oracle-fp32 {g_own:.3e}")
            assert bool((u_err <= u_bound).all())
            assert g_err <= g_tol
        n_err = rel_l2(e_next.cpu()[d], st.e_next[d]) if bool(d.any()) else 0.0
        assert n_err <= max(1e-5, 3.0 * rel_l2(st.t32, st.t_prop))


@pytest.mark.parametrize("nz,w,depth,coupling,B", T.CASES)
def test_decisions_and_state_follow_float64_at_trained_weights(lsnf, gpu_device, math, nz, w, depth, coupling, B):
    """The same steps, gates and caps on the golden trained weights (tests/trained_weights.py): a saturating sigmoid, |3 logs| up to 2,
    steps from the narrow window in which the float64 chain still accepts there."""
    test_decisions_and_state_follow_float64(lsnf, gpu_device, math, nz, w, depth, coupling, B, "default", weights=T.TRAINED)


# ---------------------------------------------------------------------------------------------
# 2. the INIT form: lsnf_reverse_langevin_step's proposal, the state written without being read
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (33,), C3 + (100,), C3 + (4100,), C3 + (8200,), TINY + (33,),
                                                   (126, 127, 2, 1, 33), (20, 12, 5, 0, 33)])
def test_init_form_is_the_plain_step(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c = lsnf.flow, gpu_device, s.c
    eps, noise = c.eps0.to(dev), c.noises[0].to(dev)
    e64, ge64 = c.quad(RM.reverse_of(c.p, c.eps0, torch.float64))
    e, ge = e64.float().to(dev), ge64.float().to(dev)
    saved, act = stash_at(lsnf, s.plan, eps)
    g = F.reverse_backward_z(s.plan, eps, saved, act, ge, None)
    for xi in (noise, F.PhiloxNoise(1234, 40, 3)):
        state = F.MalaState(*(torch.full_like(t, float("nan")) for t in (eps, eps, e)))          # never read
        e_next, acc, la = F.reverse_mala_step(s.plan, eps, saved, act, ge, e, state, xi, c.s, init=True)
        e_new = F.reverse_langevin_step(s.plan, eps, saved, act, ge, xi, c.s)[0]
        assert bits(e_next, e_new)
        assert bits(state.z, eps) and bits(state.grad, eps + g)                                  # one fp32 add on reverse_backward_z's g
        u_ref = e.double() + 0.5 * (eps.double() ** 2).sum(1)
        assert bool(((state.energy.double() - u_ref).abs() <= 1e-6 * (e.double().abs() + 0.5 * (eps.double() ** 2).sum(1))).all())
        assert bool((acc == 1.0).all()) and bits(la, torch.zeros_like(la))
    # no proposal asked for: the state alone
    state2 = F.new_mala_state(s.plan, B, dev)
    none = F.reverse_mala_step(s.plan, eps, saved, act, ge, e, state2, F.PhiloxNoise(1234, 40, 3), c.s, init=True, propose=False)
    assert none[0] is None and bits(state2.z, state.z) and bits(state2.grad, state.grad) and bits(state2.energy, state.energy)


# ---------------------------------------------------------------------------------------------
# 3. PhiloxNoise against the tensors of the same draws
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", PHILOX_CASES)
def test_philox_is_the_tensors_of_the_same_draws(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, st = lsnf.flow, gpu_device, s.c.steps[0]
    for row0 in (0, 2 ** 32 - 5):
        rng = F.PhiloxNoise(1234, 40, row0)
        xi = F.sample(s.plan, B, rng, want_eps=True)[2]
        u = torch.from_numpy(M.uniform_draws(B, 1234, 40, row0)).to(dev)
        got, ref = run(lsnf, s, st, rng), run(lsnf, s, st, xi, u)
        assert same(got, ref)
        assert 0 < int(got[2][1].sum()) < B or B < 8                    # both outcomes occur
    assert rng.offset == 40                                             # the call does not advance the generator
    ctr = torch.full((1,), 3, dtype=torch.int64, device=dev)
    a, b = run(lsnf, s, st, F.PhiloxNoise(1234, 37, 0, offset_dev=ctr)), run(lsnf, s, st, F.PhiloxNoise(1234, 40, 0))
    assert same(a, b) and not bits(a[2][0], run(lsnf, s, st, F.PhiloxNoise(1234, 37, 0))[2][0])
    with pytest.raises(lsnf.LsnfError):
        run(lsnf, s, st, rng, u)                                        # a generator and a tensor exclude each other
    with pytest.raises(lsnf.LsnfError):
        run(lsnf, s, st, xi)                                            # tensors: the uniform is required


# ---------------------------------------------------------------------------------------------
# 4. a row's result does not depend on the batch, the workgroup shape or the sharding
# ---------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch_or_the_sharding(lsnf, gpu_device):
    rows_are_their_own(lsnf, setup_of(lsnf, gpu_device, *C3, 8200), (slice(0, 8200), slice(0, 4100)))


@pytest.mark.parametrize("nz,w,depth,coupling,B", G.LARGE)      # 32 rows per workgroup at a ragged half, 64 at an empty half-tile
def test_rows_do_not_depend_on_the_workgroup_shape_at_a_ragged_half(lsnf, gpu_device, nz, w, depth, coupling, B):
    rows_are_their_own(lsnf, setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), [slice(0, n) for n in sorted({B, 4100})])


def rows_are_their_own(lsnf, s, larger):
    F, st = lsnf.flow, s.c.steps[0]
    rng = F.PhiloxNoise(99, 7, 0)
    flat = lambda r: (r[0].z, r[0].grad, r[0].energy) + tuple(r[2])
    part = run(lsnf, s, st, rng, rows=slice(0, 100))                    # 16 rows per workgroup
    for rows in larger:                                                 # 64 (ST = 4) and 32 (ST = 2) rows per workgroup
        for a, b in zip(flat(run(lsnf, s, st, rng, rows=rows)), flat(part)):
            assert bits(a[:100], b)
    lo = run(lsnf, s, st, F.PhiloxNoise(99, 7, 0), rows=slice(0, 40))
    hi = run(lsnf, s, st, F.PhiloxNoise(99, 7, 40), rows=slice(40, 100))
    for a, x, y in zip(flat(part), flat(lo), flat(hi)):
        assert bits(a, torch.cat([x, y]))
    wrong = run(lsnf, s, st, F.PhiloxNoise(99, 7, 0), rows=slice(40, 100))
    assert not bits(wrong[2][0], part[2][0][40:100])


# ---------------------------------------------------------------------------------------------
# 5. the two sources of the stash; in place; 4-byte offsets; NULL grad_g / energy_g
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (100,), TINY + (33,), C5 + (33,), (20, 12, 16, 1, 33)])
def test_stash_of_the_reverse_and_of_the_forward_decide_alike(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    st = s.c.steps[0]
    assert lsnf.flow.reverse_keep_supported(s.plan, B)
    kept = run(lsnf, s, st, st.noise.to(s.dev), st.u.to(s.dev), how="reverse")
    fwd = run(lsnf, s, st, st.noise.to(s.dev), st.u.to(s.dev), how="forward")
    d = st.decided
    assert torch.equal(kept[2][1].cpu()[d], fwd[2][1].cpu()[d]) and torch.equal(kept[2][1].cpu()[d] == 1.0, st.acc[d])
    assert bool(((kept[2][2].cpu().double() - fwd[2][2].cpu().double()).abs() <= 2.0 * st.gate)[st.smooth].all())


@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (33,), C3 + (4100,), C3 + (8200,), TINY + (33,), (126, 127, 2, 1, 33), (64, 32, 1, 1, 33)] + G.FORMS)
def test_next_proposal_over_the_proposal(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, st = lsnf.flow, gpu_device, s.c.steps[0]
    cast = lambda t: t.float().to(dev)
    for noise, u in ((st.noise.to(dev), st.u.to(dev)), (F.PhiloxNoise(5, 6, 7), None)):
        ref = run(lsnf, s, st, noise, u)
        state = F.MalaState(cast(st.e_acc), cast(st.t_acc), cast(st.u_acc))
        ep = cast(st.e_prop)
        saved, act = stash_at(lsnf, s.plan, ep)
        out = F.reverse_mala_step(s.plan, ep, saved, act, cast(st.ge), cast(st.e), state, noise, s.c.s, uniform=u, inplace=True)
        assert out[0].data_ptr() == ep.data_ptr() and same((state, None, out), ref)
    with pytest.raises(lsnf.LsnfError):                                 # no other output may be an input
        F.reverse_mala_step(s.plan, ep, saved, act, cast(st.ge), cast(st.e), F.MalaState(ep, state.grad, state.energy), noise, s.c.s)


@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (33,), C3 + (4100,), TINY + (33,)] + G.FORMS)
def test_every_tensor_four_bytes_off_a_16_byte_boundary(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, st = lsnf.flow, gpu_device, s.c.steps[0]

    def off4(t):
        t = t.float().to(dev)
        b = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
        v = b[1: 1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    ref = run(lsnf, s, st, st.noise.to(dev), st.u.to(dev))
    state = F.MalaState(off4(st.e_acc), off4(st.t_acc), off4(st.u_acc))
    ep = off4(st.e_prop)
    saved, act = stash_at(lsnf, s.plan, ep.contiguous())
    out = F.reverse_mala_step(s.plan, ep, None if saved is None else off4(saved), act, off4(st.ge), off4(st.e), state, off4(st.noise), s.c.s,
                              uniform=off4(st.u), inplace=True)
    assert same((state, None, out), ref)


@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (100,), TINY + (33,)] + G.FORMS)
def test_null_gradient_and_energy_are_zeros(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, st = lsnf.flow, gpu_device, s.c.steps[0]
    ep, rng = st.e_prop.float().to(dev), F.PhiloxNoise(8, 9, 0)
    saved, act = stash_at(lsnf, s.plan, ep)
    res = []
    for gg, e in ((None, None), (torch.zeros_like(ep), torch.zeros(B, device=dev))):
        for init in (True, False):
            state = F.MalaState(st.e_acc.float().to(dev), st.t_acc.float().to(dev), st.u_acc.float().to(dev))
            res.append((state, None, F.reverse_mala_step(s.plan, ep, saved, act, gg, e, state, rng, s.c.s, init=init)))
    assert same(res[0], res[2]) and same(res[1], res[3])
    assert bits(res[0][0].grad, ep)                                      # g = 0: grad U is eps itself


# ---------------------------------------------------------------------------------------------
# 6. the prior alone: the chain samples N(0, I) and every decision is the uniform's
# ---------------------------------------------------------------------------------------------
def test_prior_alone_decides_by_the_uniform(lsnf, gpu_device):
    nz, w, depth, coupling, B, Ks, seed, off = TINY + (4096, 3, 77, 500)
    dev, F = gpu_device, lsnf.flow
    p = O.init_params(nz, w, depth, seed=3)
    plan = lsnf.prepare(lsnf.params_from_state_dict(p, depth, dev), nz, w, depth, coupling)
    s = step_of(nz)
    eps = torch.randn(B, nz, generator=torch.Generator().manual_seed(5)).to(dev)
    state, seen = F.new_mala_state(plan, B, dev), 0
    for j in range(Ks + 1):
        saved, act = stash_at(lsnf, plan, eps)
        _, acc, la = F.reverse_mala_step(plan, eps, saved, act, None, None, state, F.PhiloxNoise(seed, off + j, 0), s, init=j == 0,
                                         propose=j < Ks, inplace=True)
        if j == 0:
            continue
        acc, la = acc.cpu(), la.cpu().double()
        lnu = torch.log(torch.from_numpy(M.uniform_draws(B, seed, off + j, 0)).double())
        assert bool(((acc == 0.0) | (acc == 1.0)).all())
        # the device compares in fp32 with its own logf: within 2 ulp of ln u, plus the rounding of the float64 value to fp32
        tol = 4.0 * 2.0 ** -24 * lnu.abs().clamp_min(1.0)
        assert bool((la[acc == 0.0] <= (lnu + tol)[acc == 0.0]).all()) and bool((la[acc == 1.0] >= (lnu - tol)[acc == 1.0]).all())
        seen += int(acc.sum())
    assert 0 < seen < Ks * B                                            # both outcomes occur
    assert bits(state.grad, state.z)                                    # the prior's gradient is eps itself
    assert bool(((state.energy.cpu().double() - 0.5 * (state.z.cpu().double() ** 2).sum(1)).abs() <= 1e-5 * (1.0 + state.energy.cpu().double())).all())


# ---------------------------------------------------------------------------------------------
# 7. the sampler
# ---------------------------------------------------------------------------------------------
def test_sampler_is_the_hand_written_loop(lsnf, gpu_device):
    nz, w, B, Ks, s, sigma = 20, 12, 33, 3, 0.9, 0.3
    p = O.init_params(nz, w, 5, seed=8)
    dev, F, L = gpu_device, lsnf.flow, lsnf.langevin
    net = K.module_of(lsnf, p, dev, False)
    torch.manual_seed(0)
    netG = ToyG(nz).to(dev)
    x = torch.tanh(torch.randn(B, 3, 4, 4)).to(dev)
    eps0 = torch.randn(B, nz, 1, 1).to(dev)
    ph = F.PhiloxNoise(77, 1000, 0)
    eps_k, z_k, rate, u_k = L.sample_mala_post_eps_with_flow(eps0, x, netG, net, g_l_steps=Ks, g_l_step_size=s, g_llhd_sigma=sigma, philox=ph)
    torch.cuda.synchronize()
    assert ph.offset == 1000 + Ks + 1 and eps_k.shape == (B, nz) and z_k.shape == (B, nz, 1, 1) and rate.shape == (B,) and u_k.shape == (B,)
    assert all(bool(torch.isfinite(t).all()) for t in (eps_k, z_k, rate, u_k))
    plan = net._plan()
    assert bits(z_k.view(B, nz), F.reverse(plan, eps_k, None)[0])
    # by hand: K + 1 calls, call j at offset + j
    state, ep, flags = F.new_mala_state(plan, B, dev), eps0.view(B, nz).clone(), []
    for j in range(Ks + 1):
        act = F.new_act_saved(plan, B, dev)
        z, _, saved = F.reverse(plan, ep, None, save_for_backward=True, act_saved=act)
        zr = z.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = 1.0 / (2.0 * sigma * sigma) * ((netG(zr) - x) ** 2).flatten(1).sum(1)
        gg = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()
        ep, acc, _ = F.reverse_mala_step(plan, ep, saved, act, gg, energy.detach(), state, F.PhiloxNoise(77, 1000 + j, 0), s, init=j == 0,
                                         propose=j < Ks)
        if j:
            flags.append(acc.clone())
    assert ep is None
    flags = torch.stack(flags)
    assert bits(eps_k, state.z) and bits(u_k, state.energy) and torch.equal(rate, flags.mean(0))
    print(f"[rmala] sampler nz={nz} B={B} s={s}: mean acceptance {rate.mean().item():.2f}")
    assert 0.0 < rate.mean().item() < 1.0
    # no step, or no rows: the input, without a launch
    ph = F.PhiloxNoise(77, 1000, 0)
    none = L.sample_mala_post_eps_with_flow(eps0, x, netG, net, g_l_steps=0, g_l_step_size=s, g_llhd_sigma=sigma, philox=ph)
    assert torch.equal(none[0], eps0.view(B, nz)) and none[2] is None and none[3] is None and ph.offset == 1000
    empty = L.sample_mala_post_eps_with_flow(eps0[:0], x[:0], netG, net, g_l_steps=Ks, g_l_step_size=s, g_llhd_sigma=sigma, philox=ph)
    assert empty[0].shape == (0, nz) and empty[2] is None and ph.offset == 1000

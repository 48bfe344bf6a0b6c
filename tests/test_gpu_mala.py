"""GPU: the Metropolis-adjusted Langevin step (lsnf_mala_step, lsnf_small3_mala_kernel: the latency bf16x3 backward with the accept /
reject tail as its output section), `flow.mala_step`, `_netF.mala_step` and `langevin.sample_mala_post_z_with_flow`.

Against float64 the chain is TEACHER-FORCED: at each step the device is given the fp32 casts of the float64 restatement's state,
proposal, grad_g / energy_g (the closed-form quadratic of tests/mala_restated.py), noise and uniform, so a decision that differs
on one row cannot move the next step's inputs.  Noise rows whose proposal would land within 2e-5 of a ReLU kink are redrawn on the
CPU (oracle.smooth_batch's rule, mala_restated.smooth_proposal), so the kink allowance below is rarely used.  Per row, scale = |u_acc| + |U_prop| + (A + Bq) / (2 s^2) and
    gate = max(1e-5 * scale, 3 * |fp32 restatement - fp64 restatement|)
(the project's log-prob / dz gate on the terms summed; the rule of tests/test_gpu_reverse_autograd.py, computed here on the CPU).
Rows whose float64 log_alpha is within the gate of ln u, and rows with oracle.relu_margin(p, z_prop) <= 2e-5, are set aside (at most
10 % of a case, 2 rows for B <= 33: asserted).  Step sizes are chosen so that the float64 chain accepts between 15 % and 85 % of its
decisions (asserted for the 3-step cases).  Everything else is bit identity between call forms.  The geometry classes of
tests/chain_geometries.py (ragged halves, whole tiles of padding) are appended to the case lists, under the same gates."""
import functools

import numpy as np
import pytest
import torch

from oracle import flow_oracle as O
import chain_geometries as G
import mala_restated as M
import trained_weights as T
import test_gpu_reverse_keep as K
from test_gpu_langevin import ToyG

pytestmark = pytest.mark.gpu

C3, C5, TINY = K.C3, K.C5, K.TINY
# (nz, width, depth, coupling, B).  C3: one row; a second 16-row tile; 33; 100; one step each at 4 100 (32 rows per workgroup, ragged),
# 8 200 (64 rows, ragged) and 16 400 (a second round of workgroups).  Then HT = 1, WT = 4, odd sizes, the smallest geometry, depth 1 and
# 16, additive.
CASES = [C3 + (B,) for B in (1, 17, 33, 100, 4100, 8200, 16400)] + \
        [TINY + (33,), C5 + (33,), (126, 127, 2, 1, 33), (2, 1, 3, 1, 33), (64, 32, 1, 1, 33), (20, 12, 16, 1, 33), (20, 12, 5, 0, 33)]
# ... and the geometry classes of tests/chain_geometries.py: every instantiation at a ragged half, with a whole tile of padding, with
# none; two of them at 32 and 64 rows per workgroup (single calls)
CASES += G.CASES + G.LARGE
RUNS = [c + ("default",) for c in CASES] + [C3 + (100, "fp32")]
PHILOX_CASES = [C3 + (33,), C3 + (4100,), C3 + (8200,), TINY + (33,)] + G.CASES          # the in-kernel draw against the tensor form
# step size by nz, chosen on the CPU from the float64 restatement alone (tests/mala_restated.py): between a quarter and three quarters
# of the decisions accepted (at the reference's 0.1 everything is accepted, which shows nothing)
STEP = {128: 0.9, 126: 0.85, 100: 0.9, 64: 1.0, 20: 1.1, 8: 1.2, 2: 0.5}
# The geometries of tests/chain_geometries.py are keyed whole (nz 66 and 128 occur with two widths), chosen the same way: the 3-step
# float64 chain of 33 rows (Case.rate) scanned over s = 0.30, 0.35, ... 1.50; the step whose rate is nearest one half (the smaller
# of two), no step setting aside more than its 2 rows.  Rates found, in the table's order: 0.48 / 0.58 / 0.56 / 0.53 / 0.49 / 0.44 /
# 0.49 / 0.46 / 0.44 (profiles/chain_geometries.txt).
STEP_GEO = {(62, 31, 2, 1): 1.0, (66, 33, 2, 1): 1.0, (124, 63, 3, 1): 0.85, (66, 33, 3, 0): 0.95, (10, 40, 2, 1): 1.2, (70, 8, 2, 1): 1.1,
            (12, 100, 2, 1): 1.15, (66, 65, 2, 1): 1.05, (128, 128, 2, 1): 0.85}


# scale of the quadratic's A = scale * randn.  u_acc is held to 1e-5 * (|e| + |ll|); at nz = 2 ll = -|z1|^2 / 2 + log 2 pi + logdet crosses
# zero on typical rows, and with e ~ 1e-2 (scale 0.1) that bound falls below fp32's resolution of ll's own terms: the float32 ORACLE
# misses it by 3.4x there.  So nz = 2 gets an energy of order 1; Case asserts that the float32 oracle is within a third of the bound
# on every accepted row, i.e. that the bound can be met in fp32 on the inputs used.
QUAD_SCALE = {2: 2.0}


def step_of(nz, geo=None, weights=T.INIT):
    if weights != T.INIT:
        return float(np.float32(T.step_of("mala z", geo)))                         # tests/trained_weights.py
    return float(np.float32(STEP_GEO[geo] if geo in STEP_GEO else STEP[nz]))      # the fp32 step the kernel sees


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


class Case:
    """One geometry and batch on the CPU: the float64 chain (teacher-forcing records) and the fp32 restatement's log_alpha."""

    def __init__(self, nz, w, depth, coupling, B, weights=T.INIT, s=None):
        self.geo, self.B, self.nz, self.depth, self.weights = (nz, w, depth, coupling), B, nz, depth, weights
        p = T.params_for(O, self.geo, weights)
        self.p = K.additive(p) if coupling == 0 else p
        self.s = step_of(nz, self.geo, weights) if s is None else float(np.float32(s))
        self.n_steps = 3 if B <= 100 else 1
        self.quad = M.Quadratic(nz, QUAD_SCALE.get(nz, 0.1), seed=7 + nz)
        g = torch.Generator().manual_seed(7 + B)
        self.z0, _ = O.smooth_batch(self.p, B, nz, seed=1007 + B)           # (the chain's start is clear of a ReLU kink too)
        self.noises = [torch.randn(B, nz, generator=g) for _ in range(self.n_steps + 1)]
        self.uniforms = [None] + [torch.rand(B, generator=g).clamp_min(2.0 ** -25) for _ in range(self.n_steps)]
        self.steps, _ = M.chain(self.p, self.z0, self.quad, self.s, self.noises, self.uniforms, redraw=g)
        for st in self.steps:
            st.la32 = M.log_alpha32(self.p, st, self.quad, self.s)
            ll32 = O.flow_log_prob(O.to_dtype(self.p, torch.float32), st.z_prop.float())[2].detach()
            own = ((st.e.float() - ll32).double() - st.U_prop).abs()
            assert bool((own <= 1e-5 * (st.e.abs() + st.ll.abs()) / 3.0)[st.acc].all()), "the u_acc bound is below fp32 on these inputs"
            st.margin = O.relu_margin(self.p, st.z_prop.float())
            scale = st.u_acc.abs() + st.U_prop.abs() + (st.A + st.Bq) / (2.0 * self.s * self.s)
            st.gate = torch.maximum(1e-5 * scale, 3.0 * (st.la32.double() - st.la).abs())
            st.smooth = st.margin > 2e-5
            st.decided = st.smooth & ((st.la - torch.log(st.u.double())).abs() > st.gate)
        self.rate = torch.stack([st.acc for st in self.steps]).double().mean().item()


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


def state_of(lsnf, dev, z, g, u):
    return lsnf.flow.MalaState(z.float().to(dev).contiguous(), g.float().to(dev).contiguous(), u.float().to(dev).contiguous())


def forced(lsnf, s, st, **kw):
    """One teacher-forced call of record st: (state after, the state's input casts, (z_next, accepted, log_alpha, ll))."""
    dev, c = s.dev, s.c
    state = state_of(lsnf, dev, st.z_acc, st.g_acc, st.u_acc)
    before = lsnf.flow.MalaState(state.z.clone(), state.grad.clone(), state.energy.clone())
    out = lsnf.flow.mala_step(s.plan, st.z_prop.float().to(dev), st.ge.float().to(dev), st.e.float().to(dev), state,
                              st.noise.to(dev), c.s, uniform=st.u.to(dev), **kw)
    return state, before, out


def rel_rows(got, ref):
    return (got.double() - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)


# ---------------------------------------------------------------------------------------------
# 1. against float64, teacher-forced
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B,mode", RUNS)
def test_decisions_and_state_follow_float64(lsnf, gpu_device, math, nz, w, depth, coupling, B, mode, weights=T.INIT):
    math(mode)
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, mode, weights)
    c = s.c
    mode = mode if weights == T.INIT else f"{mode} {weights}"
    print(f"[mala] {mode} {c.geo} B{B} s={c.s:.3f}: float64 accepts {100 * c.rate:.0f} % of {len(c.steps)} x {B} decisions")
    if c.n_steps == 3:
        assert 0.15 <= c.rate <= 0.85
    for j, st in enumerate(c.steps):
        state, before, (z_next, acc, la, ll) = forced(lsnf, s, st)
        torch.cuda.synchronize()
        aside = int((~st.decided).sum())
        allowed = 2 if B <= 33 else B // 10
        err = (la.cpu().double() - st.la).abs()
        worst = (err / st.gate)[st.smooth].max().item() if bool(st.smooth.any()) else 0.0
        print(f"[mala] {mode} {c.geo} B{B} step {j + 1}: accepted {int(st.acc.sum())}/{B}, set aside {aside} (allowed {allowed}; "
              f"{int((~st.smooth).sum())} near a kink), worst |log_alpha - fp64| / gate = {worst:.3f}, "
              f"oracle-fp32 worst {((st.la32.double() - st.la).abs() / st.gate).max().item():.3f}")
        assert aside <= allowed
        if weights != T.INIT:                                # the same share from the device's own log_alpha, together with the kink rows
            aside_dev = int((~st.smooth | ((la.cpu().double() - torch.log(st.u.double())).abs() <= st.gate)).sum())
            print(f"[mala] {mode} {c.geo} B{B} step {j + 1}: set aside by the device's log_alpha {aside_dev}")
            assert aside_dev <= allowed
        assert bool((err <= st.gate)[st.smooth].all())
        d, a64 = st.decided, st.acc
        acc_c, za, ga, ua = acc.cpu(), state.z.cpu(), state.grad.cpu(), state.energy.cpu()
        assert bool(((acc_c == 1.0) | (acc_c == 0.0)).all()) and torch.equal(acc_c[d] == 1.0, a64[d])
        yes, no = d & a64, d & ~a64
        fig = lambda t: t.max().item() if t.numel() else 0.0
        print(f"[mala] {mode} {c.geo} B{B} step {j + 1}: worst u_acc error / (1e-5 (|e| + |ll|)) = "
              f"{fig((ua[yes].double() - st.U_prop[yes]).abs() / (1e-5 * (st.e[yes].abs() + st.ll[yes].abs()))):.3f}, grad_acc rel-L2 "
              f"{fig(rel_rows(ga[yes], st.g_prop[yes])):.2e}, z_next rel-L2 {fig(rel_rows(z_next.cpu()[d], st.z_next[d])):.2e} (allowed 1e-5)")
        assert bits(za[yes], st.z_prop.float()[yes])
        assert bool(((ua[yes].double() - st.U_prop[yes]).abs() <= 1e-5 * (st.e[yes].abs() + st.ll[yes].abs())).all())
        assert bool((rel_rows(ga[yes], st.g_prop[yes]) <= 1e-5).all())
        assert bits(za[no], before.z.cpu()[no]) and bits(ga[no], before.grad.cpu()[no]) and bits(ua[no], before.energy.cpu()[no])
        assert bool((rel_rows(z_next.cpu()[d], st.z_next[d]) <= 1e-5).all())


@pytest.mark.parametrize("nz,w,depth,coupling,B", T.CASES)
def test_decisions_and_state_follow_float64_at_trained_weights(lsnf, gpu_device, math, nz, w, depth, coupling, B):
    """The same steps, gates and caps on the golden trained weights (tests/trained_weights.py): a saturating sigmoid, |3 logs| up to 2,
    |grad log p| of order 1e3, steps from the narrow window in which the float64 chain still accepts there."""
    test_decisions_and_state_follow_float64(lsnf, gpu_device, math, nz, w, depth, coupling, B, "default", weights=T.TRAINED)


# ---------------------------------------------------------------------------------------------
# 2. the INIT form: lsnf_langevin_step's proposal, the state written without being read
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (33,), C3 + (100,), C3 + (4100,), C3 + (8200,), TINY + (33,),
                                                   (126, 127, 2, 1, 33), (20, 12, 5, 0, 33)])
def test_init_form_is_the_plain_step(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c = lsnf.flow, gpu_device, s.c
    z, noise = c.z0.to(dev), c.noises[0].to(dev)
    e64, ge64 = c.quad(c.z0.double())
    e, ge = e64.float().to(dev), ge64.float().to(dev)
    for xi in (noise, F.PhiloxNoise(1234, 40, 3)):
        state = F.MalaState(*(torch.full_like(t, float("nan")) for t in (z, z, e)))          # never read
        z_next, acc, la, ll = F.mala_step(s.plan, z, ge, e, state, xi, c.s, init=True)
        z_new, ll_ref, _, _ = F.langevin_step(s.plan, z, ge, xi, c.s)
        assert bits(z_next, z_new) and bits(ll, ll_ref)
        act = F.new_act_saved(s.plan, B, dev)
        z1, _, _, saved = F.forward(s.plan, z, None, save_for_backward=True, act_saved=act)
        assert bits(state.grad, ge + F.backward_z(s.plan, z1, saved, ll_scale=-1.0, act_saved=act))
        assert bits(state.z, z) and bits(state.energy, e - ll)
        assert bool((acc == 1.0).all()) and bits(la, torch.zeros_like(la))
    # no proposal asked for: the state alone
    state2 = F.new_mala_state(s.plan, B, dev)
    none = F.mala_step(s.plan, z, ge, e, state2, F.PhiloxNoise(1234, 40, 3), c.s, init=True, propose=False)
    assert none[0] is None and bits(state2.z, state.z) and bits(state2.grad, state.grad) and bits(state2.energy, state.energy)


# ---------------------------------------------------------------------------------------------
# 3. PhiloxNoise against the tensors of the same draws
# ---------------------------------------------------------------------------------------------
def same(a, b):
    """Two (state, outputs) results hold the same bits."""
    (sa, oa), (sb, ob) = a, b
    return all(bits(x, y) for x, y in zip((sa.z, sa.grad, sa.energy) + tuple(oa), (sb.z, sb.grad, sb.energy) + tuple(ob)))


def run(lsnf, s, st, noise, uniform=None, rows=slice(None), **kw):
    """The call of record st on its rows `rows`, from the float64 state's casts: (state after, outputs)."""
    dev, cut = s.dev, (lambda t: t[rows].float().to(s.dev).contiguous())
    state = lsnf.flow.MalaState(cut(st.z_acc), cut(st.g_acc), cut(st.u_acc))
    out = lsnf.flow.mala_step(s.plan, cut(st.z_prop), cut(st.ge), cut(st.e), state, noise, s.c.s, uniform=uniform, **kw)
    return state, out


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
        assert 0 < int(got[1][1].sum()) < B or B < 8                    # both outcomes occur
    assert rng.offset == 40                                             # the call does not advance the generator
    ctr = torch.full((1,), 3, dtype=torch.int64, device=dev)
    a, b = run(lsnf, s, st, F.PhiloxNoise(1234, 37, 0, offset_dev=ctr)), run(lsnf, s, st, F.PhiloxNoise(1234, 40, 0))
    assert same(a, b) and not bits(a[1][0], run(lsnf, s, st, F.PhiloxNoise(1234, 37, 0))[1][0])
    with pytest.raises(lsnf.LsnfError):
        run(lsnf, s, st, rng, u)                                        # a generator and a tensor exclude each other
    with pytest.raises(lsnf.LsnfError):
        run(lsnf, s, st, xi)                                            # tensors: the uniform is required


# ---------------------------------------------------------------------------------------------
# 4. a row's result does not depend on the batch, the workgroup shape or the sharding
# ---------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch_or_the_sharding(lsnf, gpu_device):
    rows_are_their_own(lsnf, setup_of(lsnf, gpu_device, *C3, 8200))                # 64 rows per workgroup


@pytest.mark.parametrize("nz,w,depth,coupling,B", G.LARGE)      # 32 rows per workgroup at a ragged half, 64 at an empty half-tile
def test_rows_do_not_depend_on_the_workgroup_shape_at_a_ragged_half(lsnf, gpu_device, nz, w, depth, coupling, B):
    rows_are_their_own(lsnf, setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


def rows_are_their_own(lsnf, s):
    F, st = lsnf.flow, s.c.steps[0]
    rng = F.PhiloxNoise(99, 7, 0)
    whole = run(lsnf, s, st, rng)
    part = run(lsnf, s, st, rng, rows=slice(0, 100))        # 16 rows per workgroup
    flat = lambda r: (r[0].z, r[0].grad, r[0].energy) + tuple(r[1])
    for a, b in zip(flat(whole), flat(part)):
        assert bits(a[:100], b)
    lo = run(lsnf, s, st, F.PhiloxNoise(99, 7, 0), rows=slice(0, 40))
    hi = run(lsnf, s, st, F.PhiloxNoise(99, 7, 40), rows=slice(40, 100))
    for a, x, y in zip(flat(part), flat(lo), flat(hi)):
        assert bits(a, torch.cat([x, y]))
    wrong = run(lsnf, s, st, F.PhiloxNoise(99, 7, 0), rows=slice(40, 100))
    assert not bits(wrong[1][0], part[1][0][40:100])


# ---------------------------------------------------------------------------------------------
# 5. in place, 4-byte offsets, NULL grad_g / energy_g
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (33,), C3 + (4100,), C3 + (8200,), TINY + (33,), (126, 127, 2, 1, 33), (64, 32, 1, 1, 33)] + G.FORMS)
def test_next_proposal_over_the_proposal(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, st = lsnf.flow, gpu_device, s.c.steps[0]
    for noise, u in ((st.noise.to(dev), st.u.to(dev)), (F.PhiloxNoise(5, 6, 7), None)):
        ref = run(lsnf, s, st, noise, u)
        state = state_of(lsnf, dev, st.z_acc, st.g_acc, st.u_acc)
        zp = st.z_prop.float().to(dev)
        out = F.mala_step(s.plan, zp, st.ge.float().to(dev), st.e.float().to(dev), state, noise, s.c.s, uniform=u, inplace=True)
        assert out[0].data_ptr() == zp.data_ptr() and same((state, out), ref)
    with pytest.raises(lsnf.LsnfError):                                 # no other output may be an input
        F.mala_step(s.plan, zp, st.ge.float().to(dev), st.e.float().to(dev), F.MalaState(zp, state.grad, state.energy), noise, s.c.s)


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
    state = F.MalaState(off4(st.z_acc), off4(st.g_acc), off4(st.u_acc))
    out = F.mala_step(s.plan, off4(st.z_prop), off4(st.ge), off4(st.e), state, off4(st.noise), s.c.s, uniform=off4(st.u), inplace=True)
    assert same((state, out), ref)


@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (100,), TINY + (33,)] + G.FORMS)
def test_null_gradient_and_energy_are_zeros(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, st = lsnf.flow, gpu_device, s.c.steps[0]
    zp, rng = st.z_prop.float().to(dev), F.PhiloxNoise(8, 9, 0)
    res = []
    for gg, e in ((None, None), (torch.zeros_like(zp), torch.zeros(B, device=dev))):
        for init in (True, False):
            state = state_of(lsnf, dev, st.z_acc, st.g_acc, st.u_acc)
            res.append((state, F.mala_step(s.plan, zp, gg, e, state, rng, s.c.s, init=init)))
    assert same(res[0], res[2]) and same(res[1], res[3])


# ---------------------------------------------------------------------------------------------
# 6. antisymmetry: log_alpha(z -> z') + log_alpha(z' -> z) = 0, no oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (100,), TINY + (33,), C5 + (33,)])
def test_log_alpha_is_antisymmetric(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F, dev, c, st = lsnf.flow, gpu_device, s.c, s.c.steps[0]
    pts = [st.z_acc.float().to(dev), st.z_prop.float().to(dev)]
    pot = [tuple(t.float().to(dev) for t in c.quad(z.cpu().double())) for z in pts]         # (energy, gradient) of the quadratic
    u, la = torch.full((B,), 0.5, device=dev), []
    for a, b in ((0, 1), (1, 0)):
        state = F.new_mala_state(s.plan, B, dev)
        F.mala_step(s.plan, pts[a], pot[a][1], pot[a][0], state, None, c.s, init=True, propose=False)
        la.append(F.mala_step(s.plan, pts[b], pot[b][1], pot[b][0], state, None, c.s, uniform=u, propose=False)[2].cpu().double())
    # the reverse move's terms are the forward move's with u_acc / U_prop and A / Bq exchanged: the same scale, so its gate is at least
    # 1e-5 * scale -- the sum of the two rows' gates is at least the bound used here.  Both points are clear of a ReLU kink (Case).
    scale = st.u_acc.abs() + st.U_prop.abs() + (st.A + st.Bq) / (2.0 * c.s * c.s)
    gate = st.gate + 1e-5 * scale
    assert bool(st.smooth.all()) and bool((O.relu_margin(c.p, st.z_acc.float()) > 2e-5).all())
    worst = ((la[0] + la[1]).abs() / gate).max().item()
    print(f"[mala] {c.geo} B{B} antisymmetry: worst |sum| / (two gates) = {worst:.3e}, largest |log_alpha| {la[0].abs().max().item():.2f}")
    assert la[0].abs().max().item() > 1.0 and bool(((la[0] + la[1]).abs() <= gate).all())


# ---------------------------------------------------------------------------------------------
# 7. a non-finite row is rejected and touches nothing else
# ---------------------------------------------------------------------------------------------
def test_a_nan_row_is_rejected_and_alone(lsnf, gpu_device):
    s = setup_of(lsnf, gpu_device, *C3, 33)
    F, dev, st = lsnf.flow, gpu_device, s.c.steps[0]
    rng, bad = F.PhiloxNoise(3, 4, 0), 18
    clean = run(lsnf, s, st, rng)
    state = state_of(lsnf, dev, st.z_acc, st.g_acc, st.u_acc)
    before = [t.clone() for t in (state.z, state.grad, state.energy)]
    zp = st.z_prop.float().to(dev)
    zp[bad, 5] = float("nan")
    z_next, acc, la, ll = F.mala_step(s.plan, zp, st.ge.float().to(dev), st.e.float().to(dev), state, rng, s.c.s)
    assert acc[bad].item() == 0.0 and bool(torch.isnan(la[bad]))
    for got, was in zip((state.z, state.grad, state.energy), before):
        assert bits(got[bad], was[bad])
    keep = torch.arange(33, device=dev) != bad
    for got, ref in zip((state.z, state.grad, state.energy, z_next, acc, la, ll), (clean[0].z, clean[0].grad, clean[0].energy) + tuple(clean[1])):
        assert bits(got[keep], ref[keep])


# ---------------------------------------------------------------------------------------------
# 8. a chain captured in a graph
# ---------------------------------------------------------------------------------------------
def test_graphed_chain_is_the_eager_chain(lsnf, gpu_device):
    nz, w, depth, coupling, B = C3 + (100,)
    c = case(nz, w, depth, coupling, B)
    dev, F = gpu_device, lsnf.flow
    net = K.module_of(lsnf, c.p, dev, False)
    z0, s = c.z0.to(dev), c.s

    def chain(z, state, noise_of, after=lambda: None):
        """init + 3 deciding calls, prior-only, in place on z; returns the per-call acceptance flags and log_alpha."""
        acc, la = [], []
        for j in range(4):
            _, a, l, _ = net.mala_step(z, None, None, state, noise_of(j), s, init=j == 0, propose=j < 3, inplace=True)
            acc.append(a.clone()); la.append(l.clone())
            after()
        return torch.stack(acc), torch.stack(la)

    z_e, st_e = z0.clone(), F.new_mala_state(net._plan(), B, dev)
    acc_e, la_e = chain(z_e, st_e, lambda j: F.PhiloxNoise(21, 300 + j, 0))
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    z_g, st_g = z0.clone(), F.new_mala_state(net._plan(), B, dev)
    rng = F.PhiloxNoise(21, 0, 0, offset_dev=ctr)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                            # warm-up off the capture stream
        chain(z_g, st_g, lambda j: rng, lambda: ctr.add_(1))
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc_g, la_g = chain(z_g, st_g, lambda j: rng, lambda: ctr.add_(1))
    z_g.copy_(z0); ctr.fill_(300)
    graph.replay()
    torch.cuda.synchronize()
    assert bits(acc_g, acc_e) and bits(la_g, la_e) and bits(z_g, z_e)
    assert bits(st_g.z, st_e.z) and bits(st_g.grad, st_e.grad) and bits(st_g.energy, st_e.energy)
    assert 0 < int(acc_e[1:].sum()) < 3 * B


# ---------------------------------------------------------------------------------------------
# 9. the sampler
# ---------------------------------------------------------------------------------------------
def test_sampler_is_the_hand_written_loop(lsnf, gpu_device):
    nz, w, B, Ks, s, sigma = 20, 12, 37, 4, 0.6, 0.3
    p = O.init_params(nz, w, 5, seed=8)
    dev, F, L = gpu_device, lsnf.flow, lsnf.langevin
    net = K.module_of(lsnf, p, dev, False)
    torch.manual_seed(0)
    netG = ToyG(nz).to(dev)
    x = torch.tanh(torch.randn(B, 3, 4, 4)).to(dev)
    z0 = torch.randn(B, nz, 1, 1).to(dev)
    ph = F.PhiloxNoise(77, 1000, 0)
    z_k, rate, u_k = L.sample_mala_post_z_with_flow(z0, x, netG, net, g_l_steps=Ks, g_l_step_size=s, g_llhd_sigma=sigma, philox=ph)
    assert ph.offset == 1000 + Ks + 1 and z_k.shape == (B, nz, 1, 1) and rate.shape == (B,) and u_k.shape == (B,)
    # by hand: K + 1 calls, call j at offset + j
    state, zp, flags = F.new_mala_state(net._plan(), B, dev), z0.view(B, nz).clone(), []
    for j in range(Ks + 1):
        zr = zp.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = 1.0 / (2.0 * sigma * sigma) * ((netG(zr) - x) ** 2).flatten(1).sum(1)
        gg = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()
        zp, acc, _, _ = net.mala_step(zr.detach().view(B, nz), gg, energy.detach(), state, F.PhiloxNoise(77, 1000 + j, 0), s, init=j == 0,
                                      propose=j < Ks)
        if j:
            flags.append(acc.clone())
    assert zp is None
    flags = torch.stack(flags)
    assert bits(z_k.view(B, nz), state.z) and bits(u_k, state.energy) and bits(rate, flags.sum(0) / Ks)
    assert torch.equal(rate, flags.mean(0)) and 0.0 < rate.mean().item() < 1.0
    print(f"[mala] sampler nz={nz} B={B} s={s}: mean acceptance {rate.mean().item():.2f}")
    # no step, or no rows: the input
    ph = F.PhiloxNoise(77, 1000, 0)
    none = L.sample_mala_post_z_with_flow(z0, x, netG, net, g_l_steps=0, g_l_step_size=s, g_llhd_sigma=sigma, philox=ph)
    assert torch.equal(none[0], z0) and none[1] is None and none[2] is None and ph.offset == 1000
    empty = L.sample_mala_post_z_with_flow(z0[:0], x[:0], netG, net, g_l_steps=Ks, g_l_step_size=s, g_llhd_sigma=sigma, philox=ph)
    assert empty[0].shape == (0, nz, 1, 1) and ph.offset == 1000

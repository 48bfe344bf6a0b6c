"""GPU: the fused base-space Langevin step (lsnf_reverse_langevin_step, the UPDATE form of lsnf_small3_rbwd_kernel), the fused
eps-space sampler and its graphed form.

Inputs as tests/test_gpu_reverse_keep.py builds them: eps = f_fp64(oracle.smooth_batch(...)), the stash from flow.forward at
x = reverse(eps) (so the kernel's `eps` is that forward's own output z1).  The gradient is held to the bits of
flow.reverse_backward_z (which tests/test_gpu_reverse_autograd.py holds to float64); the update to the worst case of its four
roundings; everything else is bit identity between call forms.  The sampler is held to the float64 oracle trajectory."""
import functools

import numpy as np
import pytest
import torch

from oracle.philox_oracle import langevin_noise
import chain_geometries as G
import reverse_restated as R
import trained_weights as T
import test_gpu_reverse_keep as K

pytestmark = pytest.mark.gpu

C3, C5, TINY, C1 = K.C3, K.C5, K.TINY, K.C1
# (nz, width, depth, coupling, B).  C3: one row; a second 16-row tile; 33; 100; 4 100 (32 rows per workgroup, ragged); 8 200 (64 rows,
# ragged); 16 400 (a second round of workgroups).  Then HT = 1, WT = 4, odd sizes, the smallest geometry, depth 1 and 16, additive.
CASES = [C3 + (B,) for B in (1, 17, 33, 100, 4100, 8200, 16400)] + \
        [TINY + (33,), C5 + (33,), (126, 127, 2, 1, 33), (2, 1, 3, 1, 33), (64, 32, 1, 1, 33), (20, 12, 16, 1, 33), (20, 12, 5, 0, 33)]
CASES += G.CASES + G.LARGE                                 # the geometry classes of tests/chain_geometries.py
PHILOX_CASES = [C3 + (33,), C3 + (4100,), C3 + (8200,), TINY + (33,)] + G.CASES         # the in-kernel draw against the tensor form
RUNS = [c + ("default",) for c in CASES] + [C3 + (100, "fp32")]
STEP = float(np.float32(0.1))                              # the fp32 step the kernel sees


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


class Setup:
    """One case on the device: the plan, x = reverse(eps), the forward's outputs and stash at x, the upstream gradient, a noise tensor,
    and the results of the plain calls the tests compare with -- each computed once."""

    def __init__(self, lsnf, dev, nz, w, depth, coupling, B, mode, weights=T.INIT):
        F = lsnf.flow
        self.c = c = K.case(nz, w, depth, coupling, B, weights)
        self.geo, self.B, self.nz, self.depth, self.mode = c.geo, B, nz, depth, mode
        # the fp32 step the kernel sees: 0.1, or the trained geometry's own (tests/trained_weights.py)
        self.step_size = step = STEP if weights == T.INIT else float(np.float32(T.LANGEVIN_STEP[c.geo]))
        prev = F.set_math_mode(F.MATH_FP32) if mode == "fp32" else None
        try:
            self.plan = K.make_plan(lsnf, c, dev)
            self.x = F.reverse(self.plan, c.eps.to(dev), None)[0]
            self.act = F.new_act_saved(self.plan, B, dev)
            self.e, _, _, self.saved = F.forward(self.plan, self.x, None, want_ll=False, save_for_backward=True, act_saved=self.act)
            self.gx = c.gx.to(dev)
            self.noise = torch.randn(B, nz, generator=torch.Generator().manual_seed(7 + B)).to(dev)
            self.g_ref = F.reverse_backward_z(self.plan, self.e, self.saved, self.act, self.gx, None)
            self.plain = F.reverse_langevin_step(self.plan, self.e, self.saved, self.act, self.gx, None, step, want_g=True)
            self.noisy = F.reverse_langevin_step(self.plan, self.e, self.saved, self.act, self.gx, self.noise, step, want_g=True)
            torch.cuda.synchronize()
        finally:
            if prev is not None:
                F.set_math_mode(prev)

    def step(self, lsnf, noise, **kw):
        return lsnf.flow.reverse_langevin_step(self.plan, self.e, self.saved, self.act, self.gx, noise, self.step_size, **kw)


@functools.lru_cache(maxsize=None)
def _setup(lsnf, dev, nz, w, depth, coupling, B, mode, weights):
    return Setup(lsnf, dev, nz, w, depth, coupling, B, mode, weights)


def setup_of(lsnf, dev, nz, w, depth, coupling, B, mode="default", weights=T.INIT):
    return _setup(lsnf, dev, nz, w, depth, coupling, B, mode, weights)


@pytest.fixture
def math(request, lsnf):
    """The math mode of a run while its test calls the library (the setup's own calls set it themselves)."""
    def enter(mode):
        if mode == "fp32":
            F = lsnf.flow
            prev = F.set_math_mode(F.MATH_FP32)
            request.addfinalizer(lambda: F.set_math_mode(prev))
    return enter


def bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------
# 1. the gradient is lsnf_reverse_backward_z's, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B,mode", RUNS)
def test_gradient_bits(lsnf, gpu_device, math, nz, w, depth, coupling, B, mode, weights=T.INIT):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, mode, weights)
    math(mode)
    F, STEP = lsnf.flow, s.step_size
    assert bool(torch.isfinite(s.g_ref).all())
    assert bits(s.plain[1], s.g_ref) and bits(s.noisy[1], s.g_ref)
    # grad_g = None is explicit zeros
    zeros = torch.zeros_like(s.gx)
    a = F.reverse_langevin_step(s.plan, s.e, s.saved, s.act, None, s.noise, STEP, want_g=True)
    b = F.reverse_langevin_step(s.plan, s.e, s.saved, s.act, zeros, s.noise, STEP, want_g=True)
    assert bits(a[0], b[0]) and bits(a[1], b[1])
    assert bits(a[1], F.reverse_backward_z(s.plan, s.e, s.saved, s.act, zeros, None))


# ---------------------------------------------------------------------------------------------
# 2. the update: four fp32 roundings (and coef's own), fused or not
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B,mode", RUNS)
def test_update_arithmetic(lsnf, gpu_device, nz, w, depth, coupling, B, mode, weights=T.INIT):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, mode, weights)
    STEP = s.step_size
    e, coef = s.e.double(), 0.5 * STEP * STEP
    for what, res, n in (("no noise", s.plain, torch.zeros_like(e)), ("tensor noise", s.noisy, s.noise.double())):
        g = res[1].double()                                 # the kernel's own g
        r = e - coef * (e + g) + STEP * n
        bound = 2.0 ** -23 * (e.abs() + 3.0 * coef * (e + g).abs() + 2.0 * STEP * n.abs())
        excess = ((res[0].double() - r).abs() - bound).max().item()
        worst = ((res[0].double() - r).abs() / bound.clamp_min(1e-300)).max().item()
        print(f"[reverse-langevin] {mode} {s.geo} B{B}{'' if weights == T.INIT else ' ' + weights} {what}: worst |eps_new - r| / bound = {worst:.3f}")
        assert bool(torch.isfinite(res[0]).all()) and excess <= 0.0
    assert not bits(s.plain[0], s.noisy[0]) or B * nz < 4


# ---------------------------------------------------------------------------------------------
# 3. Philox: the in-kernel draw is lsnf_sample's eps at temperature 1, through the same instructions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", PHILOX_CASES)
def test_philox_is_the_tensor_of_the_same_draw(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F = lsnf.flow
    for row0 in (0, 2 ** 32 - 5):
        rng = F.PhiloxNoise(1234, 40, row0)
        draw = F.sample(s.plan, B, rng, want_eps=True)[2]
        got = s.step(lsnf, rng, want_g=True)
        ref = s.step(lsnf, draw, want_g=True)
        assert bits(got[0], ref[0]) and bits(got[1], ref[1]) and bits(got[2], ref[2]) and bits(got[3], ref[3])
        assert not bits(got[0], s.plain[0])
    assert rng.offset == 40                                 # the call does not advance the generator
    # a device counter is added to the offset
    ctr = torch.full((1,), 3, dtype=torch.int64, device=gpu_device)
    a = s.step(lsnf, F.PhiloxNoise(1234, 37, 0, offset_dev=ctr))
    b = s.step(lsnf, F.PhiloxNoise(1234, 40, 0))
    assert bits(a[0], b[0]) and not bits(a[0], s.step(lsnf, F.PhiloxNoise(1234, 37, 0))[0])
    with pytest.raises(lsnf.LsnfError):
        s.step(lsnf, F.PhiloxNoise(1234, 37, 0, offset_dev=ctr.cpu()))


def shard(lsnf, s, lo, hi):
    """Rows [lo, hi) of a setup as a batch of their own: sliced tensors, the stash from the forward at the sliced x (a stash is
    tiled by the batch it was written for).  The forward's rows do not depend on the batch: checked, the rest relies on it."""
    F = lsnf.flow
    x = s.x[lo:hi].contiguous()
    act = F.new_act_saved(s.plan, hi - lo, x.device)
    e, _, _, saved = F.forward(s.plan, x, None, want_ll=False, save_for_backward=True, act_saved=act)
    assert bits(e, s.e[lo:hi]) and (saved is None or bits(saved, s.saved[:, lo:hi]))
    return e, saved, act, s.gx[lo:hi].contiguous()


def test_row_sharding_with_row0(lsnf, gpu_device):
    s = setup_of(lsnf, gpu_device, *C3, 100)
    F = lsnf.flow
    whole = s.step(lsnf, F.PhiloxNoise(1234, 40, 0), want_g=True)
    e, saved, act, gx = shard(lsnf, s, 40, 100)
    part = F.reverse_langevin_step(s.plan, e, saved, act, gx, F.PhiloxNoise(1234, 40, 40), STEP, want_g=True)
    for a, b in zip(whole, part):
        assert bits(a[40:100], b)
    wrong = F.reverse_langevin_step(s.plan, e, saved, act, gx, F.PhiloxNoise(1234, 40, 0), STEP)
    assert not bits(whole[0][40:100], wrong[0])


# ---------------------------------------------------------------------------------------------
# 4. a row's result does not depend on the batch size or the workgroup shape
# ---------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_workgroup_shape(lsnf, gpu_device):
    rows_are_their_own(lsnf, setup_of(lsnf, gpu_device, *C3, 8200), (100, 4100))         # 64 rows per workgroup against 16 and 32


@pytest.mark.parametrize("nz,w,depth,coupling,B", G.LARGE)      # 32 rows per workgroup at a ragged half, 64 at an empty half-tile
def test_rows_do_not_depend_on_the_workgroup_shape_at_a_ragged_half(lsnf, gpu_device, nz, w, depth, coupling, B):
    rows_are_their_own(lsnf, setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), [n for n in (100, 4100) if n < B])


def rows_are_their_own(lsnf, s, smaller):
    F = lsnf.flow
    rng = F.PhiloxNoise(99, 7, 0)
    whole = s.step(lsnf, rng, want_g=True)
    for n in smaller:
        e, saved, act, gx = shard(lsnf, s, 0, n)
        part = F.reverse_langevin_step(s.plan, e, saved, act, gx, rng, STEP, want_g=True)
        for a, b in zip(whole, part):
            assert bits(a[:n], b)
        noise = s.noise[:n].contiguous()
        assert bits(s.noisy[0][:n], F.reverse_langevin_step(s.plan, e, saved, act, gx, noise, STEP)[0])


# ---------------------------------------------------------------------------------------------
# 5. norms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B,mode", RUNS)
def test_norms(lsnf, gpu_device, math, nz, w, depth, coupling, B, mode, weights=T.INIT):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, mode, weights)
    math(mode)
    eps_new, g, g_norm, eps_norm = s.noisy
    assert g_norm.shape == (B,) and eps_norm.shape == (B,)
    rel = (nz + 4) * 2.0 ** -24
    for what, got, of in (("g_norm", g_norm, g), ("eps_norm", eps_norm, s.e)):
        ref = of.double().norm(dim=1)
        err = ((got.double() - ref).abs() / ref.clamp_min(1e-300)).max().item()
        print(f"[reverse-langevin] {mode} {s.geo} B{B}{'' if weights == T.INIT else ' ' + weights} {what}: rel {err:.3e} allowed {rel:.3e}")
        assert err <= rel
    bare = s.step(lsnf, s.noise, want_norms=False, want_g=False)
    assert bare[1] is None and bare[2] is None and bare[3] is None and bits(bare[0], eps_new)
    only_g = s.step(lsnf, s.noise, want_norms=False, want_g=True)
    assert only_g[2] is None and bits(only_g[0], eps_new) and bits(only_g[1], g)


# ---------------------------------------------------------------------------------------------
# 5b. the three checks above on the golden trained weights (tests/trained_weights.py), each geometry at its own step
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", T.CASES)
def test_gradient_bits_at_trained_weights(lsnf, gpu_device, math, nz, w, depth, coupling, B):
    test_gradient_bits(lsnf, gpu_device, math, nz, w, depth, coupling, B, "default", weights=T.TRAINED)


@pytest.mark.parametrize("nz,w,depth,coupling,B", T.CASES)
def test_update_arithmetic_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    test_update_arithmetic(lsnf, gpu_device, nz, w, depth, coupling, B, "default", weights=T.TRAINED)


@pytest.mark.parametrize("nz,w,depth,coupling,B", T.CASES)
def test_norms_at_trained_weights(lsnf, gpu_device, math, nz, w, depth, coupling, B):
    test_norms(lsnf, gpu_device, math, nz, w, depth, coupling, B, "default", weights=T.TRAINED)


# ---------------------------------------------------------------------------------------------
# 6. in place, the scalar path, g_eps over grad_g
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (33,), C3 + (4100,), C3 + (8200,), TINY + (33,), (126, 127, 2, 1, 33), (64, 32, 1, 1, 33)] + G.FORMS)
def test_in_place_and_aliases(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    F = lsnf.flow
    for noise, ref in ((s.noise, s.noisy), (None, s.plain)):
        e = s.e.clone()
        saved0, act0 = (None if s.saved is None else s.saved.clone()), s.act.clone()
        got = F.reverse_langevin_step(s.plan, e, s.saved, s.act, s.gx, noise, STEP, inplace=True, want_g=True)
        assert got[0].data_ptr() == e.data_ptr()
        for a, b in zip(got, ref):
            assert bits(a, b)
        assert bits(s.act, act0) and (saved0 is None or bits(s.saved, saved0))
    rng = F.PhiloxNoise(5, 6, 7)
    e = s.e.clone()
    F.reverse_langevin_step(s.plan, e, s.saved, s.act, s.gx, rng, STEP, inplace=True)
    assert bits(e, s.step(lsnf, rng)[0])
    # g_eps written over grad_g
    gx = s.gx.clone()
    got = F.reverse_langevin_step(s.plan, s.e, s.saved, s.act, gx, s.noise, STEP, out=(None, gx, None, None))
    assert got[1].data_ptr() == gx.data_ptr() and bits(gx, s.g_ref) and bits(got[0], s.noisy[0])
    with pytest.raises(lsnf.LsnfError):
        F.reverse_langevin_step(s.plan, s.e, s.saved, s.act, s.gx, s.noise, STEP, out=(s.gx, None, None, None))
    with pytest.raises(lsnf.LsnfError):
        F.reverse_langevin_step(s.plan, s.e, s.saved, s.act, s.gx, s.noise, STEP, inplace=True, out=(torch.empty_like(s.e), None, None, None))


@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (33,), C3 + (4100,), TINY + (33,)] + G.FORMS)
def test_every_tensor_four_bytes_off_a_16_byte_boundary(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    dev, F = gpu_device, lsnf.flow

    def off4(t):
        b = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
        assert b.data_ptr() % 16 == 0
        v = b[1: 1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    out = tuple(off4(torch.zeros_like(t)) for t in s.noisy)
    got = F.reverse_langevin_step(s.plan, off4(s.e), off4(s.saved), s.act, off4(s.gx), off4(s.noise), STEP, out=out)
    for a, b in zip(got, s.noisy):
        assert bits(a, b)
    e4 = off4(s.e)
    F.reverse_langevin_step(s.plan, e4, off4(s.saved), s.act, off4(s.gx), F.PhiloxNoise(5, 6, 7), STEP, inplace=True)
    assert bits(e4, s.step(lsnf, F.PhiloxNoise(5, 6, 7))[0])
    with pytest.raises(lsnf.LsnfError):
        F.reverse_langevin_step(s.plan, s.e, s.saved, off4(s.act), s.gx, None, STEP)      # the stash must be 16-byte aligned


# ---------------------------------------------------------------------------------------------
# 7. the fused sampler
# ---------------------------------------------------------------------------------------------
STEPS, STEP_SIZE, SIGMA = K.STEPS, K.STEP_SIZE, K.SIGMA


@pytest.mark.parametrize("nz,w,depth,coupling,B", [TINY + (33,), C1 + (100,)])
def test_fused_sampler_follows_the_float64_trajectory(lsnf, gpu_device, monkeypatch, nz, w, depth, coupling, B):
    p, start, target, e64, z64, e32, z32 = K.trajectory_case(nz, w, depth, coupling, B)
    dev, F, L = gpu_device, lsnf.flow, lsnf.langevin
    net = K.module_of(lsnf, p, dev, False)
    netG = K.TanhGenerator(nz, torch.float32).to_device(dev)
    fwd = K.count_forward(lsnf, monkeypatch)
    draws = []
    real_sample = F.sample
    monkeypatch.setattr(F, "sample", lambda *a, **k: (draws.append(1), real_sample(*a, **k))[1])
    kw = dict(g_l_steps=STEPS, g_l_step_size=STEP_SIZE, g_llhd_sigma=SIGMA, fused=True)
    eps0, tgt = start.to(dev), target.to(dev)
    e, z, gg, gf = L.sample_langevin_post_eps_with_flow(eps0.view(B, nz, 1, 1), tgt, netG, net, noise=False, **kw)
    assert not fwd and torch.equal(eps0, start.to(dev))                       # the reverse kept the stash; the input is not written
    assert e.shape == (B, nz) and z.shape == (B, nz, 1, 1) and gg.dim() == 0 and gf.dim() == 0
    assert torch.equal(z.view(B, nz), F.reverse(net._plan(), e, None)[0])
    for what, got, r64, r32 in (("eps", e, e64, e32), ("z", z.view(B, nz), z64, z32)):
        own = R.rel_l2(r32, r64)
        err = R.rel_l2(got.cpu(), r64)
        print(f"[reverse-langevin] fused sampler {(nz, w, depth, coupling)} B{B} {what} after {STEPS} steps: "
              f"measured {err:.3e} allowed {max(2e-5, 3.0 * own):.3e} oracle-fp32 {own:.3e}")
        assert err <= max(2e-5, 3.0 * own)
    # where the keep form is not supported the three-launch form runs: the same trajectory
    prev = F.set_small_batch_max(16)
    try:
        e3, _, _, _ = L.sample_langevin_post_eps_with_flow(eps0, tgt, netG, net, noise=False, **kw)
    finally:
        F.set_small_batch_max(prev)
    assert len(fwd) == STEPS
    assert R.rel_l2(e3.cpu(), e64) <= max(2e-5, 3.0 * R.rel_l2(e32, e64))
    # an empty batch and no step, as the unfused sampler
    e0, z0, gg0, gf0 = L.sample_langevin_post_eps_with_flow(eps0[:0], tgt[:0], netG, net, **kw)
    assert e0.shape == (0, nz) and z0.shape == (0, nz, 1, 1) and gg0 is None and gf0 is None
    en, _, ggn, gfn = L.sample_langevin_post_eps_with_flow(eps0, tgt, netG, net, **dict(kw, g_l_steps=0))
    assert torch.equal(en, eps0) and ggn is None and gfn is None
    # philox noise: drawn in the update kernel at offset + k -- no sampling launch; the generator advances by the step count
    assert not draws
    ph = F.PhiloxNoise(1234, 40, 0)
    L.sample_langevin_post_eps_with_flow(eps0, tgt, netG, net, philox=ph, **kw)
    assert not draws and ph.offset == 40 + STEPS
    ph = F.PhiloxNoise(1234, 40, 0)
    one = dict(kw, g_l_steps=1)
    e_noise, _, gg1, gf1 = L.sample_langevin_post_eps_with_flow(eps0, tgt, netG, net, philox=ph, **one)
    e_plain, _, gg2, gf2 = L.sample_langevin_post_eps_with_flow(eps0, tgt, netG, net, noise=False, **one)
    assert not draws and ph.offset == 41 and torch.equal(gg1, gg2) and torch.equal(gf1, gf2)
    draw = (e_noise - e_plain) / STEP_SIZE
    ref = torch.from_numpy(langevin_noise(B, nz, 1234, 40, 0)).to(dev)
    # (v_log_f32 / v_sin_f32 / v_cos_f32 against float64 libm and the subtraction above: the bound tests/test_gpu_langevin.py holds)
    assert (draw.double() - ref).abs().max().item() <= 1e-4
    # the norms are the means of the per-row norms at the last step's input
    assert abs(gf2.item() - eps0.norm(dim=1).mean().item()) <= 1e-5 * gf2.item()
    # the unfused default is still what it was: it draws with a sampling launch of its own
    L.sample_langevin_post_eps_with_flow(eps0, tgt, netG, net, philox=F.PhiloxNoise(1234, 40, 0), **dict(one, fused=False))
    assert len(draws) == 1


# ---------------------------------------------------------------------------------------------
# 8. one step captured in a graph
# ---------------------------------------------------------------------------------------------
def test_graphed_sampler_is_the_eager_fused_sampler(lsnf, gpu_device):
    nz, w, depth, coupling, B = C1 + (100,)
    p, start, target, *_ = K.trajectory_case(nz, w, depth, coupling, B)
    dev, F, L = gpu_device, lsnf.flow, lsnf.langevin
    net = K.module_of(lsnf, p, dev, False)
    netG = K.TanhGenerator(nz, torch.float32).to_device(dev)
    eps0, tgt = start.to(dev), target.to(dev)
    sampler = L.GraphedEpsLangevinSampler(netG, net, B, nz, tgt.shape, g_l_step_size=STEP_SIZE, g_llhd_sigma=SIGMA, seed=11)
    kw = dict(g_l_steps=STEPS, g_l_step_size=STEP_SIZE, g_llhd_sigma=SIGMA, fused=True)
    for offset, e_in in ((40, eps0), (1000, 0.5 * eps0)):   # a second run from a new offset and a new start
        got = sampler.run(e_in, tgt, STEPS, offset=offset)
        torch.cuda.synchronize()
        ref = L.sample_langevin_post_eps_with_flow(e_in, tgt, netG, net, philox=F.PhiloxNoise(11, offset, 0), **kw)
        assert got[0].shape == (B, nz) and got[1].shape == (B, nz, 1, 1)
        for a, b in zip(got, ref):
            assert bits(a.reshape(-1), b.reshape(-1))
    none = sampler.run(eps0, tgt, 0)
    assert torch.equal(none[0], eps0) and none[2] is None and none[3] is None


def test_graphed_sampler_needs_the_stash_keeping_reverse(lsnf, gpu_device):
    nz, w, depth, coupling, B = TINY + (33,)
    c = K.case(nz, w, depth, coupling, B)
    dev, F = gpu_device, lsnf.flow
    net = K.module_of(lsnf, c.p, dev, False)
    netG = K.TanhGenerator(nz, torch.float32).to_device(dev)
    prev = F.set_small_batch_max(16)
    try:
        with pytest.raises(lsnf.LsnfError):
            lsnf.langevin.GraphedEpsLangevinSampler(netG, net, B, nz, (B, 16), g_l_step_size=STEP_SIZE, g_llhd_sigma=SIGMA)
    finally:
        F.set_small_batch_max(prev)


# ---------------------------------------------------------------------------------------------
# 9. flow.reverse(z_saved_out=): the caller-owned block-output buffer the graphed sampler uses
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (33,), (64, 32, 1, 1, 33)])
def test_reverse_writes_the_block_outputs_into_the_caller_s_buffer(lsnf, gpu_device, nz, w, depth, coupling, B):
    s = setup_of(lsnf, gpu_device, nz, w, depth, coupling, B)
    dev, F = gpu_device, lsnf.flow
    eps = s.c.eps.to(dev)
    act0, act1 = F.new_act_saved(s.plan, B, dev), F.new_act_saved(s.plan, B, dev)
    act0.fill_(float("nan")); act1.fill_(float("nan"))           # (the stash has words no row owns: compared as they were left)
    x0, o0, saved0 = F.reverse(s.plan, eps, None, save_for_backward=True, act_saved=act0)
    buf = torch.full((max(depth - 1, 1), B, nz), float("nan"), device=dev)
    x1, o1, saved1 = F.reverse(s.plan, eps, None, act_saved=act1, z_saved_out=buf)         # (implies save_for_backward)
    assert bits(x1, x0) and bits(o1, o0) and bits(act1, act0)
    if depth > 1:
        assert saved1 is buf and bits(buf, saved0)
        with pytest.raises(lsnf.LsnfError):
            F.reverse(s.plan, eps, None, act_saved=act1, z_saved_out=buf.flatten()[:-1])   # one element short
        with pytest.raises(lsnf.LsnfError):
            F.reverse(s.plan, eps, None, act_saved=act1, z_saved_out=buf.cpu())
        with pytest.raises(lsnf.LsnfError):
            F.reverse(s.plan, eps, None, act_saved=act1, z_saved_out=buf.double())
    else:
        assert saved0 is None and saved1 is None and bool(torch.isnan(buf).all())           # depth 1 has no block outputs to keep
    # without the keyword the call is what it was
    assert len(F.reverse(s.plan, eps, None)) == 2

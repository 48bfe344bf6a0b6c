"""GPU: per-row step sizes and their on-device dual-averaging adaptation for Hamiltonian Monte Carlo in the flow's base space
(lsnf_reverse_hmc_step_rows, lsnf_small3_rhmcr_kernel), `flow.reverse_hmc_step_rows`, `_netF.reverse_hmc_step_rows` and
`langevin.sample_hmc_adaptive_post_eps_with_flow`.  The checks are tests/hmc_rows_gpu.py's, shared with tests/test_gpu_hmc_rows.py
(whose docstring lists them); the cases, their teacher-forcing records and their steps are tests/test_gpu_rhmc.py's."""
import pytest
import torch

import hmc_rows_gpu as HG
import hmc_rows_restated as R
import test_gpu_rhmc as TR
import test_gpu_reverse_keep as K
from test_gpu_langevin import ToyG
import trained_weights as TW

pytestmark = pytest.mark.gpu
SP = HG.Space("eps", TR)
bits = HG.bits


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


@pytest.mark.parametrize("nz,w,depth,coupling,B", HG.IDENTITY)
def test_per_row_is_the_scalar_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B):
    HG.check_per_row_is_the_scalar_call(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", HG.ARITHMETIC)
def test_adaptation_arithmetic(lsnf, gpu_device, nz, w, depth, coupling, B):
    HG.check_adaptation_arithmetic(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


def test_rows_do_not_depend_on_the_batch_or_the_sharding(lsnf, gpu_device):
    HG.check_rows_do_not_depend_on_the_batch(lsnf, SP, TR.setup_of(lsnf, gpu_device, *HG.C3, 8200))


def test_a_nan_row_shrinks_its_own_step_and_is_alone(lsnf, gpu_device):
    HG.check_a_nan_row(lsnf, SP, TR.setup_of(lsnf, gpu_device, *HG.C3, 33))


def test_graphed_warm_up_is_the_eager_warm_up(lsnf, gpu_device):
    """The stash-keeping reverse and `reverse_hmc_step_rows` in place on static buffers, prior-only: the whole warm-up chain (init, three
    adapting trajectories of two steps: "update", "update", "last") captured in ONE graph, the draws from a device-side counter."""
    nz, w, depth, coupling, B = HG.C3 + (100,)
    c = TR.case(nz, w, depth, coupling, B)
    dev, F = gpu_device, lsnf.flow
    net = K.module_of(lsnf, c.p, dev, False)
    plan = net._plan()
    assert F.reverse_keep_supported(plan, B)
    eps0, L, Kt = c.eps0.to(dev), 2, 3
    modes = {1: "update", 2: "update", 3: "last"}
    f32 = dict(dtype=torch.float32, device=dev)

    class Buffers:
        def __init__(self):
            self.eps, self.z, self.obj = eps0.clone(), torch.zeros(B, nz, **f32), torch.zeros(B, **f32)
            self.saved, self.act = torch.zeros(depth - 1, B, nz, **f32), F.new_act_saved(plan, B, dev)
            self.state, self.steps = F.new_hmc_state(plan, B, dev), HG.three_steps(lsnf, c, B, dev)[1]

    def chain(b, noise_of, after=lambda: None):
        acc, la = [], []
        with torch.no_grad():
            for j in range(Kt * L + 1):
                inner, t = j % L != 0, j // L
                F.reverse(plan, b.eps, None, out=(b.z, b.obj), act_saved=b.act, z_saved_out=b.saved)
                _, a, l = F.reverse_hmc_step_rows(plan, b.eps, b.saved, b.act, None, None, b.state, None if inner else noise_of(t), b.steps,
                                                  phase="inner" if inner else "end" if j else "init", propose=j < Kt * L, inplace=True,
                                                  adapt=None if inner or not j else modes[t])
                if not inner:
                    acc.append(a.clone()); la.append(l.clone())
                    after()
        return torch.stack(acc), torch.stack(la)

    be = Buffers()
    acc_e, la_e = chain(be, lambda t: F.PhiloxNoise(21, 300 + t, 0))
    bg = Buffers()
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    rng = F.PhiloxNoise(21, 0, 0, offset_dev=ctr)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                            # warm-up off the capture stream
        chain(bg, lambda t: rng, lambda: ctr.add_(1))
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc_g, la_g = chain(bg, lambda t: rng, lambda: ctr.add_(1))
    start = HG.three_steps(lsnf, c, B, dev)[1]
    bg.eps.copy_(eps0); ctr.fill_(300); bg.steps.step.copy_(start.step); bg.steps.adapt.copy_(start.adapt)
    graph.replay()
    torch.cuda.synchronize()
    assert bits(acc_g, acc_e) and bits(la_g, la_e) and bits(bg.eps, be.eps)
    assert all(bits(getattr(bg.state, f), getattr(be.state, f)) for f in HG.FIELDS)
    assert bits(bg.steps.step, be.steps.step) and bits(bg.steps.adapt, be.steps.adapt)
    assert bool((be.steps.adapt[:, 2] == Kt).all()) and not bits(be.steps.step, start.step) and 0 < int(acc_e[1:].sum()) < Kt * B


def test_sampler_without_warm_up_is_the_existing_sampler(lsnf, gpu_device):
    nz, w, B, Ks, L, s, sigma = 20, 12, 37, 3, 2, 0.6, 0.3
    from oracle import flow_oracle as O
    p = O.init_params(nz, w, 5, seed=8)
    dev, F, Lv = gpu_device, lsnf.flow, lsnf.langevin
    net = K.module_of(lsnf, p, dev, False)
    plan = net._plan()
    torch.manual_seed(0)
    netG = ToyG(nz).to(dev)
    x = torch.tanh(torch.randn(B, 3, 4, 4)).to(dev)
    eps0 = torch.randn(B, nz, 1, 1).to(dev)
    kw = dict(g_l_steps=Ks, leapfrog_steps=L, g_l_step_size=s, g_llhd_sigma=sigma)
    ph1, ph2 = F.PhiloxNoise(77, 1000, 0), F.PhiloxNoise(77, 1000, 0)
    e_a, z_a, rate_a, u_a = (t.clone() for t in Lv.sample_hmc_post_eps_with_flow(eps0, x, netG, net, philox=ph1, **kw))
    e_b, z_b, rate_b, u_b, steps = Lv.sample_hmc_adaptive_post_eps_with_flow(eps0, x, netG, net, warmup_steps=0, philox=ph2, **kw)
    assert bits(e_a, e_b) and bits(z_a, z_b) and bits(rate_a, rate_b) and bits(u_a, u_b) and ph1.offset == ph2.offset == 1000 + Ks + 1
    assert isinstance(steps, F.HmcRowSteps) and bool((steps.step == torch.tensor(s).float().item()).all()) and bool((steps.adapt[:, 2] == 0).all())
    assert 0.0 < rate_b.mean().item() < 1.0
    # with warm-up: the hand-written loop of the per-row calls (end calls 1, 2 adapt, the second with "last"; 3, 4 run frozen)
    Ks, W = 4, 2
    kw.update(g_l_steps=Ks)
    ph = F.PhiloxNoise(78, 50, 0)
    first = torch.linspace(0.3, 0.9, B).to(dev)
    e_k, z_k, rate, u_k, steps = Lv.sample_hmc_adaptive_post_eps_with_flow(eps0, x, netG, net, warmup_steps=W, philox=ph, **dict(kw, g_l_step_size=first))
    assert ph.offset == 50 + Ks + 1 and bits(z_k.view(B, nz), F.reverse(plan, e_k, None)[0])
    mine, state, ep, flags = F.new_hmc_row_steps(B, dev, first), F.new_hmc_state(plan, B, dev), eps0.view(B, nz).clone(), []
    for j in range(Ks * L + 1):
        act = F.new_act_saved(plan, B, dev)
        z, _, saved = F.reverse(plan, ep, None, save_for_backward=True, act_saved=act)
        zr = z.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = 1.0 / (2.0 * sigma * sigma) * ((netG(zr) - x) ** 2).flatten(1).sum(1)
        gg = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()
        inner, t = j % L != 0, j // L
        ep, acc, _ = F.reverse_hmc_step_rows(plan, ep, saved, act, gg, energy.detach(), state, None if inner else F.PhiloxNoise(78, 50 + t, 0), mine,
                                             phase="inner" if inner else "end" if j else "init", propose=j < Ks * L,
                                             adapt=None if inner or not j or t > W else "last" if t == W else "update")
        if j and not inner and t > W:
            flags.append(acc.clone())
    assert ep is None and len(flags) == Ks - W
    assert bits(e_k, state.z) and bits(u_k, state.energy) and bits(rate, torch.stack(flags).sum(0) / (Ks - W))
    assert bits(steps.step, mine.step) and bits(steps.adapt, mine.adapt) and bool((steps.adapt[:, 2] == W).all()) and not bits(steps.step, first)


def test_sampler_frozen_phase_acceptance_lies_in_the_cpu_band(lsnf, gpu_device):
    dev, F, Lv = gpu_device, lsnf.flow, lsnf.langevin
    net, netG, x, eps0, first = HG.warmup_problem(lsnf, K, dev, "eps")
    e_k, z_k, rate, u_k, steps = Lv.sample_hmc_adaptive_post_eps_with_flow(eps0, x, netG, net, g_l_steps=R.WARMUP_K + R.FROZEN_K,
                                                                           leapfrog_steps=R.WARMUP_L, warmup_steps=R.WARMUP_K, g_l_step_size=first,
                                                                           g_llhd_sigma=1.0, philox=F.PhiloxNoise(5, 0, 0))
    torch.cuda.synchronize()
    HG.check_frozen_phase_acceptance(SP, rate.cpu(), steps)


# ---------------------------------------------------------------------------------------------
# The golden trained weights (tests/trained_weights.py, TW): the checks above on the scalar module's trained cases, each at its own step.
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_per_row_is_the_scalar_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    HG.check_per_row_is_the_scalar_call(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_adaptation_arithmetic_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    HG.check_adaptation_arithmetic(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))

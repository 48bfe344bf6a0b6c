"""GPU: per-row step sizes and their on-device dual-averaging adaptation for Hamiltonian Monte Carlo in z (lsnf_hmc_step_rows,
lsnf_small3_hmcr_kernel), `flow.hmc_step_rows`, `_netF.hmc_step_rows` and `langevin.sample_hmc_adaptive_post_z_with_flow`.  The checks
are tests/hmc_rows_gpu.py's, shared with tests/test_gpu_rhmc_rows.py; the cases, their teacher-forcing records and their steps are
tests/test_gpu_hmc.py's.

1. without adaptation a row is the scalar call at its step, bit for bit, in every phase, with noise tensors and with Philox;
2. an adapting end call decides as the plain one and then updates: adapt and step against the float64 update of the device's own
   log_alpha within 1e-5 (1 + |mu| + (sqrt(t) / gamma) |hbar|) (widened to 3 x the fp32 restatement's own error where that exceeds
   a third of it, test_gpu_hmc.widened), the next point and momentum the fp32 restatement's bits at the device's new step;
3. rows do not depend on B, the workgroup shape or the row0 sharding, with adaptation on;
4. a NaN row counts as a rejection, shrinks its own step and leaves every other row's bits alone; pinned rows stay finite;
5. a warm-up chain replayed from one captured graph is the eager chain, the step and adapt arrays included;
6. the sampler: warmup_steps = 0 is the existing sampler, with warm-up it is the hand-written loop, and its frozen-phase acceptance
   lies in the band tests/test_hmc_rows_cpu.py established for the same configuration."""
import pytest
import torch

import hmc_rows_gpu as HG
import hmc_rows_restated as R
import test_gpu_hmc as TH
import test_gpu_reverse_keep as K
from test_gpu_langevin import ToyG
import trained_weights as TW

pytestmark = pytest.mark.gpu
SP = HG.Space("z", TH)
bits = HG.bits


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


@pytest.mark.parametrize("nz,w,depth,coupling,B", HG.IDENTITY)
def test_per_row_is_the_scalar_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B):
    HG.check_per_row_is_the_scalar_call(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", HG.ARITHMETIC)
def test_adaptation_arithmetic(lsnf, gpu_device, nz, w, depth, coupling, B):
    HG.check_adaptation_arithmetic(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


def test_rows_do_not_depend_on_the_batch_or_the_sharding(lsnf, gpu_device):
    HG.check_rows_do_not_depend_on_the_batch(lsnf, SP, TH.setup_of(lsnf, gpu_device, *HG.C3, 8200))


def test_a_nan_row_shrinks_its_own_step_and_is_alone(lsnf, gpu_device):
    HG.check_a_nan_row(lsnf, SP, TH.setup_of(lsnf, gpu_device, *HG.C3, 33))


def test_graphed_warm_up_is_the_eager_warm_up(lsnf, gpu_device):
    nz, w, depth, coupling, B = HG.C3 + (100,)
    c = TH.case(nz, w, depth, coupling, B)
    dev, F = gpu_device, lsnf.flow
    net = K.module_of(lsnf, c.p, dev, False)
    z0, L, Kt = c.z0.to(dev), 2, 3
    modes = {1: "update", 2: "update", 3: "last"}

    def chain(z, state, steps, noise_of, after=lambda: None):
        """init + 3 adapting trajectories of 2 steps, prior-only, in place on z; returns the end calls' acceptance flags and log_alpha."""
        acc, la = [], []
        for j in range(Kt * L + 1):
            inner, t = j % L != 0, j // L
            _, a, l, _ = net.hmc_step_rows(z, None, None, state, None if inner else noise_of(t), steps,
                                           phase="inner" if inner else "end" if j else "init", propose=j < Kt * L, inplace=True,
                                           adapt=None if inner or not j else modes[t])
            if not inner:
                acc.append(a.clone()); la.append(l.clone())
                after()
        return torch.stack(acc), torch.stack(la)

    fresh = lambda: HG.three_steps(lsnf, c, B, dev)[1]
    z_e, st_e, steps_e = z0.clone(), F.new_hmc_state(net._plan(), B, dev), fresh()
    acc_e, la_e = chain(z_e, st_e, steps_e, lambda t: F.PhiloxNoise(21, 300 + t, 0))
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    z_g, st_g, steps_g = z0.clone(), F.new_hmc_state(net._plan(), B, dev), fresh()
    rng = F.PhiloxNoise(21, 0, 0, offset_dev=ctr)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                            # warm-up off the capture stream
        chain(z_g, st_g, steps_g, lambda t: rng, lambda: ctr.add_(1))
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc_g, la_g = chain(z_g, st_g, steps_g, lambda t: rng, lambda: ctr.add_(1))
    start = fresh()
    z_g.copy_(z0); ctr.fill_(300); steps_g.step.copy_(start.step); steps_g.adapt.copy_(start.adapt)
    graph.replay()
    torch.cuda.synchronize()
    assert bits(acc_g, acc_e) and bits(la_g, la_e) and bits(z_g, z_e)
    assert all(bits(getattr(st_g, f), getattr(st_e, f)) for f in HG.FIELDS)
    assert bits(steps_g.step, steps_e.step) and bits(steps_g.adapt, steps_e.adapt)
    assert bool((steps_e.adapt[:, 2] == Kt).all()) and not bits(steps_e.step, start.step) and 0 < int(acc_e[1:].sum()) < Kt * B


def test_sampler_without_warm_up_is_the_existing_sampler(lsnf, gpu_device):
    nz, w, B, Ks, L, s, sigma = 20, 12, 37, 3, 2, 0.6, 0.3
    from oracle import flow_oracle as O
    p = O.init_params(nz, w, 5, seed=8)
    dev, F, Lv = gpu_device, lsnf.flow, lsnf.langevin
    net = K.module_of(lsnf, p, dev, False)
    torch.manual_seed(0)
    netG = ToyG(nz).to(dev)
    x = torch.tanh(torch.randn(B, 3, 4, 4)).to(dev)
    z0 = torch.randn(B, nz, 1, 1).to(dev)
    kw = dict(g_l_steps=Ks, leapfrog_steps=L, g_l_step_size=s, g_llhd_sigma=sigma)
    ph1, ph2 = F.PhiloxNoise(77, 1000, 0), F.PhiloxNoise(77, 1000, 0)
    z_a, rate_a, u_a = (t.clone() for t in Lv.sample_hmc_post_z_with_flow(z0, x, netG, net, philox=ph1, **kw))
    z_b, rate_b, u_b, steps = Lv.sample_hmc_adaptive_post_z_with_flow(z0, x, netG, net, warmup_steps=0, philox=ph2, **kw)
    assert bits(z_a, z_b) and bits(rate_a, rate_b) and bits(u_a, u_b) and ph1.offset == ph2.offset == 1000 + Ks + 1
    assert isinstance(steps, F.HmcRowSteps) and bool((steps.step == torch.tensor(s).float().item()).all()) and bool((steps.adapt[:, 2] == 0).all())
    assert 0.0 < rate_b.mean().item() < 1.0
    # with warm-up: the hand-written loop of the per-row calls (end calls 1, 2 adapt, the second with "last"; 3, 4 run frozen)
    Ks, W = 4, 2
    kw.update(g_l_steps=Ks)
    ph = F.PhiloxNoise(78, 50, 0)
    first = torch.linspace(0.3, 0.9, B).to(dev)
    z_k, rate, u_k, steps = Lv.sample_hmc_adaptive_post_z_with_flow(z0, x, netG, net, warmup_steps=W, philox=ph, **dict(kw, g_l_step_size=first))
    assert ph.offset == 50 + Ks + 1
    mine, state, zp, flags = F.new_hmc_row_steps(B, dev, first), F.new_hmc_state(net._plan(), B, dev), z0.view(B, nz).clone(), []
    for j in range(Ks * L + 1):
        zr = zp.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = 1.0 / (2.0 * sigma * sigma) * ((netG(zr) - x) ** 2).flatten(1).sum(1)
        gg = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()
        inner, t = j % L != 0, j // L
        zp, acc, _, _ = net.hmc_step_rows(zr.detach().view(B, nz), gg, energy.detach(), state, None if inner else F.PhiloxNoise(78, 50 + t, 0), mine,
                                          phase="inner" if inner else "end" if j else "init", propose=j < Ks * L,
                                          adapt=None if inner or not j or t > W else "last" if t == W else "update")
        if j and not inner and t > W:
            flags.append(acc.clone())
    assert len(flags) == Ks - W
    assert bits(z_k.view(B, nz), state.z) and bits(u_k, state.energy) and bits(rate, torch.stack(flags).sum(0) / (Ks - W))
    assert bits(steps.step, mine.step) and bits(steps.adapt, mine.adapt) and bool((steps.adapt[:, 2] == W).all()) and not bits(steps.step, first)


def test_sampler_frozen_phase_acceptance_lies_in_the_cpu_band(lsnf, gpu_device):
    dev, F, Lv = gpu_device, lsnf.flow, lsnf.langevin
    net, netG, x, z0, first = HG.warmup_problem(lsnf, K, dev, "z")
    z_k, rate, u_k, steps = Lv.sample_hmc_adaptive_post_z_with_flow(z0, x, netG, net, g_l_steps=R.WARMUP_K + R.FROZEN_K, leapfrog_steps=R.WARMUP_L,
                                                                    warmup_steps=R.WARMUP_K, g_l_step_size=first, g_llhd_sigma=1.0,
                                                                    philox=F.PhiloxNoise(5, 0, 0))
    torch.cuda.synchronize()
    HG.check_frozen_phase_acceptance(SP, rate.cpu(), steps)


# ---------------------------------------------------------------------------------------------
# The golden trained weights (tests/trained_weights.py, TW): the checks above on the scalar module's trained cases, each at its own step.
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_per_row_is_the_scalar_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    HG.check_per_row_is_the_scalar_call(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_adaptation_arithmetic_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    HG.check_adaptation_arithmetic(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))

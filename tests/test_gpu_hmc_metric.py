"""GPU: a diagonal metric per row, estimated in warm-up windows on the device, for Hamiltonian Monte Carlo in z (lsnf_hmc_step_metric,
lsnf_small3_hmcm_kernel), `flow.hmc_step_metric`, `_netF.hmc_step_metric` and `langevin.sample_hmc_metric_post_z_with_flow`.  The checks
are tests/hmc_metric_gpu.py's, shared with tests/test_gpu_rhmc_metric.py; the cases, their teacher-forcing records and their steps are
tests/test_gpu_hmc.py's.

1. a unit scale is the per-row call, bit for bit, in every phase, with tensors and with Philox, with and without adaptation, on every
   instantiation of the kernel; scale, mean, m2 and count are untouched;
2. a power-of-two scale 2^k at step s is the per-row call at step s 2^k, bit for bit;
3. a column-varying scale 2^U(-3, 3): every call teacher-forced against float64 under the scalar module's gates, the begin to the bit
   from the device's own stored state; in place, 4 bytes off a 16-byte boundary, NULL optionals;
4. a fold from an empty window stores the state after the decision to the bit (accepted and rejected rows); from windows of 1 and 50
   states it follows float64 within 1e-5 of the magnitudes entering mean' and m2' (widened by the fp32 restatement's own error);
5. a close: sd' against float64 under the same rule, zeros for the window, a single-state window keeps its scale's bits, clamped rows
   sit at the clamp, the dual averaging restarts at log(10 s') with "update" and is the per-row call's with "last", the next
   trajectory begins with sd' and s' to the bit, and without a next point mom is the full-step momentum at the old step and scale;
6. rows do not depend on B, the workgroup shape or the row0 sharding, scale and accumulators included;
7. a NaN row rejects, folds its kept state and leaves every other row's bits alone;
9. the sampler on the warm-up experiment's problem lies in the CPU bands of profiles/hmc_metric_cpu.txt, leaves every window closed,
   and with windows=(None, []) is the adaptive sampler bit for bit.
(8, a chain that adapts and folds replayed from captured graphs, is the base-space file's.)"""
import pytest
import torch

import hmc_metric_gpu as MG
import hmc_rows_gpu as HG
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


@pytest.mark.parametrize("nz,w,depth,coupling,B", MG.IDENTITY)
def test_unit_scale_is_the_per_row_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_unit_scale_is_the_per_row_call(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", MG.POWER_OF_TWO)
def test_power_of_two_scale_is_the_per_row_call_at_the_scaled_step(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_power_of_two_scale_is_the_step_times_it(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", MG.COLUMN)
def test_column_scale_follows_float64_and_begins_to_the_bit(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_column_scale_follows_float64(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", MG.FORMS)
def test_in_place_four_bytes_off_and_null_optionals(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_forms(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", MG.WINDOW)
def test_fold(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_fold(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", MG.WINDOW)
def test_close(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_close(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


def test_rows_do_not_depend_on_the_batch_or_the_sharding(lsnf, gpu_device):
    MG.check_rows_do_not_depend_on_the_batch(lsnf, SP, TH.setup_of(lsnf, gpu_device, *MG.C3, 8200))


def test_a_nan_row_folds_its_kept_state_and_is_alone(lsnf, gpu_device):
    MG.check_a_nan_row(lsnf, SP, TH.setup_of(lsnf, gpu_device, *MG.C3, 33))


def test_sampler_lies_in_the_cpu_bands(lsnf, gpu_device):
    dev, F, Lv = gpu_device, lsnf.flow, lsnf.langevin
    net, netG, x, z0, quad = MG.experiment_problem(lsnf, K, dev, "z")
    z_k, rate, u_k, steps, metric = Lv.sample_hmc_metric_post_z_with_flow(
        z0, x, netG, net, g_l_steps=MG.MR.EXP_W + MG.MR.EXP_FROZEN, leapfrog_steps=MG.MR.EXP_L, warmup_steps=MG.MR.EXP_W,
        g_l_step_size=MG.MR.EXP_S0, g_llhd_sigma=1.0, philox=F.PhiloxNoise(5, 0, 0))
    torch.cuda.synchronize()
    assert isinstance(metric, F.HmcRowMetric) and isinstance(steps, F.HmcRowSteps)
    MG.check_sampler_figures(SP, rate, steps, metric, quad)


def test_sampler_without_windows_is_the_adaptive_sampler(lsnf, gpu_device):
    nz, w, B, Ks, W, L, sigma = 20, 12, 37, 4, 2, 2, 0.3
    from oracle import flow_oracle as O
    p = O.init_params(nz, w, 5, seed=8)
    dev, F, Lv = gpu_device, lsnf.flow, lsnf.langevin
    net = K.module_of(lsnf, p, dev, False)
    torch.manual_seed(0)
    netG = ToyG(nz).to(dev)
    x = torch.tanh(torch.randn(B, 3, 4, 4)).to(dev)
    z0 = torch.randn(B, nz, 1, 1).to(dev)
    first = torch.linspace(0.3, 0.9, B).to(dev)
    kw = dict(g_l_steps=Ks, leapfrog_steps=L, warmup_steps=W, g_l_step_size=first, g_llhd_sigma=sigma)
    ph1, ph2 = F.PhiloxNoise(78, 50, 0), F.PhiloxNoise(78, 50, 0)
    z_a, rate_a, u_a, steps_a = Lv.sample_hmc_adaptive_post_z_with_flow(z0, x, netG, net, philox=ph1, **kw)
    z_a, rate_a, u_a = z_a.clone(), rate_a.clone(), u_a.clone()
    z_b, rate_b, u_b, steps_b, metric = Lv.sample_hmc_metric_post_z_with_flow(z0, x, netG, net, philox=ph2, windows=(None, []), **kw)
    assert bits(z_a, z_b) and bits(rate_a, rate_b) and bits(u_a, u_b) and ph1.offset == ph2.offset == 50 + Ks + 1
    assert bits(steps_a.step, steps_b.step) and bits(steps_a.adapt, steps_b.adapt) and bool((steps_b.adapt[:, 2] == W).all())
    assert bool((metric.scale == 1.0).all()) and not metric.count.any() and not metric.mean.any() and not metric.m2.any()
    # with windows it is another chain, and the hand-written loop of the metric calls
    ph3 = F.PhiloxNoise(78, 50, 0)
    z_c, rate_c, u_c, steps_c, metric_c = Lv.sample_hmc_metric_post_z_with_flow(z0, x, netG, net, philox=ph3, windows=(1, [2, 3]),
                                                                               **dict(kw, warmup_steps=4))
    modes, wins = {1: "update", 2: "update", 3: "update", 4: "last"}, {1: "fold", 2: "close", 3: "close", 4: None}
    mine, mm, state, zp = F.new_hmc_row_steps(B, dev, first), F.new_hmc_row_metric(net._plan(), B, dev), F.new_hmc_state(net._plan(), B, dev), z0.view(B, nz).clone()
    for j in range(Ks * L + 1):
        zr = zp.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = 1.0 / (2.0 * sigma * sigma) * ((netG(zr) - x) ** 2).flatten(1).sum(1)
        gg = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()
        inner, t = j % L != 0, j // L
        end = bool(j) and not inner
        zp, acc, _, _ = net.hmc_step_metric(zr.detach().view(B, nz), gg, energy.detach(), state, None if inner else F.PhiloxNoise(78, 50 + t, 0), mine,
                                            mm, phase="inner" if inner else "end" if j else "init", propose=j < Ks * L,
                                            adapt=modes[t] if end else None, window=wins[t] if end else None)
    assert bits(z_c.view(B, nz), state.z) and bits(u_c, state.energy) and bits(steps_c.step, mine.step) and bits(steps_c.adapt, mine.adapt)
    assert all(bits(getattr(metric_c, f), getattr(mm, f)) for f in MG.METRIC)
    assert not bits(metric_c.scale, torch.ones_like(metric_c.scale)) and not metric_c.count.any() and bool((steps_c.adapt[:, 2] == 1).all())
    assert not bits(z_c, z_b)


# ---------------------------------------------------------------------------------------------
# The golden trained weights (tests/trained_weights.py, TW): the checks above on the scalar module's trained cases, each at its own step.
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_unit_scale_is_the_per_row_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_unit_scale_is_the_per_row_call(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_column_scale_follows_float64_and_begins_to_the_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_column_scale_follows_float64(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))

"""GPU: a diagonal metric per row, estimated in warm-up windows on the device, for Hamiltonian Monte Carlo in the flow's base space
(lsnf_reverse_hmc_step_metric, lsnf_small3_rhmcm_kernel), `flow.reverse_hmc_step_metric`, `_netF.reverse_hmc_step_metric` and
`langevin.sample_hmc_metric_post_eps_with_flow`.  The checks are tests/hmc_metric_gpu.py's, shared with tests/test_gpu_hmc_metric.py
(whose docstring lists them); the cases, their teacher-forcing records and their steps are tests/test_gpu_rhmc.py's.  Here as well:

8. a chain with the stash-keeping reverse, a generator, adaptation and folding, captured once per call form and replayed, gives the
   eager run's bits -- steps, adaptation state, scales and accumulators included."""
import pytest
import torch

from oracle import flow_oracle as O
import hmc_metric_gpu as MG
import hmc_rows_gpu as HG
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


@pytest.mark.parametrize("nz,w,depth,coupling,B", MG.IDENTITY)
def test_unit_scale_is_the_per_row_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_unit_scale_is_the_per_row_call(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", MG.POWER_OF_TWO)
def test_power_of_two_scale_is_the_per_row_call_at_the_scaled_step(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_power_of_two_scale_is_the_step_times_it(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", MG.COLUMN)
def test_column_scale_follows_float64_and_begins_to_the_bit(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_column_scale_follows_float64(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", MG.FORMS)
def test_in_place_four_bytes_off_and_null_optionals(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_forms(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", MG.WINDOW)
def test_fold(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_fold(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", MG.WINDOW)
def test_close(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_close(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


def test_rows_do_not_depend_on_the_batch_or_the_sharding(lsnf, gpu_device):
    MG.check_rows_do_not_depend_on_the_batch(lsnf, SP, TR.setup_of(lsnf, gpu_device, *MG.C3, 8200))


def test_a_nan_row_folds_its_kept_state_and_is_alone(lsnf, gpu_device):
    MG.check_a_nan_row(lsnf, SP, TR.setup_of(lsnf, gpu_device, *MG.C3, 33))


def test_graphed_chain_with_adaptation_and_folding_is_the_eager_chain(lsnf, gpu_device):
    """tests/test_gpu_rhmc.py's graphed chain through `reverse_hmc_step_metric`: four trajectories of two steps whose end calls adapt
    the steps and fold (1), close (2), fold (3) and end the warm-up (4, proposing nothing); one capture per call form."""
    nz, w, depth, B, Kt, L, sigma = 20, 12, 5, 37, 4, 2, 0.3
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
    first = torch.linspace(0.2, 0.6, B).to(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    modes, wins = {1: "update", 2: "update", 3: "update", 4: "last"}, {1: "fold", 2: "close", 3: "fold", 4: None}

    class Buffers:
        def __init__(self):
            self.eps, self.z, self.obj = torch.zeros(B, nz, **f32), torch.zeros(B, nz, **f32), torch.zeros(B, **f32)
            self.saved, self.act = torch.zeros(depth - 1, B, nz, **f32), F.new_act_saved(plan, B, dev)
            self.state, self.steps, self.metric = F.new_hmc_state(plan, B, dev), F.new_hmc_row_steps(B, dev, first), F.new_hmc_row_metric(plan, B, dev)

        def tensors(self):
            return [self.eps] + [getattr(self.state, f) for f in HG.FIELDS] + [self.steps.step, self.steps.adapt] + \
                   [getattr(self.metric, f) for f in MG.METRIC]

    def step(b, form, noise):
        phase, propose, adapt, window = form
        with torch.no_grad():
            F.reverse(plan, b.eps, None, out=(b.z, b.obj), act_saved=b.act, z_saved_out=b.saved)
        zr = b.z.view(B, nz, 1, 1).detach().requires_grad_(True)
        energy = 1.0 / (2.0 * sigma * sigma) * ((netG(zr) - x) ** 2).flatten(1).sum(1)
        gg = torch.autograd.grad(energy.sum(), zr)[0].reshape(B, nz).contiguous()
        with torch.no_grad():
            _, acc, la = F.reverse_hmc_step_metric(plan, b.eps, b.saved, b.act, gg, energy.detach(), b.state, noise, b.steps, b.metric,
                                                   phase=phase, propose=propose, inplace=True, adapt=adapt, window=window)
        return acc, la
    forms = [("init", True, None, None) if j == 0 else ("inner", True, None, None) if j % L else ("end", j < Kt * L, modes[j // L], wins[j // L])
             for j in range(Kt * L + 1)]
    # eager
    be = Buffers()
    be.eps.copy_(eps0)
    eager = []
    for j, form in enumerate(forms):
        acc, la = step(be, form, None if form[0] == "inner" else F.PhiloxNoise(21, 300 + j // L, 0))
        if form[0] != "inner":
            eager.append((acc.clone(), la.clone()))
    # graphed: one capture per call form
    bg = Buffers()
    start = [t.clone() for t in bg.tensors()]
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    rng = F.PhiloxNoise(21, 0, 0, offset_dev=ctr)

    def graphed_step(form):
        out = step(bg, form, None if form[0] == "inner" else rng)
        if form[0] != "inner":
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
    assert len(graphs) == 5                                  # init; inner; end that folds; end that closes; the end of the warm-up
    for t, t0 in zip(bg.tensors(), start):
        t.copy_(t0)
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
    for tg, te in zip(bg.tensors(), be.tensors()):
        assert bits(tg, te)
    assert 0 < int(sum(a.sum() for a, _ in eager[1:])) < Kt * B
    # the chain did adapt, close a window (at trajectory 2) and fold one more state (at 3)
    assert not bits(be.steps.step, first) and not bits(be.metric.scale, torch.ones_like(be.metric.scale))
    assert bool((be.metric.count == 1.0).all()) and bool((be.steps.adapt[:, 2] == 2.0).all())


def test_sampler_lies_in_the_cpu_bands(lsnf, gpu_device):
    dev, F, Lv = gpu_device, lsnf.flow, lsnf.langevin
    net, netG, x, e0, quad = MG.experiment_problem(lsnf, K, dev, "eps")
    e_k, z_k, rate, u_k, steps, metric = Lv.sample_hmc_metric_post_eps_with_flow(
        e0, x, netG, net, g_l_steps=MG.MR.EXP_W + MG.MR.EXP_FROZEN, leapfrog_steps=MG.MR.EXP_L, warmup_steps=MG.MR.EXP_W,
        g_l_step_size=MG.MR.EXP_S0, g_llhd_sigma=1.0, philox=F.PhiloxNoise(5, 0, 0))
    torch.cuda.synchronize()
    assert isinstance(metric, F.HmcRowMetric) and isinstance(steps, F.HmcRowSteps)
    MG.check_sampler_figures(SP, rate, steps, metric, quad)


def test_sampler_without_windows_is_the_adaptive_sampler(lsnf, gpu_device):
    nz, w, B, Ks, W, L, sigma = 20, 12, 37, 4, 2, 2, 0.3
    p = O.init_params(nz, w, 5, seed=8)
    dev, F, Lv = gpu_device, lsnf.flow, lsnf.langevin
    net = K.module_of(lsnf, p, dev, False)
    torch.manual_seed(0)
    netG = ToyG(nz).to(dev)
    x = torch.tanh(torch.randn(B, 3, 4, 4)).to(dev)
    e0 = torch.randn(B, nz).to(dev)
    first = torch.linspace(0.2, 0.6, B).to(dev)
    kw = dict(g_l_steps=Ks, leapfrog_steps=L, warmup_steps=W, g_l_step_size=first, g_llhd_sigma=sigma)
    ph1, ph2 = F.PhiloxNoise(78, 50, 0), F.PhiloxNoise(78, 50, 0)
    a = [t.clone() for t in Lv.sample_hmc_adaptive_post_eps_with_flow(e0, x, netG, net, philox=ph1, **kw)[:4]]
    steps_a = F.new_hmc_row_steps(B, dev, first)
    ph1 = F.PhiloxNoise(78, 50, 0)
    Lv.sample_hmc_adaptive_post_eps_with_flow(e0, x, netG, net, philox=ph1, steps=steps_a, **kw)
    e_b, z_b, rate_b, u_b, steps_b, metric = Lv.sample_hmc_metric_post_eps_with_flow(e0, x, netG, net, philox=ph2, windows=(None, []), **kw)
    assert all(bits(s, t) for s, t in zip(a, (e_b, z_b, rate_b, u_b))) and ph1.offset == ph2.offset == 50 + Ks + 1
    assert bits(steps_a.step, steps_b.step) and bits(steps_a.adapt, steps_b.adapt) and bool((steps_b.adapt[:, 2] == W).all())
    assert bool((metric.scale == 1.0).all()) and not metric.count.any() and not metric.mean.any() and not metric.m2.any()
    # with windows it is another chain
    e_c, _, _, _, steps_c, metric_c = Lv.sample_hmc_metric_post_eps_with_flow(e0, x, netG, net, philox=F.PhiloxNoise(78, 50, 0), windows=(1, [2, 3]),
                                                                             **dict(kw, warmup_steps=4))
    assert not bits(e_c, e_b) and not bits(metric_c.scale, torch.ones_like(metric_c.scale)) and not metric_c.count.any()
    assert bool((steps_c.adapt[:, 2] == 1).all())


# ---------------------------------------------------------------------------------------------
# The golden trained weights (tests/trained_weights.py, TW): the checks above on the scalar module's trained cases, each at its own step.
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_unit_scale_is_the_per_row_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_unit_scale_is_the_per_row_call(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_column_scale_follows_float64_and_begins_to_the_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    MG.check_column_scale_follows_float64(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))

"""GPU: a likelihood temperature per row and the fused importance weight of annealed importance sampling, for Hamiltonian Monte Carlo
in the flow's base space (lsnf_reverse_hmc_step_tempered, lsnf_small3_rhmct_kernel), `flow.reverse_hmc_step_tempered`,
`_netF.reverse_hmc_step_tempered` and `langevin.estimate_log_px_ais_eps_with_flow`.  The checks are tests/hmc_tempered_gpu.py's, shared
with tests/test_gpu_hmc_tempered.py (whose docstring lists them); the cases, their teacher-forcing records and their steps are
tests/test_gpu_rhmc.py's.  like_grad is the kernel's own J_{f^-1}(eps)^T grad_g, held to `reverse_backward_z`'s bits.  Here as well:

8. one end call with ANNEAL, captured in a graph and replayed twice with beta_next rewritten between the replays, gives the two eager
   calls' bits -- state, temperatures and weights included."""
import pytest
import torch

import hmc_rows_gpu as HG
import hmc_tempered_gpu as TG
import test_gpu_rhmc as TR
import test_gpu_reverse_keep as K
import trained_weights as TW

pytestmark = pytest.mark.gpu
SP = HG.Space("eps", TR)
bits = HG.bits


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


@pytest.mark.parametrize("nz,w,depth,coupling,B", TG.IDENTITY)
def test_unit_temperature_is_the_metric_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_unit_temperature_is_the_metric_call(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TG.POWER_OF_TWO)
def test_power_of_two_temperature_is_the_metric_call_at_the_scaled_likelihood(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_power_of_two_temperature_is_the_scaled_likelihood(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TG.GENERAL)
def test_general_temperature_follows_float64(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_general_temperature_follows_float64(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TG.ANNEAL)
def test_anneal_lines_hold_on_the_stored_values(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_anneal_lines(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TG.ANNEAL)
def test_fifty_anneals_sum_to_the_float64_weight(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_anneal_sum(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


def test_rows_do_not_depend_on_the_batch_or_the_sharding(lsnf, gpu_device):
    TG.check_rows_do_not_depend_on_the_batch(lsnf, SP, TR.setup_of(lsnf, gpu_device, *HG.C3, 8200))


def test_a_nan_row_anneals_from_its_kept_state_and_is_alone(lsnf, gpu_device):
    TG.check_a_nan_row(lsnf, SP, TR.setup_of(lsnf, gpu_device, *HG.C3, 33))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TG.FORMS)
def test_in_place_off_the_boundary_and_null_optionals(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_forms(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


def test_captured_annealing_end_call_replays_with_a_rewritten_beta_next(lsnf, gpu_device):
    s = TR.setup_of(lsnf, gpu_device, *HG.C3, 33)
    c, dev, F = s.c, gpu_device, lsnf.flow
    B, r = c.B, SP.end_calls(c)[0]
    cut = lambda t: t.float().to(dev).contiguous()
    eps, ge, e = cut(r.e_prop), cut(r.ge), cut(r.e)
    saved, act = TR.stash_at(lsnf, s.plan, eps)
    noise, uniform = HG.draws(lsnf, SP, c, r, "tensors", dev, True)
    beta = TG.beta_rows(B, 5).to(dev)
    bn1 = TG.next_beta(beta, 5)
    bn2 = TG.next_beta(bn1, 6)

    class Buffers:
        def __init__(self):
            self.state, self.steps, self.metric = TR.state_for(lsnf, s, r), F.new_hmc_row_steps(B, dev, c.s), F.new_hmc_row_metric(s.plan, B, dev)
            self.temper = TG.weights_at(TG.new_temper(lsnf, s, B, beta, "old"))
            self.bn = bn1.clone()

        def tensors(self):
            return [getattr(self.state, f) for f in HG.FIELDS] + [self.steps.step, self.metric.scale] + [getattr(self.temper, f) for f in TG.TEMPER] + [self.bn]

    def step(b):
        with torch.no_grad():
            return F.reverse_hmc_step_tempered(s.plan, eps, saved, act, ge, e, b.state, noise, b.steps, b.metric, b.temper, phase="end",
                                               uniform=uniform, propose=True, anneal=b.bn)
    # eager: two calls, the second annealing on to bn2
    be = Buffers()
    first = [t.clone() for t in step(be)]
    mid = [t.clone() for t in be.tensors()]
    be.bn.copy_(bn2)
    second = [t.clone() for t in step(be)]
    # graphed: ONE capture, replayed twice
    bg = Buffers()
    start = [t.clone() for t in bg.tensors()]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                            # warm-up off the capture stream
        step(bg)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(bg)
    for t, t0 in zip(bg.tensors(), start):
        t.copy_(t0)
    graph.replay()
    got1 = [t.clone() for t in out]
    assert all(bits(a, b) for a, b in zip(bg.tensors(), mid))
    bg.bn.copy_(bn2)
    graph.replay()
    got2 = [t.clone() for t in out]
    torch.cuda.synchronize()
    assert all(bits(a, b) for a, b in zip(got1, first)) and all(bits(a, b) for a, b in zip(got2, second))
    assert all(bits(a, b) for a, b in zip(bg.tensors(), be.tensors()))
    # both calls annealed: the temperatures are the second call's, the weights moved twice
    assert bits(be.temper.beta, bn2) and bits(mid[7], bn1) and not bits(mid[10], start[10]) and not bits(be.temper.log_w, mid[10])
    assert 0 < int(first[1].sum()) < B


def test_sampler_finds_the_closed_form(lsnf, gpu_device):
    TG.check_samplers(lsnf, SP, K, gpu_device)


# ---------------------------------------------------------------------------------------------
# The golden trained weights (tests/trained_weights.py, TW): the checks above on the scalar module's trained cases, each at its own step.
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_unit_temperature_is_the_metric_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_unit_temperature_is_the_metric_call(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_general_temperature_follows_float64_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_general_temperature_follows_float64(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_anneal_lines_hold_on_the_stored_values_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_anneal_lines(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_fifty_anneals_sum_to_the_float64_weight_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_anneal_sum(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))

"""GPU: replica exchange (parallel tempering) between rows at distinct temperatures, fused into the end call of Hamiltonian Monte
Carlo in the flow's base space (lsnf_reverse_hmc_step_exchange, lsnf_small3_rhmcx_kernel), `flow.reverse_hmc_step_exchange`,
`_netF.reverse_hmc_step_exchange` and `langevin.sample_hmc_pt_post_eps_with_flow`.  The checks are tests/hmc_exchange_gpu.py's, shared
with tests/test_gpu_hmc_exchange.py (whose docstring lists them); the cases, their teacher-forcing records and their steps are
tests/test_gpu_rhmc.py's.  The state is (eps, eps + beta like_grad, |eps|^2 / 2 + beta like_energy) with like_grad the kernel's own
J_{f^-1}(eps)^T grad_g.  The swap, its next trajectory, the in-kernel uniform and the call forms of a swapping call run the same case lists
(tests/hmc_exchange_gpu.py SWAP, NEXT, UNIFORM, FORMS: C3, TINY, C5 and the geometry classes of tests/chain_geometries.py).  Here as well:

7. one swapping end call that draws in-kernel, captured in a graph and replayed, gives the eager call's bits -- state, likelihood
   parts, swapped and log_swap included."""
import pytest
import torch

import hmc_exchange_gpu as XG
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


@pytest.mark.parametrize("nz,w,depth,coupling,B", XG.IDENTITY)
def test_without_swap_every_phase_is_the_tempered_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B):
    XG.check_no_swap_is_the_tempered_call(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", XG.SWAP)
def test_swap_is_the_restated_exchange_of_the_plain_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    XG.check_swap_bits(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), R)


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", XG.NEXT)
def test_next_trajectory_of_a_swapping_call_follows_float64(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    XG.check_next_trajectory_follows_float64(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), R)


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", XG.UNIFORM)
def test_in_kernel_swap_uniform_is_philox_field_3_of_the_lower_row(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    XG.check_in_kernel_uniform(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), R)


def test_captured_swapping_end_call_replays_to_the_same_bits(lsnf, gpu_device):
    s = TR.setup_of(lsnf, gpu_device, *XG.C3, 64)
    c, dev, F = s.c, gpu_device, lsnf.flow
    B, R, r = c.B, 8, SP.end_calls(c)[0]
    cut = lambda t: t.float().to(dev).contiguous()
    eps, ge, e = cut(r.e_prop), cut(r.ge), cut(r.e)
    saved, act = TR.stash_at(lsnf, s.plan, eps)
    beta = (torch.linspace(0.2, 1.4, R).repeat(B // R) + 0.05 * torch.rand(B, generator=torch.Generator().manual_seed(7200))).float()

    class Buffers:
        def __init__(self):
            self.state, self.steps, self.metric = TR.state_for(lsnf, s, r), F.new_hmc_row_steps(B, dev, c.s), F.new_hmc_row_metric(s.plan, B, dev)
            self.temper = TG.new_temper(lsnf, s, B, beta, "old")

        def tensors(self):
            return [getattr(self.state, f) for f in HG.FIELDS] + [self.steps.step, self.metric.scale] + [getattr(self.temper, f) for f in TG.TEMPER]

    def step(b):
        with torch.no_grad():
            return F.reverse_hmc_step_exchange(s.plan, eps, saved, act, ge, e, b.state, F.PhiloxNoise(41, 9, 0), b.steps, b.metric, b.temper,
                                               phase="end", propose=True, swap="even", ladder=R)
    be = Buffers()
    eager = [t.clone() for t in step(be)]
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
    torch.cuda.synchronize()
    assert all(bits(a, b) for a, b in zip(out, eager)) and all(bits(a, b) for a, b in zip(bg.tensors(), be.tensors()))
    assert 0 < int(eager[3].sum()) < B and 0 < int(eager[1].sum()) < B     # some pairs swapped, some trajectories were accepted
    assert not bits(be.state.z, start[0])


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", XG.FORMS)
def test_swapping_call_in_place_four_bytes_off_null_optionals_and_reused_buffers(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    XG.check_swap_forms(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), R)


def test_sampler_is_the_hand_written_loop(lsnf, gpu_device, monkeypatch):
    XG.check_samplers(lsnf, SP, K, gpu_device, monkeypatch)


# ---------------------------------------------------------------------------------------------
# The golden trained weights (tests/trained_weights.py, TW): the checks above on the scalar module's trained cases, each at its own step.
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_without_swap_every_phase_is_the_tempered_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    XG.check_no_swap_is_the_tempered_call(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", TW.LADDERS)
def test_swap_is_the_restated_exchange_of_the_plain_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    XG.check_swap_bits(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED), R)


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", TW.LADDERS)
def test_next_trajectory_of_a_swapping_call_follows_float64_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    XG.check_next_trajectory_follows_float64(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED), R)

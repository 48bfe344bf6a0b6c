"""GPU: the resampling move of a sequential Monte Carlo sampler, fused into the annealing end call of Hamiltonian Monte Carlo in the
flow's base space (lsnf_reverse_hmc_step_resample, lsnf_small3_rhmcs_kernel), `flow.reverse_hmc_step_resample`,
`_netF.reverse_hmc_step_resample` and `langevin.estimate_log_px_smc_eps_with_flow`.  The checks are tests/hmc_resample_gpu.py's, shared
with tests/test_gpu_hmc_resample.py (whose docstring lists them); the cases, their teacher-forcing records and their steps are
tests/test_gpu_rhmc.py's.  The state is (eps, eps + beta like_grad, |eps|^2 / 2 + beta like_energy) with like_grad the kernel's own
J_{f^-1}(eps)^T grad_g.  Here as well:

8. one resampling end call that draws in-kernel, captured in a graph and replayed, gives the eager call's bits -- state, likelihood
   parts, weights, ancestor and ess included."""
import pytest
import torch

import hmc_resample_gpu as SG
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


@pytest.mark.parametrize("nz,w,depth,coupling,B", SG.IDENTITY)
def test_without_resample_every_phase_is_the_tempered_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B):
    SG.check_no_resample_is_the_tempered_call(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B,P", SG.MOVE)
def test_move_is_the_restated_resampling_of_the_plain_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B, P):
    SG.check_move_bits(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), P)


@pytest.mark.parametrize("nz,w,depth,coupling,B,P", SG.UNIFORM)
def test_always_never_and_equal_weights(lsnf, gpu_device, nz, w, depth, coupling, B, P):
    SG.check_always_and_never(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), P)


@pytest.mark.parametrize("nz,w,depth,coupling,B,P", SG.UNIFORM)
def test_in_kernel_uniform_is_philox_field_4_of_the_groups_first_row(lsnf, gpu_device, nz, w, depth, coupling, B, P):
    SG.check_in_kernel_uniform(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), P)


def test_captured_resampling_end_call_replays_to_the_same_bits(lsnf, gpu_device):
    s = TR.setup_of(lsnf, gpu_device, *SG.C3, 64)
    c, dev, F = s.c, gpu_device, lsnf.flow
    B, P, r = c.B, 8, SP.end_calls(c)[0]
    cut = lambda t: t.float().to(dev).contiguous()
    eps, ge, e = cut(r.e_prop), cut(r.ge), cut(r.e)
    saved, act = TR.stash_at(lsnf, s.plan, eps)
    beta = TG.beta_rows(B, 9, lo=0.1, hi=0.9)
    bn = TG.next_beta(beta, 9).to(dev)

    class Buffers:
        def __init__(self):
            self.state, self.steps, self.metric = TR.state_for(lsnf, s, r), F.new_hmc_row_steps(B, dev, c.s), F.new_hmc_row_metric(s.plan, B, dev)
            self.temper = TG.weights_at(TG.new_temper(lsnf, s, B, beta, "old"))
            self.temper.log_w[:, 0] *= 0.3

        def tensors(self):
            return [getattr(self.state, f) for f in HG.FIELDS] + [self.steps.step, self.metric.scale] + [getattr(self.temper, f) for f in TG.TEMPER]

    def step(b):
        with torch.no_grad():
            return F.reverse_hmc_step_resample(s.plan, eps, saved, act, ge, e, b.state, F.PhiloxNoise(41, 9, 0), b.steps, b.metric, b.temper,
                                               phase="end", propose=True, anneal=bn, resample=P, ess_threshold=0.5)
    be = Buffers()
    eager = [t.clone() for t in step(be)]
    bg = Buffers()
    start = [t.clone() for t in bg.tensors()]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                            # warm-up off the capture stream
        step(bg)
    torch.cuda.current_stream(dev).wait_stream(side)
    for t, t0 in zip(bg.tensors(), start):
        t.copy_(t0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(bg)
    for t, t0 in zip(bg.tensors(), start):
        t.copy_(t0)
    graph.replay()
    torch.cuda.synchronize()
    assert all(bits(a, b) for a, b in zip(out, eager)) and all(bits(a, b) for a, b in zip(bg.tensors(), be.tensors()))
    own = (torch.arange(B) % P).float().to(dev)
    assert 0 < int((eager[3] != own).sum()) < B              # some rows took another row's state, some kept their own
    assert not bits(be.state.z, start[0])


@pytest.mark.parametrize("nz,w,depth,coupling,B,P", SG.FORMS)
def test_resampling_call_in_place_four_bytes_off_null_optionals_and_reused_buffers(lsnf, gpu_device, nz, w, depth, coupling, B, P):
    SG.check_move_forms(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), P)


@pytest.mark.parametrize("nz,w,depth,coupling,B,P", SG.UNIFORM[:2])
def test_a_nan_row_leaves_its_group_alone_and_the_others_untouched(lsnf, gpu_device, nz, w, depth, coupling, B, P):
    SG.check_a_nan_row(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), P)


def test_sampler_is_the_hand_written_loop(lsnf, gpu_device, monkeypatch):
    SG.check_samplers(lsnf, SP, K, gpu_device, monkeypatch)


def test_sampler_lands_inside_the_cpu_experiments_band(lsnf, gpu_device):
    SG.check_sampler_band(lsnf, SP, K, gpu_device)


# ---------------------------------------------------------------------------------------------
# The golden trained weights (tests/trained_weights.py, TW): the checks above on the scalar module's trained cases, each at its own step.
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_without_resample_every_phase_is_the_tempered_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    SG.check_no_resample_is_the_tempered_call(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", TW.LADDERS)
def test_move_is_the_restated_resampling_of_the_plain_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    SG.check_move_bits(lsnf, SP, TR.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED), R)

"""GPU: the groups' next temperature searched inside the annealing call of Hamiltonian Monte Carlo in z (lsnf_hmc_step_schedule,
lsnf_small3_hmca_kernel), `flow.hmc_step_schedule`, `_netF.hmc_step_schedule` and `langevin.estimate_log_px_smc_adaptive_z_with_flow`.
The checks are tests/hmc_schedule_gpu.py's, shared with tests/test_gpu_rhmc_schedule.py; the cases, their teacher-forcing records and
their steps are tests/test_gpu_hmc.py's.

1. Without `schedule` every phase and form is the resampling call bit for bit (every instantiation, by the dispatch rule).
2. With it, the device against itself, on INIT and on end calls, with and without RESAMPLE: the resampling entry called from the same
   inputs with beta_next = beta' gives every output bit for bit.
3. beta' is equal on the rows of a group and within the derived bound of the float64 root of cess64(delta) = target; every launch of
   three groups or more has groups that search, groups that reach their ceiling and groups at it (tests/hmc_schedule_gpu.py `design`).
4. The hand-made edge groups of tests/test_hmc_schedule_cpu.py on the device.
5. The call forms: in place, 4 bytes off, NULL optionals, reused buffers, tensor noise and Philox, a group alone at row0 = k P.
6. One scheduling, resampling end call that draws in-kernel, captured in a graph and replayed twice with beta_rows advancing between
   the replays, gives the two eager calls' bits -- state, likelihood parts, weights, temperatures, ancestor and ess included.
7. The sampler is the hand-driven loop of `_netF.hmc_step_schedule` calls, with its launch counts, `resampled`, `steps_used`, the
   Philox offset and `check_every` leaving early; it lands inside the CPU experiment's bands."""
import pytest

import hmc_rows_gpu as HG
import hmc_schedule_gpu as AG
import test_gpu_hmc as TH
import test_gpu_reverse_keep as K
import trained_weights as TW

pytestmark = pytest.mark.gpu
SP = HG.Space("z", TH)


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


@pytest.mark.parametrize("nz,w,depth,coupling,B", AG.IDENTITY)
def test_without_schedule_every_phase_is_the_resampling_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B):
    AG.check_no_schedule_is_the_resample_call(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B,P", AG.MOVE)
def test_schedule_is_the_resampling_call_at_its_own_beta_and_within_the_bound_of_float64(lsnf, gpu_device, nz, w, depth, coupling, B, P):
    AG.check_schedule_against_itself_and_float64(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), P)


@pytest.mark.parametrize("nz,w,depth,coupling,B,P", AG.EDGE)
def test_hand_made_edge_groups(lsnf, gpu_device, nz, w, depth, coupling, B, P):
    AG.check_edge_groups(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), P)


@pytest.mark.parametrize("nz,w,depth,coupling,B,P", AG.FORMS)
def test_scheduling_call_in_place_four_bytes_off_null_optionals_reused_buffers_and_sharded(lsnf, gpu_device, nz, w, depth, coupling, B, P):
    AG.check_schedule_forms(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), P)


def test_captured_scheduling_end_call_replays_to_the_same_bits_with_beta_advancing(lsnf, gpu_device):
    AG.check_captured_call(lsnf, SP, TH.setup_of(lsnf, gpu_device, *AG.C3, 64))


def test_sampler_is_the_hand_written_loop(lsnf, gpu_device, monkeypatch):
    AG.check_samplers(lsnf, SP, K, gpu_device, monkeypatch)


def test_sampler_lands_inside_the_cpu_experiments_band(lsnf, gpu_device):
    AG.check_sampler_band(lsnf, SP, K, gpu_device)


# ---------------------------------------------------------------------------------------------
# The golden trained weights (tests/trained_weights.py, TW): the checks above on the scalar module's trained cases, each at its own step.
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_without_schedule_every_phase_is_the_resampling_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    AG.check_no_schedule_is_the_resample_call(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", TW.LADDERS)
def test_schedule_is_the_resampling_call_at_its_own_beta_and_within_the_bound_of_float64_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    AG.check_schedule_against_itself_and_float64(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED), R)

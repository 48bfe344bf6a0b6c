"""GPU: the resampling move of a sequential Monte Carlo sampler, fused into the annealing end call of Hamiltonian Monte Carlo in z
(lsnf_hmc_step_resample, lsnf_small3_hmcs_kernel), `flow.hmc_step_resample`, `_netF.hmc_step_resample` and
`langevin.estimate_log_px_smc_z_with_flow`.  The checks are tests/hmc_resample_gpu.py's, shared with tests/test_gpu_rhmc_resample.py;
the cases, their teacher-forcing records and their steps are tests/test_gpu_hmc.py's.

1. Without `resample` every phase and form is the tempered call bit for bit (every instantiation, by the dispatch rule).
2. The move, the device against itself: from the stored state of the same annealing call without the flag, `ancestor` is the forced
   float64 decision, the state is the restated gather and re-temper to the bit, rows that keep their state and groups that do not
   resample have the plain call's bits, the next trajectory is the fp32 lines on the resampled state; ess and the new log_w are held to
   float64 under the restatement's bounds (tests/hmc_resample_gpu.py's docstring: the forcing, the margins, the threshold at P = 2).
3. ess_threshold = 2 resamples every group, 0 none; equal weights leave every row its own ancestor whatever u is.
4. The in-kernel uniform is Philox field 4 of the group's first row; a group alone at row0 = k P is group k of the batch.
5. The call forms of a resampling call: in place, 4 bytes off, NULL optionals, reused buffers.
6. A NaN row leaves its group unresampled and the others untouched.
7. The sampler is the hand-driven loop of `_netF.hmc_step_resample` calls, with its launch counts, `resampled` and Philox offset.
(A captured resampling end call replayed is the base-space file's.)"""
import pytest

import hmc_resample_gpu as SG
import hmc_rows_gpu as HG
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


@pytest.mark.parametrize("nz,w,depth,coupling,B", SG.IDENTITY)
def test_without_resample_every_phase_is_the_tempered_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B):
    SG.check_no_resample_is_the_tempered_call(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B,P", SG.MOVE)
def test_move_is_the_restated_resampling_of_the_plain_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B, P):
    SG.check_move_bits(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), P)


@pytest.mark.parametrize("nz,w,depth,coupling,B,P", SG.UNIFORM)
def test_always_never_and_equal_weights(lsnf, gpu_device, nz, w, depth, coupling, B, P):
    SG.check_always_and_never(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), P)


@pytest.mark.parametrize("nz,w,depth,coupling,B,P", SG.UNIFORM)
def test_in_kernel_uniform_is_philox_field_4_of_the_groups_first_row(lsnf, gpu_device, nz, w, depth, coupling, B, P):
    SG.check_in_kernel_uniform(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), P)


@pytest.mark.parametrize("nz,w,depth,coupling,B,P", SG.FORMS)
def test_resampling_call_in_place_four_bytes_off_null_optionals_and_reused_buffers(lsnf, gpu_device, nz, w, depth, coupling, B, P):
    SG.check_move_forms(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), P)


@pytest.mark.parametrize("nz,w,depth,coupling,B,P", SG.UNIFORM[:2])
def test_a_nan_row_leaves_its_group_alone_and_the_others_untouched(lsnf, gpu_device, nz, w, depth, coupling, B, P):
    SG.check_a_nan_row(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), P)


def test_sampler_is_the_hand_written_loop(lsnf, gpu_device, monkeypatch):
    SG.check_samplers(lsnf, SP, K, gpu_device, monkeypatch)


def test_sampler_lands_inside_the_cpu_experiments_band(lsnf, gpu_device):
    SG.check_sampler_band(lsnf, SP, K, gpu_device)


# ---------------------------------------------------------------------------------------------
# The golden trained weights (tests/trained_weights.py, TW): the checks above on the scalar module's trained cases, each at its own step.
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_without_resample_every_phase_is_the_tempered_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    SG.check_no_resample_is_the_tempered_call(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", TW.LADDERS)
def test_move_is_the_restated_resampling_of_the_plain_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    SG.check_move_bits(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED), R)

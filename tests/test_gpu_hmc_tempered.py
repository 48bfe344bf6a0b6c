"""GPU: a likelihood temperature per row and the fused importance weight of annealed importance sampling, for Hamiltonian Monte Carlo
in z (lsnf_hmc_step_tempered, lsnf_small3_hmct_kernel), `flow.hmc_step_tempered`, `_netF.hmc_step_tempered` and
`langevin.estimate_log_px_ais_z_with_flow`.  The checks are tests/hmc_tempered_gpu.py's, shared with tests/test_gpu_rhmc_tempered.py; the
cases, their teacher-forcing records and their steps are tests/test_gpu_hmc.py's.

1. beta = 1 without ANNEAL is the metric call, bit for bit, in every phase, with tensors and with Philox, with and without adaptation
   and windows, on every instantiation of the kernel; like_grad / like_energy hold gl / el on accepted rows and their old bits on
   rejected ones; beta and log_w are untouched;
2. beta = 2^k (k = -2, 0, 3 cycled over the rows) is the metric call at (2^k grad_g, 2^k energy_g), bit for bit;
3. a general beta per row (U(0, 1), with 0.0 and 1.5): every call teacher-forced against float64 under the scalar module's gates;
4. ANNEAL: from the device's own stored state the header's fp32 lines hold to the bit -- beta, energy and grad of EVERY row, the
   Kahan pair, the next trajectory's momentum and point from the re-tempered gradient -- for INIT and for end calls that do and do not
   propose; after 50 annealing calls log_weight() is the float64 sum within 1e-6 of the sum of the increments' magnitudes;
5. rows do not depend on B, the workgroup shape or the row0 sharding, the five new arrays included;
6. a NaN row rejects, anneals from its kept state and leaves every other row's bits alone;
7. in place, every tensor off its 16-byte boundary (log_w stays 8-byte aligned), NULL grad_g / energy_g are zeros;
9. the sampler on the CPU experiment's problem lies in the bands of profiles/ais_cpu.txt around each datum's closed form, ends at
   beta = 1, is plain importance sampling with betas = [0, 1], and is the hand-written loop of `_netF.hmc_step_tempered` calls bit for bit.
(8, a captured annealing end call replayed with beta_next rewritten, is the base-space file's.)"""
import pytest

import hmc_rows_gpu as HG
import hmc_tempered_gpu as TG
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


@pytest.mark.parametrize("nz,w,depth,coupling,B", TG.IDENTITY)
def test_unit_temperature_is_the_metric_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_unit_temperature_is_the_metric_call(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TG.POWER_OF_TWO)
def test_power_of_two_temperature_is_the_metric_call_at_the_scaled_likelihood(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_power_of_two_temperature_is_the_scaled_likelihood(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TG.GENERAL)
def test_general_temperature_follows_float64(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_general_temperature_follows_float64(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TG.ANNEAL)
def test_anneal_lines_hold_on_the_stored_values(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_anneal_lines(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TG.ANNEAL)
def test_fifty_anneals_sum_to_the_float64_weight(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_anneal_sum(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


def test_rows_do_not_depend_on_the_batch_or_the_sharding(lsnf, gpu_device):
    TG.check_rows_do_not_depend_on_the_batch(lsnf, SP, TH.setup_of(lsnf, gpu_device, *HG.C3, 8200))


def test_a_nan_row_anneals_from_its_kept_state_and_is_alone(lsnf, gpu_device):
    TG.check_a_nan_row(lsnf, SP, TH.setup_of(lsnf, gpu_device, *HG.C3, 33))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TG.FORMS)
def test_in_place_off_the_boundary_and_null_optionals(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_forms(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


def test_sampler_finds_the_closed_form(lsnf, gpu_device):
    TG.check_samplers(lsnf, SP, K, gpu_device)


# ---------------------------------------------------------------------------------------------
# The golden trained weights (tests/trained_weights.py, TW): the checks above on the scalar module's trained cases, each at its own step.
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_unit_temperature_is_the_metric_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_unit_temperature_is_the_metric_call(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_general_temperature_follows_float64_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_general_temperature_follows_float64(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_anneal_lines_hold_on_the_stored_values_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_anneal_lines(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_fifty_anneals_sum_to_the_float64_weight_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    TG.check_anneal_sum(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))

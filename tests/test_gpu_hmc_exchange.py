"""GPU: replica exchange (parallel tempering) between rows at distinct temperatures, fused into the end call of Hamiltonian Monte
Carlo in z (lsnf_hmc_step_exchange, lsnf_small3_hmcx_kernel), `flow.hmc_step_exchange`, `_netF.hmc_step_exchange` and
`langevin.sample_hmc_pt_post_z_with_flow`.  The checks are tests/hmc_exchange_gpu.py's, shared with tests/test_gpu_rhmc_exchange.py; the
cases, their teacher-forcing records and their steps are tests/test_gpu_hmc.py's.

1. without swap every phase, form and instantiation of the kernel gives the tempered call's bits -- with tensors and with Philox, at
   a general beta per row, with and without adaptation, windows and the anneal -- and returns no swapped / log_swap;
2. the swap's state, the device against itself: the end call with the swap against the same call without it on the same inputs and
   the restated fp32 exchange (tests/hmc_exchange_restated.py) applied to that call's stored result -- state.z, state.grad,
   state.energy, like_grad, like_energy, swapped and log_swap to the bit; both parities, R = 2, 4, 8, 16, with and without a next
   point; B = R, a ragged tile (24 rows of R = 8), two and four ladders of 16 (32 and 64 rows), and 4100 / 8200 / 16400 rows (16, 32 and
   64 rows per workgroup) at C3 (128, 64), TINY (8, 4) and C5 (100, 128; half 50); every geometry of tests/chain_geometries.py at
   24 rows of R = 8, every R at a ragged half -- (66, 33) as two ladders of 16 and as 4 rows of R = 2, (62, 31) as one ladder of 16,
   (12, 100) as 20 rows of R = 4 --, the empty second half-tile of <2, 2> and <2, 4>, additive coupling, and (66, 33) at 4100 rows of
   R = 4 / (10, 40) at 8200 rows of R = 8 (32 and 64 rows per workgroup); the pairs' uniforms forced from the float64 log_r at a
   margin of 1 nat, every case with a swapping and a non-swapping pair (R = 2 with odd parity: no pair at all);
3. the next trajectory of a swapping call (z_next, state.mom, state.kin) against float64 under hmc_metric_gpu.gates -- C3, TINY, and
   (124, 63) (half 62: a four-column draw straddles the end of the half) and (10, 40) (an empty half-tile);
4. beta, step, scale, adapt and the window accumulators do not move, and rows that do not swap -- idle rungs among them -- have the
   call-without-swap's bits (checked with 2.);
5. with a PhiloxNoise the pair's uniform is Philox at field 3 of the lower row's counter: the tensor form with the restated draws gives
   the same bits, a ladder alone at row0 = k R gives ladder k of the whole batch, the trajectory's own uniforms in their place do not
   (C3, TINY, (66, 33) and (10, 40));
6. the sampler (K = 6, N = 2, R = 4) is the same sequence of `_netF.hmc_step_exchange` calls driven by hand, bit for bit; swap_rate is
   the mean of swapped per pair; the flow's side launches one forward and one exchanging call per leapfrog step and nothing else.
8. the call forms of a swapping end call at the four call-form geometries of tests/chain_geometries.py (24 rows of R = 8, odd
   parity): in place, every tensor 4 bytes off a 16-byte boundary, grad_g = energy_g = None (every pair swaps), reuse_buffers=True --
   each the plain form's bits.
(A captured swapping end call replayed, 7., is the base-space file's.  tests/test_chain_geometries_cpu.py holds the case lists to the
geometry table; profiles/hmc_exchange_geometries.txt has the figures and the mutants the swap cases catch.)"""
import pytest

import hmc_exchange_gpu as XG
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


@pytest.mark.parametrize("nz,w,depth,coupling,B", XG.IDENTITY)
def test_without_swap_every_phase_is_the_tempered_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B):
    XG.check_no_swap_is_the_tempered_call(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B))


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", XG.SWAP)
def test_swap_is_the_restated_exchange_of_the_plain_call_bit_for_bit(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    XG.check_swap_bits(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), R)


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", XG.NEXT)
def test_next_trajectory_of_a_swapping_call_follows_float64(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    XG.check_next_trajectory_follows_float64(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), R)


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", XG.UNIFORM)
def test_in_kernel_swap_uniform_is_philox_field_3_of_the_lower_row(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    XG.check_in_kernel_uniform(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), R)


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", XG.FORMS)
def test_swapping_call_in_place_four_bytes_off_null_optionals_and_reused_buffers(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    XG.check_swap_forms(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B), R)


def test_sampler_is_the_hand_written_loop(lsnf, gpu_device, monkeypatch):
    XG.check_samplers(lsnf, SP, K, gpu_device, monkeypatch)


# ---------------------------------------------------------------------------------------------
# The golden trained weights (tests/trained_weights.py, TW): the checks above on the scalar module's trained cases, each at its own step.
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz,w,depth,coupling,B", TW.SMALL)
def test_without_swap_every_phase_is_the_tempered_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B):
    XG.check_no_swap_is_the_tempered_call(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED))


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", TW.LADDERS)
def test_swap_is_the_restated_exchange_of_the_plain_call_bit_for_bit_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    XG.check_swap_bits(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED), R)


@pytest.mark.parametrize("nz,w,depth,coupling,B,R", TW.LADDERS)
def test_next_trajectory_of_a_swapping_call_follows_float64_at_trained_weights(lsnf, gpu_device, nz, w, depth, coupling, B, R):
    XG.check_next_trajectory_follows_float64(lsnf, SP, TH.setup_of(lsnf, gpu_device, nz, w, depth, coupling, B, weights=TW.TRAINED), R)

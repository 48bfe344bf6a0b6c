"""The trained-weight chain cases (tests/trained_weights.py), on the CPU: the fixtures are the geometries the table says, their weights
really are far from initialisation, every case constructs in all four Case classes with its assertions intact and its float64 rate
and set-aside counts inside the caps, the diverging records diverge, and every GPU test that is to run the trained cases runs them.
Importing the GPU test modules needs no device."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import flow_oracle as O
import chain_geometries as G
import trained_weights as T
import test_gpu_hmc as HZ
import test_gpu_mala as MZ
import test_gpu_reverse_keep as K
import test_gpu_reverse_langevin as RL
import test_gpu_rhmc as HE
import test_gpu_rmala as ME

KINDS = {"hmc z": HZ, "hmc eps": HE, "mala z": MZ, "mala eps": ME}


def cases_of(test):
    """The argument list of a test's (single) parametrize mark."""
    (mark,) = [m for m in test.pytestmark if m.name == "parametrize"]
    return list(mark.args[1])


def test_every_fixture_is_its_case_geometry():
    assert set(T.WEIGHTS) == {T.C3, T.C5, T.TINY} == {c[:4] for c in T.CASES}
    assert {G.pick_tiles(geo[0] // 2, geo[1]) for geo in T.WEIGHTS} == {(1, 1), (2, 2), (2, 4)}       # the three instantiations
    for geo, name in T.WEIGHTS.items():
        p, rest = load_golden(name)
        nz, w, depth, coupling = geo
        assert (int(rest["meta_nz"]), int(rest["meta_width"]), int(rest["meta_depth"])) == (nz, w, depth)
        assert O.depth_of(p) == depth and O.coupling_of(p) == coupling
        init = O.init_params(nz, w, depth, seed=3)
        assert set(p) == set(init) and all(p[k].shape == init[k].shape for k in p)
        q = T.params_of(geo)
        assert set(q) == set(p) and all(bool(torch.equal(q[k], p[k])) for k in p)
    assert T.CASES == [T.C3 + (B,) for B in (33, 100, 4100, 8200)] + [T.C5 + (33,), T.C5 + (4100,), T.TINY + (33,)]
    assert T.SMALL == [c for c in T.CASES if c[4] == 33] and len(T.SMALL) == 3


def test_the_weights_are_far_from_initialisation():
    rms = lambda t: t.double().pow(2).mean().sqrt().item()
    for geo in T.WEIGHTS:
        p, init = T.params_of(geo), O.init_params(*geo[:3], seed=3)
        logs = max(p[k].abs().max().item() for k in p if k.endswith("fc_zeros.logs"))
        if geo != T.TINY:
            assert 3.0 * logs >= 1.0, (geo, logs)
        # Every live tensor (the fc biases are dead: the reference never trains them, and both sets hold zeros there) has a larger RMS
        # than oracle.init_params(seed=3) gives it -- but for the two matrices whose size init_params does not start small: fc_zeros.w,
        # which the reference starts at zero and init_params draws at 0.05 so that the coupling is exercised at all (trained: 0.017 ..
        # 0.025 on C3 / C5, 0.12 .. 0.16 on TINY), and the 1x1 convolution, orthogonal at initialisation in both (RMS 1 / sqrt(nz)
        # whatever its entries: 0.0903 against 0.0884 on C3, 0.344 .. 0.388 against 0.354 on TINY).  Those two are held to having moved:
        # fc_zeros.w away from the reference's zero, W away from orthogonal.
        live = [k for k in p if not (k.endswith("fc_1.b") or k.endswith("fc_2.b") or k.endswith("bias"))]
        assert len(live) == 12 * geo[2]
        for k in live:
            if k.endswith("fc_zeros.w"):
                assert rms(p[k]) > 0.01, (geo, k)
            elif k.endswith("invertible_1x1_conv.w"):
                W = p[k].double()
                assert (W @ W.T - torch.eye(geo[0], dtype=torch.float64)).abs().max().item() > 0.05, (geo, k)
                W0 = init[k].double()
                assert (W0 @ W0.T - torch.eye(geo[0], dtype=torch.float64)).abs().max().item() < 1e-5, (geo, k)
            else:
                assert rms(p[k]) > rms(init[k]), (geo, k, rms(p[k]), rms(init[k]))


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_case_constructs_with_its_rate_and_set_aside_counts_inside_the_caps(kind):
    mod = KINDS[kind]
    for cs in T.CASES:
        c = mod.case(*cs, weights=T.TRAINED)                  # (Case's own assertions: the u_acc bound, the hmc set-aside cap)
        B, geo = cs[4], cs[:4]
        assert c.weights == T.TRAINED and c.s == float(np.float32(T.STEP[kind][geo]))
        records = c.calls if kind.startswith("hmc") else c.steps
        decided = [r for r in records if hasattr(r, "gate")]
        assert len(decided) == ((2 if B <= 100 else 1) if kind.startswith("hmc") else (3 if B <= 100 else 1))
        for r in decided:
            assert int((~r.decided).sum()) <= (2 if B <= 33 else B // 10), (kind, cs)
            # (C3 in eps: a few rows of the batches above 33 leave the stable window in float64; they are among those set aside)
            lost = ~torch.isfinite(r.gate) | ~torch.isfinite(r.la)
            assert not bool((lost & r.decided).any()) and (B > 33 or not bool(lost.any())), (kind, cs)
        if B <= 100:
            assert 0.15 <= c.rate <= 0.85, (kind, cs, c.rate)
    # the selector is part of the cache's key: the init-weight case of a geometry and batch is another object with another flow
    small = T.SMALL[-1]
    assert mod.case(*small) is not mod.case(*small, weights=T.TRAINED) and mod.case(*small).weights == T.INIT


def test_the_ladder_cases_construct_in_both_spaces():
    for mod in (HZ, HE):
        for cs in T.LADDERS:
            c = mod.case(*cs[:5], weights=T.TRAINED)
            assert 0.15 <= c.rate <= 0.85 and cs[4] % cs[5] == 0, (mod.__name__, cs, c.rate)
            assert all(int((~r.decided).sum()) <= 2 for r in c.calls if r.phase == "end")


def test_the_stash_keeping_reverse_cases_construct():
    for cs in T.CASES:
        c = K.case(*cs, weights=T.TRAINED)
        assert c.weights == T.TRAINED and bool(torch.isfinite(c.eps).all())
    assert K.TRAINED_PARAM_CASES == [T.C3 + (100,), T.C3 + (4100,), T.C5 + (33,)]
    assert set(T.LANGEVIN_STEP) == set(T.WEIGHTS)


def test_the_diverging_records_diverge():
    z = HZ.Case(*T.C3, 33, weights=T.TRAINED, s=T.DIVERGING_STEP["hmc z"], diverging=True)
    e = HE.Case(*T.C3, 33, s=T.DIVERGING_STEP["hmc eps"], light=True, weights=T.TRAINED)
    for mod, c in ((HZ, z), (HE, e)):
        r, bad = mod.diverged_rows(c)
        assert r.phase == "end" and int(bad.sum()) >= T.DIVERGING_ROWS and not bool(r.acc[bad].any())
        assert bool(torch.isnan(c.calls[2].g).any())          # a NaN gradient at the second inner call already
        g, gbad = mod.diverging_call(c)                       # three rows grafted from the stable case: finite, and not diverged
        assert int(gbad.sum()) == 33 - len(T.GRAFTED) >= T.DIVERGING_ROWS and not bool(gbad[list(T.GRAFTED)].any())
        assert all(bool(torch.isfinite(getattr(g, k)[list(T.GRAFTED)]).all()) for k in ("la", "mom_in", "ge", "e"))
    assert T.DIVERGING_STEP["hmc z"] == 0.2
    # base space: the smallest multiple of 0.05 that shows it -- one multiple below, the second inner call's gradient is still finite
    below = HE.Case(*T.C3, 33, s=T.DIVERGING_STEP["hmc eps"] - 0.05, light=True, weights=T.TRAINED)
    assert bool(torch.isfinite(below.calls[2].g).all())


def test_every_list_runs_the_trained_cases_it_claims():
    for mod in (HZ, HE):
        assert cases_of(mod.test_every_call_follows_float64_at_trained_weights) == T.CASES
    for mod in (MZ, ME):
        assert cases_of(mod.test_decisions_and_state_follow_float64_at_trained_weights) == T.CASES
    for test in (RL.test_gradient_bits_at_trained_weights, RL.test_update_arithmetic_at_trained_weights, RL.test_norms_at_trained_weights,
                 K.test_keep_form_bits_block_outputs_and_stash_at_trained_weights):
        assert cases_of(test) == T.CASES
    assert cases_of(K.test_parameter_gradients_from_the_reverse_workspace_at_trained_weights) == K.TRAINED_PARAM_CASES
    # the six levels, both spaces: the identity check and the float64-held checks at SMALL, the ladder checks at LADDERS
    import importlib
    levels = {"rows": ["per_row_is_the_scalar_call_bit_for_bit", "adaptation_arithmetic"],
              "metric": ["unit_scale_is_the_per_row_call_bit_for_bit", "column_scale_follows_float64_and_begins_to_the_bit"],
              "tempered": ["unit_temperature_is_the_metric_call_bit_for_bit", "general_temperature_follows_float64",
                           "anneal_lines_hold_on_the_stored_values", "fifty_anneals_sum_to_the_float64_weight"],
              "exchange": ["without_swap_every_phase_is_the_tempered_call_bit_for_bit"],
              "resample": ["without_resample_every_phase_is_the_tempered_call_bit_for_bit"],
              "schedule": ["without_schedule_every_phase_is_the_resampling_call_bit_for_bit"]}
    ladders = {"exchange": ["swap_is_the_restated_exchange_of_the_plain_call_bit_for_bit", "next_trajectory_of_a_swapping_call_follows_float64"],
               "resample": ["move_is_the_restated_resampling_of_the_plain_call_bit_for_bit"],
               "schedule": ["schedule_is_the_resampling_call_at_its_own_beta_and_within_the_bound_of_float64"]}
    for space in ("hmc", "rhmc"):
        for level in levels:
            mod = importlib.import_module(f"test_gpu_{space}_{level}")
            for name in levels[level]:
                assert cases_of(getattr(mod, f"test_{name}_at_trained_weights")) == T.SMALL, (space, level, name)
                assert hasattr(mod, f"test_{name}")                                   # the init-weight check it mirrors
            for name in ladders.get(level, []):
                assert cases_of(getattr(mod, f"test_{name}_at_trained_weights")) == T.LADDERS, (space, level, name)
    assert T.LADDERS == [g + bR for g in (T.C3, T.TINY) for bR in ((24, 8), (32, 16))]
    # the init-weight lists are what they were: no trained case is keyed into them
    for mod in (HZ, HE, MZ, ME, RL):
        assert len(mod.RUNS) == len(set(mod.RUNS))

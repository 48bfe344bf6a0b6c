"""CPU: the adaptive-tempering SMC sampler restated in float64 (tests/hmc_schedule_restated.py `adaptive_chain`) on
tests/ais_restated.py's closed-form problem: one seed in both spaces inside the bands of profiles/smc_adaptive_cpu.txt (seeds 0 .. 7, the
range widened by 3 standard deviations, as smc_restated.BAND was made); the bands' own consistency with that file; that a target so
low that every group jumps to 1 in the init call, with a threshold that never resamples, IS the one-step AIS run to the last bit; and
the schedule's own properties.  What the adaptive schedule buys over the fixed one is a finding recorded in
profiles/smc_adaptive_cpu.txt and DESIGN.md, not a threshold here."""
import ast
import os
import re

import pytest
import torch

from conftest import ROOT
import ais_restated as A
import hmc_schedule_restated as S


def inside(v, band):
    v = torch.as_tensor(v, dtype=torch.float64).reshape(-1)
    return bool(((v >= band[0]) & (v <= band[1])).all())


@pytest.mark.parametrize("space", ("z", "eps"))
def test_one_seed_lies_inside_the_bands(space):
    err, ess, acc, used = S.experiment(0, space)
    band = S.BAND[space]
    print(f"[{space}] adaptive SMC, target {S.EXP_TARGET}, max_steps {S.EXP_MAX_STEPS}: errors {err.tolist()} ess {ess.tolist()} "
          f"acceptance {acc:.4f}; steps used {used.tolist()}")
    assert inside(err, band["error"]) and inside(ess, band["ess"]) and inside(acc, band["accept"]) and inside(used, band["steps"])
    assert used.shape == (len(A.EXP_DATA) * A.EXP_CHAINS // 16,) and float(used.max()) < S.EXP_MAX_STEPS


def test_bands_are_the_profile_s():
    text = open(os.path.join(ROOT, "profiles", "smc_adaptive_cpu.txt")).read()
    for space in ("z", "eps"):
        b = S.BAND[space]
        assert b["error"][0] < 0.0 < b["error"][1] and b["ess"][1] > b["ess"][0] and 0.0 < b["accept"][0] < b["accept"][1] < 1.0
        assert 1.0 <= b["steps"][0] < b["steps"][1] < S.EXP_MAX_STEPS
        line = re.search(r'^# "%s": (.*)$' % space, text, flags=re.M).group(1)
        assert ast.literal_eval(line) == {k: tuple(v) for k, v in b.items()}
    for said in ("fixed T = 20", "fixed T = 100", f"CESS target {S.EXP_TARGET}", "steps used"):
        assert said in text


def test_a_target_every_group_meets_at_once_is_the_one_step_ais_run():
    p = A.affine_flow()
    quads = [A.datum(s) for s in A.EXP_DATA]
    one = A.run(p, quads, "z", torch.tensor([0.0, 1.0], dtype=torch.float64), 2, 16, A.EXP_STEP, 3)
    for K in (2, 4):
        ad = S.run(p, quads, "z", K, 2, 16, A.EXP_STEP, 3, particles=8, cess_target=1e-6, ess_threshold=0.0)
        tr = ad[3]
        assert torch.equal(tr.steps_used, torch.ones(4, dtype=torch.float64)) and bool((tr.betas == 1.0).all()) and not bool(tr.resampled.any())
        assert torch.equal(ad[0], one[0]) and torch.equal(ad[1], one[1])                      # log Z_hat and ess, to the last bit
        assert torch.equal(tr.log_w[0], one[3].log_w[0]) and torch.equal(tr.log_w[1], one[3].log_w[1])
    # max_steps = 1: the init call anneals into the last transition and does not search -- the one-step run whatever the target
    ad = S.run(p, quads, "z", 1, 2, 16, A.EXP_STEP, 3, particles=8, cess_target=0.999, ess_threshold=0.0)
    assert torch.equal(ad[0], one[0]) and ad[2] == one[2] and torch.equal(ad[3].steps_used, torch.ones(4, dtype=torch.float64))


def test_the_schedule_rises_arrives_and_respects_min_step():
    p = A.affine_flow()
    quads = [A.datum(s) for s in A.EXP_DATA]
    K = 12
    _, _, _, tr = S.run(p, quads, "eps", K, 2, 32, A.EXP_STEP, 1, particles=16, cess_target=0.9)
    b = tr.betas                                             # (K, G): after the init call and end calls 1 .. K - 1
    assert b.shape == (K, 4) and bool((b[-1] == 1.0).all()) and bool((b[1:] >= b[:-1]).all()) and bool((b[0] > 0.0).all())
    step = b[1:] - b[:-1]
    moving = b[:-1] < 1.0
    ms = 1.0 / (4.0 * K)
    assert bool(((step >= ms * (1.0 - 1e-12)) | (b[1:] == 1.0))[moving].all())      # every moving step: at least min_step, or onto 1
    assert torch.equal(tr.steps_used, moving.sum(0).double() + 1.0)
    # a tight target does not arrive by itself: the last annealing call takes every group to 1 in one plain step
    _, _, _, tr = S.run(p, quads, "eps", 4, 2, 32, A.EXP_STEP, 1, particles=16, cess_target=0.999, min_step=0.0)
    assert bool((tr.betas[-2] < 1.0).all()) and bool((tr.betas[-1] == 1.0).all()) and bool((tr.steps_used == 4.0).all())
    # the groups of one run choose different schedules
    assert len({round(v, 9) for v in tr.betas[0].tolist()}) > 1

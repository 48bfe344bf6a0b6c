"""CPU: the sequential Monte Carlo sampler restated in float64 (tests/smc_restated.py, tests/hmc_resample_restated.py `smc_chain`) on
tests/ais_restated.py's closed-form problem: one seed at the short schedule (T = 20) in both spaces, beside plain AIS from the same
draws, inside the bands of profiles/smc_cpu.txt (seeds 0 .. 7, the range widened by 3 standard deviations, as ais_restated.BAND was
made); the bands' own consistency; and that a run whose threshold never resamples IS the AIS run.  Whether SMC's spread is smaller than
AIS's is a finding recorded in profiles/smc_cpu.txt and DESIGN.md, not a threshold here."""
import pytest
import torch

import ais_restated as A
import smc_restated as S


def inside(v, band):
    v = torch.as_tensor(v, dtype=torch.float64).reshape(-1)
    return bool(((v >= band[0]) & (v <= band[1])).all())


@pytest.mark.parametrize("space", ("z", "eps"))
def test_one_seed_at_the_short_schedule_lies_inside_the_bands(space):
    T = S.SHORT_T
    err, ess, acc, res = S.experiment(0, space, T=T)
    band = S.BAND["smc"][T][space]
    print(f"[{space}] SMC T={T}: errors {err.tolist()} ess {ess.tolist()} acceptance {acc:.4f}; groups resampled at {res.tolist()} of {T - 1} steps")
    assert inside(err, band["error"]) and inside(ess, band["ess"]) and inside(acc, band["accept"])
    assert res.shape == (len(A.EXP_DATA) * A.EXP_CHAINS // S.EXP_PARTICLES,) and 0 < int(res.sum()) < res.numel() * (T - 1)
    err, ess, acc = A.experiment(0, space, T=T)
    band = S.BAND["ais"][T][space]
    assert inside(err, band["error"]) and inside(ess, band["ess"]) and inside(acc, band["accept"])


def test_bands_hold_the_closed_form_and_the_ais_figures():
    for kind in ("smc", "ais"):
        for T in (A.EXP_T, S.SHORT_T):
            for space in ("z", "eps"):
                b = S.BAND[kind][T][space]
                assert b["error"][0] < 0.0 < b["error"][1] and b["ess"][1] > b["ess"][0] and 0.0 < b["accept"][0] < b["accept"][1] < 1.0
    for space in ("z", "eps"):                               # plain AIS at T = 100 is ais_restated's experiment: the same bands
        for k in ("error", "ess", "accept"):
            for a, b in zip(S.BAND["ais"][A.EXP_T][space][k], A.BAND[space][k]):
                assert abs(a - b) <= 0.1501 if k == "ess" else abs(a - b) <= 0.0011


def test_a_threshold_that_never_resamples_is_the_ais_run():
    p = A.affine_flow()
    quads = [A.datum(s) for s in A.EXP_DATA]
    betas = A.schedule(6)
    a = A.run(p, quads, "z", betas, 2, 16, A.EXP_STEP, 3)
    s = S.run(p, quads, "z", betas, 2, 16, A.EXP_STEP, 3, particles=8, ess_threshold=0.0)
    assert torch.equal(a[0], s[0]) and torch.equal(a[1], s[1]) and a[2] == s[2] and not bool(s[3].resampled.any())
    # and one that always does keeps every group's mean weight: the estimate moves by rounding only
    r = S.run(p, quads, "z", betas[:2], 2, 16, A.EXP_STEP, 3, particles=8, ess_threshold=2.0)
    assert torch.equal(r[0], A.run(p, quads, "z", betas[:2], 2, 16, A.EXP_STEP, 3)[0])      # (T = 1: no resampling step at all)

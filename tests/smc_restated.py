"""TEST INFRASTRUCTURE (CPU; float64): the sequential Monte Carlo sampler (tests/hmc_resample_restated.py `smc_chain`) on
tests/ais_restated.py's closed-form problem, beside plain AIS at the same settings.  `run`: one float64 SMC run with ais_restated.run's
draws (the same generator, the groups' uniforms drawn after them); `experiment`: the errors log Z_hat - closed form, the final ess and
the mean acceptance of one seed; BAND: the figures over seeds 0 .. 7 (profiles/smc_cpu.txt), made as ais_restated.BAND was made."""
import torch

import ais_restated as A
import hmc_resample_restated as R
import hmc_tempered_restated as TR

EXP_PARTICLES, EXP_THRESHOLD, SHORT_T = 16, 0.5, 20


def run(p, quads, space, betas, L, chains, step, seed, particles=EXP_PARTICLES, ess_threshold=EXP_THRESHOLD):
    """One float64 SMC run: (log Z_hat (N), ess (N), the mean acceptance, the trace)."""
    f64 = torch.float64
    T, B, nz = betas.numel() - 1, len(quads) * chains, A.GEO[0]
    g = torch.Generator().manual_seed(5000 + seed)
    x0, _ = A.prior_draws(p, space, B, g)
    noises = [torch.randn(B, nz, generator=g, dtype=f64) for _ in range(T)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g, dtype=f64).clamp_min(2.0 ** -25) for _ in range(T)]
    ru = [None] + [torch.rand(B, generator=g, dtype=f64) for _ in range(T)]
    rows = lambda t: torch.full((B,), float(betas[t]), dtype=f64)
    anneals = [rows(t + 1) for t in range(T)] + [None]
    tr = R.smc_chain(TR.flow_parts(space, p, A.Stacked(quads, chains)), x0, torch.full((B,), step, dtype=f64), torch.ones(B, nz, dtype=f64), L,
                     noises, uniforms, rows(0), anneals, particles, ess_threshold, ru)
    logz, ess = A.reduce(tr.log_w[0] - tr.log_w[1], chains)
    return logz, ess, tr.acc.double().mean().item(), tr


def experiment(seed, space, T=A.EXP_T, L=A.EXP_L, chains=A.EXP_CHAINS, step=A.EXP_STEP, data=A.EXP_DATA):
    """The experiment at one seed: (errors log Z_hat - closed form (N), final ess (N), mean acceptance, resampling steps per group)."""
    p = A.affine_flow()
    quads = [A.datum(s) for s in data]
    logz, ess, acc, tr = run(p, quads, space, A.schedule(T), L, chains, step, seed)
    exact = torch.tensor([A.closed_form(p, q) for q in quads], dtype=torch.float64)
    return logz - exact, ess, acc, tr.resampled.sum(0)


# The figures over seeds 0 .. 7 (profiles/smc_cpu.txt has every seed's figures and the arithmetic; tests/test_smc_cpu.py holds one
# seed to them): [kind][T][space]; error, ess and accept as ais_restated.BAND's.  The "ais" entries are plain AIS at the same settings
# and draws (at T = 100: ais_restated.BAND up to the last digit's rounding).
BAND = {
    "smc": {
        100: {"z": {"error": (-0.81, 0.811), "ess": (15.8, 69.1), "accept": (0.955, 0.97)},
              "eps": {"error": (-0.636, 0.582), "ess": (20.3, 67.7), "accept": (0.889, 0.911)}},
        20: {"z": {"error": (-1.617, 1.926), "ess": (9.5, 62.4), "accept": (0.949, 0.98)},
             "eps": {"error": (-0.969, 1.043), "ess": (17.3, 73.3), "accept": (0.877, 0.924)}},
    },
    "ais": {
        100: {"z": {"error": (-0.862, 0.796), "ess": (9.2, 55.2), "accept": (0.954, 0.97)},
              "eps": {"error": (-0.642, 0.582), "ess": (18.1, 54.2), "accept": (0.889, 0.912)}},
        20: {"z": {"error": (-1.843, 2.177), "ess": (-6.1, 29.2), "accept": (0.949, 0.979)},
             "eps": {"error": (-1.352, 1.625), "ess": (-4.9, 32.9), "accept": (0.878, 0.929)}},
    },
}

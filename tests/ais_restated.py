"""TEST INFRASTRUCTURE (CPU; float64): annealed importance sampling (Neal 2001) with the tempered HMC transitions of
tests/hmc_tempered_restated.py, on a problem whose log p(x) has a closed form.

The problem: `O.init_params(8, 4, 5, seed=3, fcz_std=0.0)` is an AFFINE flow (every coupling's last layer is zero), so the prior is a
Gaussian N(m, S); netG(z) = A z with A = diag(a), a log-spaced from 0.3 to 3.0, sigma = 1 and x = A t, so the likelihood's energy is
E(z) = 1/2 |A (z - t)|^2 and
    log Z = log int p(z) exp(-E(z)) dz = -1/2 log det(I + S L) - 1/2 (m - t)^T L (I + S L)^-1 (m - t),   L = A^T A
(`closed_form`; m and S are read off the oracle's forward on the basis vectors).  log p(x) = log Z - D / 2 log(2 pi sigma^2).

The estimator: B = N * chains rows, row n * chains + c chain c of datum n, start from exact prior draws, beta_0 = 0 .. beta_T = 1; the
init call weighs the start and anneals to beta_1, end call t < T anneals to beta_{t+1}, end call T does not;
log Z_hat = logsumexp_c(log_w) - log(chains).  `experiment`: the run of the CPU and GPU sampler tests, stated once."""
import math

import torch

from oracle import flow_oracle as O
import hmc_metric_restated as MR
import hmc_tempered_restated as TR

GEO = (8, 4, 5, 1)
EXP_T, EXP_L, EXP_CHAINS, EXP_STEP, EXP_DATA = 100, 3, 64, 0.28, (21, 22)


def schedule(T, kind="sigmoid", delta=4.0):
    """langevin.ais_schedule, restated: beta_t = (sigma(delta (2 t / T - 1)) - sigma(-delta)) / (sigma(delta) - sigma(-delta))."""
    t = torch.arange(T + 1, dtype=torch.float64) / T
    if kind == "linear":
        return t
    sg = lambda v: 1.0 / (1.0 + torch.exp(-v))
    lo, hi = sg(torch.tensor(-delta, dtype=torch.float64)), sg(torch.tensor(delta, dtype=torch.float64))
    b = (sg(delta * (2.0 * t - 1.0)) - lo) / (hi - lo)
    b[0], b[-1] = 0.0, 1.0
    return b


def affine_flow():
    return O.init_params(GEO[0], GEO[1], GEO[2], seed=3, fcz_std=0.0)


def datum(seed):
    """The axis-aligned quadratic energy of the datum x = A t, t = randn(8, seed): hmc_metric_restated.Diagonal with a in 0.3 .. 3.0."""
    return MR.Diagonal(GEO[0], lo=0.3, hi=3.0, seed=seed)


def prior_gaussian(p):
    """(W, b, m, S) of the affine flow eps = f(z) = z W^T + b, from the oracle's forward on 0 and the basis vectors (and a check that it
    IS affine on a random point): the prior of z is N(m, S), m = -W^-1 b, S = W^-1 W^-T."""
    f64 = torch.float64
    nz = GEO[0]
    q = O.to_dtype(p, f64)
    fwd = lambda z: O.flow_forward(q, z, torch.zeros(z.shape[0], dtype=f64))[0].detach()
    b = fwd(torch.zeros(1, nz, dtype=f64))[0]
    W = (fwd(torch.eye(nz, dtype=f64)) - b).T                # column i = f(e_i) - f(0)
    z = torch.randn(3, nz, generator=torch.Generator().manual_seed(1), dtype=f64)
    assert bool(((fwd(z) - (z @ W.T + b)).abs() <= 1e-12).all()), "the flow is not affine"
    Wi = torch.linalg.inv(W)
    return W, b, -(Wi @ b), Wi @ Wi.T


def closed_form(p, quad):
    """log int p(z) exp(-1/2 |A (z - t)|^2) dz for the Gaussian prior of the affine flow p."""
    _, _, m, S = prior_gaussian(p)
    Lm = quad.A.T @ quad.A
    M = torch.eye(GEO[0], dtype=torch.float64) + S @ Lm
    d = m - quad.t
    return (-0.5 * torch.linalg.slogdet(M)[1] - 0.5 * d @ (Lm @ torch.linalg.solve(M, d))).item()


class Stacked:
    """The energies of N data, `chains` rows each: row n * chains + c belongs to datum n."""

    def __init__(self, quads, chains):
        self.a = torch.stack([q.a for q in quads]).repeat_interleave(chains, 0)
        self.t = torch.stack([q.t for q in quads]).repeat_interleave(chains, 0)

    def __call__(self, z):
        a, t = self.a.to(z.dtype), self.t.to(z.dtype)
        r = (z - t) * a
        return 0.5 * (r * r).sum(1), r * a


def reduce(log_w, chains):
    """(log Z_hat (N), ess (N)) of the rows' log weights (N * chains)."""
    lw = log_w.double().view(-1, chains)
    lse = torch.logsumexp(lw, 1)
    return lse - math.log(chains), torch.exp(2.0 * lse - torch.logsumexp(2.0 * lw, 1))


def prior_draws(p, space, B, g):
    """(start of the chain in `space`, eps) of B exact draws of the prior from the generator g."""
    eps = torch.randn(B, GEO[0], generator=g, dtype=torch.float64)
    if space == "eps":
        return eps, eps
    q = O.to_dtype(p, torch.float64)
    return O.flow_reverse(q, eps, torch.zeros(B, dtype=torch.float64))[0].detach(), eps


def run(p, quads, space, betas, L, chains, step, seed):
    """One float64 AIS run: (log Z_hat (N), ess (N), the mean acceptance, the trace)."""
    f64 = torch.float64
    T, B, nz = betas.numel() - 1, len(quads) * chains, GEO[0]
    g = torch.Generator().manual_seed(5000 + seed)
    x0, _ = prior_draws(p, space, B, g)
    noises = [torch.randn(B, nz, generator=g, dtype=f64) for _ in range(T)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g, dtype=f64).clamp_min(2.0 ** -25) for _ in range(T)]
    rows = lambda t: torch.full((B,), float(betas[t]), dtype=f64)
    anneals = [rows(t + 1) for t in range(T)] + [None]      # the init call anneals to beta_1, end call t < T to beta_{t+1}, end call T does not
    tr = TR.chain(TR.flow_parts(space, p, Stacked(quads, chains)), x0, torch.full((B,), step, dtype=f64), torch.ones(B, nz, dtype=f64), L,
                  noises, uniforms, rows(0), anneals)
    logz, ess = reduce(tr.log_w[0] - tr.log_w[1], chains)
    return logz, ess, tr.acc.double().mean().item(), tr


def experiment(seed, space, T=EXP_T, L=EXP_L, chains=EXP_CHAINS, step=EXP_STEP, data=EXP_DATA):
    """The experiment at one seed: (errors log Z_hat - closed form (N), ess (N), mean acceptance)."""
    p = affine_flow()
    quads = [datum(s) for s in data]
    logz, ess, acc, _ = run(p, quads, space, schedule(T), L, chains, step, seed)
    exact = torch.tensor([closed_form(p, q) for q in quads], dtype=torch.float64)
    return logz - exact, ess, acc


# The figures over seeds 0 .. 7 (profiles/ais_cpu.txt has every seed's figures and the arithmetic; tests/test_hmc_tempered_cpu.py states
# the bands again and holds these constants to them).  error: log Z_hat - closed form of a datum, the observed range over the 16
# estimates widened by 3 standard deviations of them; ess likewise; accept: the range of the 8 runs widened by 3 SE of one run's
# T x 128 decisions.
BAND = {
    "z": {"error": (-0.863, 0.797), "ess": (9.1, 55.3), "accept": (0.954, 0.971)},
    "eps": {"error": (-0.642, 0.582), "ess": (18.1, 54.2), "accept": (0.888, 0.912)},
}

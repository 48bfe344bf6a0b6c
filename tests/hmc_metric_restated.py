"""TEST INFRASTRUCTURE (CPU; float64 and float32): the per-row diagonal metric of `lsnf_hmc_step_metric` /
`lsnf_reverse_hmc_step_metric` (include/lsnf_flow_mcmc.h) and its windowed estimation, restated on tests/hmc_rows_restated.py.

Row b has a scale per column, sd[b, c]; the chain is HMC with identity mass in y = z / sd (s the row's step, hs = s / 2):
    begin   kin0 = 1/2 sum xi^2;  qh = xi  - hs (sd g_s);  z_1     = z_s + s (sd qh)
    inner   at z_i:               qh = qh  - s  (sd g);    z_{i+1} = z_i + s (sd qh)
    end     at z_L:               qL = qh  - hs (sd g);    kinL = 1/2 sum qL^2;  log_alpha, accept: the per-row chain's
    fold    n = count + 1;  d = x - mean;  mean' = mean + d / n;  m2' = m2 + d (x - mean')        (x: the state after the decision)
    close   n >= 2:  v = (n / (n + n0)) (m2' / (n - 1)) + var0 (n0 / (n + n0));  sd' = clamp(sqrt v, scale_min, scale_max);  n < 2: sd' = sd
            mean = m2 = count = 0;  with "update": the dual-averaging state restarts as {0, 0, 0, log(10 s')}

`begin` / `inner` / `end`: those lines on tensors of any dtype (fp32: every operation a torch fp32 operation, the products sd g and
sd qh formed first).  `fold` / `close`: the window's arithmetic likewise.  `chain`: the float64 chain over any potential
`pot(x) -> (U, grad U, ...)`, with steps, adaptation modes and window modes per end call.  `experiment`: the warm-up experiment of the
CPU and GPU sampler tests, stated once."""
import math
from dataclasses import dataclass

import torch

from oracle import flow_oracle as O
import hmc_restated as H
import hmc_rows_restated as R


@dataclass
class Reg:
    """include/lsnf_flow_mcmc.h LsnfMetricReg, with `flow.HmcRowMetric`'s defaults."""
    n0: float = 5.0
    var0: float = 1e-3
    scale_min: float = 1e-3
    scale_max: float = 1e3


def begin(x_s, g_s, xi, s, sd):
    """(qh, x_1, kin0) in the tensors' dtype; s (B, 1) or a float, sd (B, nz)."""
    xi = xi.to(x_s.dtype)
    qh = xi - (0.5 * s) * (sd * g_s)
    return qh, x_s + s * (sd * qh), 0.5 * (xi * xi).sum(1)


def inner(x, mom, g, s, sd):
    qh = mom - s * (sd * g)
    return qh, x + s * (sd * qh)


def end(mom, g_prop, s, sd):
    ql = mom - (0.5 * s) * (sd * g_prop)
    return ql, 0.5 * (ql * ql).sum(1)


def fold(mean, m2, count, x):
    """(mean', m2', count') of one fold of the rows x, every operation in the tensors' dtype; count (B)."""
    n = count + 1.0
    d = x - mean
    mean2 = mean + d / n[:, None]
    return mean2, m2 + d * (x - mean2), n


def close(sd, m2, n, reg, dtype=torch.float64):
    """sd' (B, nz) from the folded m2 and the rows' counts n (B), in `dtype`; the constants are the fp32 values the kernel is given."""
    c = lambda v: torch.tensor(float(torch.tensor(v, dtype=torch.float32)), dtype=dtype)
    sd, m2, n = sd.to(dtype), m2.to(dtype), n.to(dtype)[:, None]
    n0, var0 = c(reg.n0), c(reg.var0)
    v = (n / (n + n0)) * (m2 / (n - 1.0)) + var0 * (n0 / (n + n0))
    new = torch.sqrt(v).clamp(float(c(reg.scale_min)), float(c(reg.scale_max)))
    return torch.where(n >= 2.0, new, sd)


def restart(step, dtype=torch.float64):
    """The dual-averaging state a close leaves with "update": {0, 0, 0, log(10 s')} (B, 4)."""
    ad = torch.zeros(step.shape[0], 4, dtype=dtype)
    ad[:, 3] = torch.log(torch.tensor(10.0, dtype=dtype) * step.to(dtype))
    return ad


class Trace:
    """What `chain` returns: la / acc (K, B) of the end calls, steps (K + 1, B) as hmc_rows_restated.Trace's, states (K, B, nz) the
    state after every decision, scale / mean / m2 / count and adapt as the last end call left them, the final state (x, grad, U)."""


def chain(pot, x0, step, sd, L, noises, uniforms, da=None, modes=None, windows=None, reg=None, adapt=None):
    """The float64 chain from x0 (B, nz) on the potential `pot`: K = len(noises) - 1 trajectories of L steps, noises[t] starting
    trajectory t + 1, uniforms[t] deciding trajectory t, row b at step[b] and scale sd[b].  modes[k - 1] in (None, "update", "last"),
    windows[k - 1] in (None, "fold", "close"): what end call k does to the rows' steps and windows.  The decision of a trajectory is
    made with the step and scale it ran at; fold, close and the step update come after it and before the next momentum is used."""
    f64 = torch.float64
    K, B = len(noises) - 1, x0.shape[0]
    modes = [None] * K if modes is None else modes
    windows = [None] * K if windows is None else windows
    reg = Reg() if reg is None else reg
    s = step.to(f64).reshape(B, 1).clone()
    sd = sd.to(f64).clone()
    ad = R.new_adapt(s[:, 0]) if adapt is None else adapt.to(f64).clone()
    mean, m2, count = torch.zeros_like(sd), torch.zeros_like(sd), torch.zeros(B, dtype=f64)
    x_acc = x0.to(f64)
    u_acc, g_acc = pot(x_acc)[:2]
    out = Trace()
    out.la, out.acc, out.steps, out.states = [], [], [s[:, 0].clone()], []
    for k in range(1, K + 1):
        qh, x, kin0 = begin(x_acc, g_acc, noises[k - 1].to(f64), s, sd)
        for i in range(1, L):
            qh, x = inner(x, qh, pot(x)[1], s, sd)
        U_prop, g_prop = pot(x)[:2]
        _, kinL = end(qh, g_prop, s, sd)
        la = H.log_alpha(u_acc, U_prop, kin0, kinL)
        acc = H.accept(la, uniforms[k])
        a = acc[:, None]
        x_acc, g_acc, u_acc = torch.where(a, x, x_acc), torch.where(a, g_prop, g_acc), torch.where(acc, U_prop, u_acc)
        if modes[k - 1] is not None:
            ad, s_new = R.dual_average(ad, la, da, modes[k - 1] == "last")
            s = s_new.reshape(B, 1)
        if windows[k - 1] is not None:
            mean, m2, count = fold(mean, m2, count, x_acc)
            if windows[k - 1] == "close":
                sd = close(sd, m2, count, reg)
                mean, m2, count = torch.zeros_like(mean), torch.zeros_like(m2), torch.zeros_like(count)
                if modes[k - 1] == "update":
                    ad = restart(s[:, 0])
        out.la.append(la); out.acc.append(acc); out.steps.append(s[:, 0].clone()); out.states.append(x_acc.clone())
    out.la, out.acc, out.steps, out.states = torch.stack(out.la), torch.stack(out.acc), torch.stack(out.steps), torch.stack(out.states)
    out.scale, out.mean, out.m2, out.count, out.adapt, out.state = sd, mean, m2, count, ad, (x_acc, g_acc, u_acc)
    return out


def flow_potential(space, p, quad):
    """`pot` of the flow prior plus the energy `quad`, on z or on eps (hmc_rows_restated.potential)."""
    return lambda x: R.potential(space, p, x, quad)


def schedule(W, frozen, first, closes):
    """(modes, windows) of W warm-up and `frozen` frozen end calls with the windows (first, closes) of `langevin.warmup_windows`: the
    step adapts on every warm-up end call ("last" on the W-th), end calls first .. the last close fold, the closes close."""
    modes = ["update"] * (W - 1) + ["last"] + [None] * frozen
    last = closes[-1] if closes else 0
    windows = [None if not closes or t < first or t > last else "close" if t in closes else "fold" for t in range(1, W + frozen + 1)]
    return modes, windows


# ---- the warm-up experiment of tests/test_hmc_metric_cpu.py and of the GPU sampler tests, stated once -------------------------------
EXP_GEO = (8, 4, 5, 1)                       # tests/test_gpu_reverse_keep.py TINY
EXP_B, EXP_L, EXP_W, EXP_FROZEN, EXP_S0 = 64, 3, 300, 60, 0.3
EXP_WINDOWS = (76, [100, 150, 250])          # langevin.warmup_windows(300)


class Diagonal:
    """e(z) = 1/2 sum_c a_c^2 (z_c - t_c)^2, a log-spaced from 0.3 to 30: hmc_restated.Quadratic with A = diag(a)."""

    def __init__(self, nz, lo=0.3, hi=30.0, seed=21):
        self.a = torch.logspace(math.log10(lo), math.log10(hi), nz, dtype=torch.float64)
        self.A = torch.diag(self.a)
        self.t = torch.randn(nz, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)

    def __call__(self, z):
        a, t = self.a.to(z.dtype), self.t.to(z.dtype)
        r = (z - t) * a
        return 0.5 * (r * r).sum(1), r * a


def experiment_target():
    """(p, quad) of the experiment: the TINY flow of O.init_params(8, 4, 5, seed=3) and the axis-aligned quadratic energy."""
    nz, w, depth, _ = EXP_GEO
    return O.init_params(nz, w, depth, seed=3), Diagonal(nz)


def closed_form(quad):
    """(1 + a^2)^-1/2 per column: the posterior's standard deviation under a unit-normal prior, the figure a scale is compared with."""
    return 1.0 / torch.sqrt(1.0 + quad.a * quad.a)


def experiment_start(space, seed, B=EXP_B):
    """The rows' start of the run at `seed`: O.smooth_batch's rows in z, unit-normal rows in eps."""
    p, _ = experiment_target()
    if space == "eps":
        return torch.randn(B, EXP_GEO[0], generator=torch.Generator().manual_seed(2000 + seed), dtype=torch.float64)
    return O.smooth_batch(p, B, EXP_GEO[0], seed=2000 + seed)[0].double()


def figures(acc, step, scale, quad):
    """(frozen mean acceptance, frozen median step, median |log(scale / closed form)|) of a run."""
    dev = (torch.log(scale.double().cpu()) - torch.log(closed_form(quad))[None, :]).abs()
    return acc.double().mean().item(), step.double().median().item(), dev.median().item()


def experiment(seed, space="z", metric=True, B=EXP_B, W=EXP_W, frozen=EXP_FROZEN, L=EXP_L, windows=EXP_WINDOWS):
    """The experiment in float64 at one seed: `figures` of the run, with the windowed metric or (metric=False) the step adaptation
    alone, and the lag-1 autocorrelation of the softest coordinate over the frozen states."""
    nz = EXP_GEO[0]
    p, quad = experiment_target()
    g = torch.Generator().manual_seed(1000 + seed)
    T = W + frozen
    noises = [torch.randn(B, nz, generator=g, dtype=torch.float64) for _ in range(T)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g, dtype=torch.float64).clamp_min(2.0 ** -25) for _ in range(T)]
    modes, wins = schedule(W, frozen, *(windows if metric else (None, [])))
    tr = chain(flow_potential(space, p, quad), experiment_start(space, seed, B), torch.full((B,), EXP_S0, dtype=torch.float64),
               torch.ones(B, nz, dtype=torch.float64), L, noises, uniforms, da=R.DualAvg(), modes=modes, windows=wins)
    x = tr.states[W:, :, 0]                                  # the softest coordinate (a = 0.3)
    xc = x - x.mean(0, keepdim=True)
    rho = ((xc[1:] * xc[:-1]).sum(0) / (xc * xc).sum(0).clamp_min(1e-300)).mean().item()
    return figures(tr.acc[W:], tr.steps[-1], tr.scale, quad) + (rho, tr)


# The figures of the frozen phase over the B rows, float64 restatement, seeds 0 .. 7, each band the observed range widened by 3 standard
# errors of one run (profiles/hmc_metric_cpu.txt has every seed's figures and the arithmetic; tests/test_hmc_metric_cpu.py states the
# bands again and holds these constants to them).
BAND = {
    "z": {"accept": (0.871, 0.925), "step": (0.646, 0.739), "scale": (0.093, 0.127)},
    "eps": {"accept": (0.963, 0.984), "step": (0.115, 0.168), "scale": (1.095, 1.338)},
}

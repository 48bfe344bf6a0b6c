"""TEST INFRASTRUCTURE (CPU; float64 and float32): the per-row step sizes of `lsnf_hmc_step_rows` / `lsnf_reverse_hmc_step_rows`
(include/lsnf_flow_mcmc.h) and their dual-averaging adaptation, restated on tests/hmc_restated.py.

    a    = min(1, exp(log_alpha))  (a NaN log_alpha: 0)
    t    = count + 1;  eta = 1 / (t + t0)
    hbar = (1 - eta) hbar + eta (target_accept - a)
    ls   = clamp(mu - (sqrt(t) / gamma) hbar, log step_min, log step_max)
    w    = t^-kappa;  lsb = w ls + (1 - w) lsb
    s'   = exp(last ? lsb : ls)

`dual_average`: that update on tensors, in float64 or in float32 (every operation a torch fp32 operation: the fp32 restatement whose
own error widens a GPU bound).  `chain`: the float64 chain of tests/hmc_restated.py with the step a (B, 1) tensor -- `begin`, `inner`
and `end` there broadcast it -- and its own kink redraw: `hmc_restated.smooth_trajectory` takes the bad rows' state and noise but would
keep every row's step.  With space="eps" the same for the base-space chain of tests/rhmc_restated.py."""
import math
from dataclasses import dataclass

import torch

from oracle import flow_oracle as O
import hmc_restated as H


@dataclass
class DualAvg:
    """include/lsnf_flow_mcmc.h LsnfDualAvg, with `flow.new_hmc_row_steps`' defaults."""
    target_accept: float = 0.8
    gamma: float = 0.05
    t0: float = 10.0
    kappa: float = 0.75
    step_min: float = 1e-4
    step_max: float = 1e2


def new_adapt(step, dtype=torch.float64):
    """The (B, 4) state {log_step_bar, hbar, count, mu} of fresh rows at `step` (B): mu = log(10 step)."""
    ad = torch.zeros(step.shape[0], 4, dtype=dtype)
    ad[:, 3] = torch.log(10.0 * step.to(dtype))
    return ad


def dual_average(ad, la, da, last, dtype=torch.float64):
    """(the new (B, 4) state, the new step (B)) from the state `ad` and the rows' log_alpha `la`, every operation in `dtype`.  The
    constants are the fp32 values the kernel is given (the two logs: of the fp32 step_min / step_max, taken in float64 and rounded
    to fp32 as the host's logf leaves them to within its last bit)."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    c = lambda v: torch.tensor(v, dtype=dtype)
    ad, la = ad.to(dtype), la.to(dtype)
    lo, hi = (f32(math.log(f32(v))) if dtype == torch.float32 else math.log(f32(v)) for v in (da.step_min, da.step_max))
    a = torch.where(torch.isnan(la), torch.zeros_like(la), torch.exp(la).clamp_max(1.0))
    t = ad[:, 2] + 1.0
    eta = 1.0 / (t + c(f32(da.t0)))
    hbar = (1.0 - eta) * ad[:, 1] + eta * (c(f32(da.target_accept)) - a)
    ls = (ad[:, 3] - (torch.sqrt(t) / c(f32(da.gamma))) * hbar).clamp(lo, hi)
    w = torch.pow(t, c(-f32(da.kappa)))
    lsb = w * ls + (1.0 - w) * ad[:, 0]
    return torch.stack([lsb, hbar, t, ad[:, 3]], 1), torch.exp(lsb if last else ls)


def update_scale(ad, da):
    """1 + |mu| + (sqrt(t) / gamma) |hbar| per row, of the state AFTER an update: the magnitudes the new log step is formed from."""
    ad = ad.double()
    return 1.0 + ad[:, 3].abs() + (torch.sqrt(ad[:, 2]) / da.gamma) * ad[:, 1].abs()


SPACES = ("z", "eps")                        # lsnf_hmc_step_rows' chain on z; lsnf_reverse_hmc_step_rows' on eps with x = f^-1(eps)


def potential(space, p, point, quad):
    """(U, grad U, ...) in float64 at the rows `point`: hmc_restated.potential, or rhmc_restated's (whose fifth entry is x)."""
    if space == "z":
        return H.potential(p, point, quad, torch.float64)
    import rhmc_restated as RH
    return RH.potential(p, point, quad, torch.float64)


def trajectory(space, p, quad, x_s, g_s, xi, s, L):
    """`hmc_restated.trajectory` / `rhmc_restated.trajectory` with s (B, 1): z[i] the points (of either space), pot[i], ph[i], kin0."""
    t = H.Trajectory()
    ph, x1, t.kin0 = H.begin(x_s, g_s, xi.to(torch.float64), s)
    t.z, t.ph, t.pot = [None, x1], [ph], [None]
    for i in range(1, L + 1):
        t.pot.append(potential(space, p, t.z[i], quad))
        if i < L:
            ph, xn = H.inner(t.z[i], t.ph[i - 1], t.pot[i][1], s)
            t.ph.append(ph)
            t.z.append(xn)
    return t


def smooth_trajectory(space, p, quad, z_s, g_s, noise, s, L, redraw, margin=2e-5, max_rounds=100):
    """`hmc_restated.smooth_trajectory` (`rhmc_restated`'s: the kink is looked for at x) with s (B, 1): a redrawn row keeps its own step."""
    t = trajectory(space, p, quad, z_s, g_s, noise, s, L)
    if redraw is None:
        return t

    def near(tr):
        at = [z.float() for z in tr.z[1:]] if space == "z" else [pot[4] for pot in tr.pot[1:]]
        return torch.stack([O.relu_margin(p, x) <= margin for x in at]).any(0)
    bad = torch.nonzero(near(t)).flatten()
    for _ in range(max_rounds):
        if bad.numel() == 0:
            return t
        noise[bad] = torch.randn(int(bad.numel()), noise.shape[1], generator=redraw, dtype=noise.dtype)
        sub = trajectory(space, p, quad, z_s[bad], g_s[bad], noise[bad], s[bad], L)
        t.kin0[bad] = sub.kin0
        for i in range(1, L + 1):
            t.z[i][bad] = sub.z[i]
            for a, b in zip(t.pot[i], sub.pot[i]):
                a[bad] = b
        for i in range(L):
            t.ph[i][bad] = sub.ph[i]
        bad = bad[near(sub)]
    raise RuntimeError(f"smooth_trajectory: {bad.numel()} trajectories still within {margin} of a ReLU kink after {max_rounds} redraws")


class Trace:
    """What `chain` returns: la / acc (K, B) of the end calls, steps (K + 1, B): steps[k] ran trajectory k + 1 (the last: what the
    last end call left), adapt (B, 4), the final state (z, grad, U)."""


def chain(p, z0, quad, step, L, noises, uniforms, redraw=None, da=None, modes=None, adapt=None, space="z"):
    """The float64 chain of `hmc_restated.chain` -- K = len(noises) - 1 trajectories of L steps, noises[t] starting trajectory t + 1,
    uniforms[t] deciding trajectory t -- with a step per row: `step` (B).  modes[k - 1] in (None, "update", "last") says what end
    call k does to the rows' steps (None everywhere by default: no adaptation), with the constants `da` and the state `adapt`
    (fresh by default).  The decision of a trajectory is made with the step it ran at; the update comes after it and before the next
    momentum is used.  space "eps": `rhmc_restated.chain`'s chain instead (z0 is then eps0)."""
    f64 = torch.float64
    K, B = len(noises) - 1, z0.shape[0]
    modes = [None] * K if modes is None else modes
    s = step.to(f64).reshape(B, 1).clone()
    ad = new_adapt(s[:, 0]) if adapt is None else adapt.to(f64).clone()
    z_acc = z0.to(f64)
    u_acc, g_acc = potential(space, p, z_acc, quad)[:2]
    tr = smooth_trajectory(space, p, quad, z_acc, g_acc, noises[0], s, L, redraw)
    out = Trace()
    out.la, out.acc, out.steps = [], [], [s[:, 0].clone()]
    for k in range(1, K + 1):
        U_prop, g_prop = tr.pot[L][0], tr.pot[L][1]
        _, kinL = H.end(tr.ph[L - 1], g_prop, s)
        la = H.log_alpha(u_acc, U_prop, tr.kin0, kinL)
        acc = H.accept(la, uniforms[k])
        a = acc[:, None]
        z_acc, g_acc, u_acc = torch.where(a, tr.z[L], z_acc), torch.where(a, g_prop, g_acc), torch.where(acc, U_prop, u_acc)
        if modes[k - 1] is not None:
            ad, s_new = dual_average(ad, la, da, modes[k - 1] == "last")
            s = s_new.reshape(B, 1)
        out.la.append(la); out.acc.append(acc); out.steps.append(s[:, 0].clone())
        if noises[k] is not None:
            tr = smooth_trajectory(space, p, quad, z_acc, g_acc, noises[k], s, L, redraw)
    out.la, out.acc, out.steps = torch.stack(out.la), torch.stack(out.acc), torch.stack(out.steps)
    out.adapt, out.state = ad, (z_acc, g_acc, u_acc)
    return out


# ---- the warm-up experiment of tests/test_hmc_rows_cpu.py and of the GPU sampler tests: one configuration per space, stated once ----
WARMUP_GEO = (8, 4, 5, 1)                    # tests/test_gpu_reverse_keep.py TINY
WARMUP_B, WARMUP_L, WARMUP_K, FROZEN_K = 64, 3, 60, 60
SOUND_STEP = {"z": 1.2, "eps": 1.13}         # tests/test_gpu_hmc.py STEP[8], tests/test_gpu_rhmc.py STEP_GEO[TINY]; L = 3
QUAD_SCALE, QUAD_SEED = 0.1, 7 + 8           # the quadratic of both files at nz = 8
# The mean acceptance of the FROZEN_K frozen trajectories over the B rows (half started at 10 x, half at 0.1 x SOUND_STEP), float64
# restatement, seeds 0 .. 7, widened by 3 standard errors of one run (profiles/hmc_rows_cpu.txt has every seed's figure and the
# arithmetic; tests/test_hmc_rows_cpu.py states it again and holds these constants to it).
BAND = {"z": (0.912, 0.946), "eps": (0.872, 0.915)}
BAND_HALF = {"z": (0.900, 0.957), "eps": (0.863, 0.925)}     # a half of the rows: those started at 10 x, those at 0.1 x


def warmup_start(space, B=WARMUP_B):
    """The rows' first steps: the even rows at 10 x, the odd rows at 0.1 x the sound step."""
    s = SOUND_STEP[space]
    return torch.where(torch.arange(B) % 2 == 0, torch.tensor(10.0 * s), torch.tensor(0.1 * s)).double()


def warmup_target(space="z"):
    """(p, quad) of the experiment: the TINY flow and the quadratic energy."""
    nz, w, depth, _ = WARMUP_GEO
    return O.init_params(nz, w, depth, seed=3), H.Quadratic(nz, QUAD_SCALE, seed=QUAD_SEED)


def warmup_run(seed, space="z", B=WARMUP_B, K=WARMUP_K, frozen=FROZEN_K, L=WARMUP_L, da=None):
    """The experiment in float64 at one seed: (frozen-phase mean acceptance, frozen-phase acceptance of the two halves, the frozen steps)."""
    nz = WARMUP_GEO[0]
    p, quad = warmup_target(space)
    g = torch.Generator().manual_seed(1000 + seed)
    z0, _ = O.smooth_batch(p, B, nz, seed=2000 + seed)
    if space == "eps":
        z0 = torch.randn(B, nz, generator=g, dtype=torch.float64)
    T = K + frozen
    noises = [torch.randn(B, nz, generator=g, dtype=torch.float64) for _ in range(T)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g, dtype=torch.float64).clamp_min(2.0 ** -25) for _ in range(T)]
    modes = ["update"] * (K - 1) + ["last"] + [None] * frozen
    tr = chain(p, z0, quad, warmup_start(space, B), L, noises, uniforms, redraw=None, da=da or DualAvg(), modes=modes, space=space)
    acc = tr.acc[K:].double()
    return acc.mean().item(), (acc[:, 0::2].mean().item(), acc[:, 1::2].mean().item()), tr.steps[-1]

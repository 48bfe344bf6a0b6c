"""TEST INFRASTRUCTURE (CPU; float64 and float32): the schedule search of `lsnf_hmc_step_schedule` / `lsnf_reverse_hmc_step_schedule`
(include/lsnf_flow_mcmc.h), restated on tests/hmc_resample_restated.py and tests/hmc_tempered_restated.py.

Rows [k P, (k + 1) P) are the particles of group k.  On an annealing call with LSNF_HMC_SCHEDULE, with {w_i, c_i} the rows' Kahan
pairs BEFORE the increment, el_i the likelihood energy of their states after the decision, and `tree` the xor-butterfly over the rungs:
    b = beta_rows[rung 0];  cap = beta_next[rung 0];  D = cap - b
    l_i = w_i - c_i;  m = tree fmax l_i;  W_i = exp(l_i - m);  S0 = tree + W_i;  emin = tree fmin el_i;  r_i = el_i - emin
    cess(x) = (N1 * N1) / (N2 * S0),  N1 = tree + W_i v_i,  N2 = tree + (W_i v_i) v_i,  v_i = exp(-(x * r_i))
    !(D > 0): beta' = b;   cess(D) >= frac: beta' = cap;   else twelve halvings of [0, D], delta = fmax(lo, min_step),
    beta' = fmin(b + delta, cap)
`search`: those lines on tensors of any dtype (fp32: every operation a torch fp32 operation in the header's order); `cess64` / `root64`:
the exact function and the float64 root of cess64(delta) = frac; `monotone`: the condition on a test's inputs; `slack`: the bound s of
the fp32 search; `adaptive_chain`: the float64 sampler over any `parts(x) -> Parts`; `run` / `experiment` / BAND: the closed-form
problem of tests/ais_restated.py.

THE BOUND.  In exact arithmetic twelve halvings of [0, D] end with lo <= delta* < lo + h, h = D 2^-12, so delta - delta* lies in
(-h, 0].  In fp32 a comparison cess(mid) >= frac can come out wrong only where |cess64(mid) - frac| <= eps_c frac, eps_c the relative
error of the fp32 cess, i.e. where |mid - delta*| <= eps_c frac / |slope|, slope the slope of cess64 at the root (taken as the
smaller of the two secants over one final bracket on either side of the root).  The fp32 result is therefore within
    -(1 + s) h <= delta32 - delta* <= s h,      s = eps_c frac / (|slope| h) + 2^-24 (|b| + |beta'|) / h
(the second term: the rounding of b + delta, which is how delta32 is read back from beta_rows).  eps_c from the operation sequence,
u = 2^-24, E = EXP_ULP (the device's expf, hmc_resample_restated), lmax >= max |l_i|, amax >= D max r_i, L = log2 P:
    W_i: the roundings of l_i, m and l_i - m move the argument by <= 4 u lmax, expf by E ulps = 2 E u:       eW = u (4 lmax + 2 E)
    v_i: the roundings of r_i and x r_i move the argument by <= 2 u amax, expf by 2 E u:                       ev = u (2 amax + 2 E)
    t_i = W_i v_i: eW + ev + u;   q_i = t_i v_i: eW + 2 ev + 2 u;   a tree sum adds L u
    cess = (N1 N1) / (N2 S0): 2 (eW + ev + u + L u) + (eW + 2 ev + 2 u + L u) + (eW + L u) + 3 u
    eps_c = 1.01 u (16 lmax + 8 amax + 16 E + 4 L + 7)                                          (1 %: the second-order terms)
Nothing of this is fitted to a device."""
import math
import types

import torch

import hmc_resample_restated as R

GROUPS = R.GROUPS
HALVINGS = 12
U32 = R.U32


def _tree(x, op):
    """The xor-butterfly over the last dimension (P a power of two): every entry of a group ends with the same bits."""
    P = x.shape[1]
    k = torch.arange(P, device=x.device)
    s = 1
    while s < P:
        x = op(x, x[:, k ^ s])
        s <<= 1
    return x


def _parts(l, el, P):
    L, E = l.view(-1, P), el.view(-1, P)
    m = _tree(L, torch.fmax)
    W = torch.exp(L - m)
    S0 = _tree(W, torch.add)
    emin = _tree(E, torch.fmin)
    return W, E - emin, S0


def _cess(x, W, r, S0):
    a = x * r
    v = torch.exp(-a)
    t = W * v
    q = t * v
    N1, N2 = _tree(t, torch.add), _tree(q, torch.add)
    return (N1 * N1) / (N2 * S0)


def search(b, cap, l, el, P, cess_frac, min_step):
    """beta' (B) of every row in l's dtype.  b, cap, l, el (B): beta_rows, beta_next, the log weights w - c before the increment, el_s.
    Returns beta (B), searching (G) bool (the group ran the halvings' result), whole (G) bool (it reached its ceiling in one step), idle
    (G) bool (!(D > 0)), lo (G)."""
    assert P in GROUPS and l.shape[0] % P == 0
    dt = l.dtype
    frac, ms = torch.tensor(cess_frac, dtype=dt), torch.tensor(min_step, dtype=dt)
    b0 = b.to(dt).view(-1, P)[:, :1].expand(-1, P)
    c0 = cap.to(dt).view(-1, P)[:, :1].expand(-1, P)
    D = c0 - b0
    W, r, S0 = _parts(l, el.to(dt), P)
    whole = _cess(D, W, r, S0) >= frac
    lo, hi = torch.zeros_like(D), D.clone()
    half = torch.tensor(0.5, dtype=dt)
    for _ in range(HALVINGS):
        mid = half * (lo + hi)
        ok = _cess(mid, W, r, S0) >= frac
        lo, hi = torch.where(ok, mid, lo), torch.where(ok, hi, mid)
    delta = torch.fmax(lo, ms)
    stepped = torch.fmin(b0 + delta, c0)
    idle = ~(D > 0)
    beta = torch.where(idle, b0, torch.where(whole, c0, stepped))
    return types.SimpleNamespace(beta=beta.reshape(-1), searching=(~idle & ~whole)[:, 0], whole=(~idle & whole)[:, 0], idle=idle[:, 0],
                                 lo=lo[:, 0])


def cess64(delta, l, el, P):
    """cess (G) of the groups at the steps delta (G), float64, with plain sums (the exact function up to float64 rounding)."""
    L, E = l.double().view(-1, P), el.double().view(-1, P)
    W = torch.exp(L - L.max(dim=1, keepdim=True).values)
    v = torch.exp(-delta.double()[:, None] * (E - E.min(dim=1, keepdim=True).values))
    t = W * v
    return t.sum(1) ** 2 / ((t * v).sum(1) * W.sum(1))


def root64(D, l, el, P, cess_frac, iters=80):
    """delta* (G) in [0, D] with cess64(delta*) = cess_frac, by float64 bisection (for groups with cess64(D) < cess_frac <= 1)."""
    lo, hi = torch.zeros_like(D, dtype=torch.float64), D.double().clone()
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        ok = cess64(mid, l, el, P) >= cess_frac
        lo, hi = torch.where(ok, mid, lo), torch.where(ok, hi, mid)
    return 0.5 * (lo + hi)


def monotone(D, l, el, P, points=513):
    """(G) bool: cess64 does not rise along a grid of `points` steps over [0, D] -- a condition on a test's inputs."""
    prev, ok = None, torch.ones(D.shape[0], dtype=torch.bool)
    for i in range(points):
        c = cess64(D.double() * (i / (points - 1)), l, el, P)
        if prev is not None:
            ok &= c <= prev * (1.0 + 1e-13)
        prev = c
    return ok


def eps_c(P, lmax, amax):
    """The relative error of the fp32 cess (module docstring)."""
    return 1.01 * U32 * (16.0 * lmax + 8.0 * amax + 16.0 * R.EXP_ULP + 4.0 * math.log2(P) + 7.0)


def slack(D, b, l, el, P, cess_frac, root):
    """s (G) of the module docstring's bound for searching groups, D, b (G) and root = root64(..)."""
    L, E = l.double().view(-1, P), el.double().view(-1, P)
    h = D.double() * 2.0 ** -HALVINGS
    lmax = L.abs().max(dim=1).values
    amax = D.double() * (E - E.min(dim=1, keepdim=True).values).max(dim=1).values
    e = torch.tensor([eps_c(P, a, c) for a, c in zip(lmax.tolist(), amax.tolist())], dtype=torch.float64)
    up = (cess64((root + h).clamp(max=D.double()), l, el, P) - cess_frac).abs() / ((root + h).clamp(max=D.double()) - root).clamp_min(1e-300)
    dn = (cess64((root - h).clamp(min=0.0), l, el, P) - cess_frac).abs() / (root - (root - h).clamp(min=0.0)).clamp_min(1e-300)
    slope = torch.minimum(up, dn)
    return e * cess_frac / (slope * h) + U32 * (b.double().abs() + (b.double() + root).abs()) / h


# ---- the float64 adaptive sampler --------------------------------------------------------------------------------------------------
def adaptive_chain(parts_fn, x0, step, sd, L, noises, uniforms, max_steps, P, cess_target, min_step, ess_frac, resample_u):
    """hmc_resample_restated.smc_chain with the temperatures chosen by `search`: K = max_steps transitions from beta = 0; the init call
    and every end call k < K - 1 search with a ceiling of 1, end call K - 1 anneals to 1 in one plain step, end call K does not anneal;
    end calls k < K resample.  Returns smc_chain's record plus steps_used (G) -- the annealing calls a group entered below 1 -- and
    betas (K, G): every group's temperature after every annealing call."""
    import hmc_restated as H
    import hmc_metric_restated as MR
    import hmc_tempered_restated as TR
    f64 = torch.float64
    K, B = max_steps, x0.shape[0]
    s, sd = step.to(f64).reshape(B, 1), sd.to(f64)
    beta = torch.zeros(B, dtype=f64)
    one = torch.ones(B, dtype=f64)
    w, c = torch.zeros(B, dtype=f64), torch.zeros(B, dtype=f64)
    x_acc = x0.to(f64)
    Pt = parts_fn(x_acc)
    u_acc, g_acc = TR.tempered(Pt, beta)
    el_acc, gl_acc = Pt.el, Pt.gl
    out = types.SimpleNamespace(acc=[], resampled=[], ess=[], betas=[])
    used = torch.zeros(B // P, dtype=f64)

    def anneal(k):
        nonlocal w, c, u_acc, g_acc, beta, used
        if k >= K:
            return
        used += (beta.view(-1, P)[:, 0] < 1.0).double()
        bn = search(beta, one, w - c, el_acc, P, cess_target, min_step).beta if k < K - 1 else one
        d = bn - beta
        w, c = TR.weigh(w, c, d, el_acc)
        u_acc, g_acc = TR.retemper(u_acc, g_acc, el_acc, gl_acc, d)
        beta = bn.clone()
        out.betas.append(beta.view(-1, P)[:, 0].clone())
    anneal(0)
    for k in range(1, K + 1):
        qh, x, kin0 = MR.begin(x_acc, g_acc, noises[k - 1].to(f64), s, sd)
        for i in range(1, L):
            qh, x = MR.inner(x, qh, TR.tempered(parts_fn(x), beta)[1], s, sd)
        Pt = parts_fn(x)
        U_prop, g_prop = TR.tempered(Pt, beta)
        _, kinL = MR.end(qh, g_prop, s, sd)
        la = H.log_alpha(u_acc, U_prop, kin0, kinL)
        acc = H.accept(la, uniforms[k])
        a = acc[:, None]
        x_acc, g_acc, u_acc = torch.where(a, x, x_acc), torch.where(a, g_prop, g_acc), torch.where(acc, U_prop, u_acc)
        gl_acc, el_acc = torch.where(a, Pt.gl, gl_acc), torch.where(acc, Pt.el, el_acc)
        anneal(k)
        out.acc.append(acc)
        if k < K:
            d = R.decide(w - c, resample_u[k].to(f64), P, ess_frac)
            x_acc, g_acc, u_acc, gl_acc, el_acc = R.gather(beta, x_acc, g_acc, u_acc, gl_acc, el_acc, d.ancestor)
            w, c = torch.where(d.on, d.lw, w), torch.where(d.on, torch.zeros_like(c), c)
            out.resampled.append(d.group_on); out.ess.append(d.ess.view(-1, P)[:, 0])
    out.acc = torch.stack(out.acc)
    out.resampled = torch.stack(out.resampled) if out.resampled else torch.zeros(0, B // P, dtype=torch.bool)
    out.betas = torch.stack(out.betas)
    out.state, out.beta, out.log_w, out.steps_used = (x_acc, g_acc, u_acc, gl_acc, el_acc), beta, (w, c), used
    return out


EXP_MAX_STEPS, EXP_TARGET = 40, 0.98


def run(p, quads, space, max_steps, L, chains, step, seed, particles=16, cess_target=EXP_TARGET, ess_threshold=0.5, min_step=None):
    """One float64 adaptive run with ais_restated.run's draws (the same generator; the groups' uniforms after them): (log Z_hat (N),
    ess (N), the mean acceptance, the trace)."""
    import ais_restated as A
    import hmc_tempered_restated as TR
    f64 = torch.float64
    K, B, nz = max_steps, len(quads) * chains, A.GEO[0]
    g = torch.Generator().manual_seed(5000 + seed)
    x0, _ = A.prior_draws(p, space, B, g)
    noises = [torch.randn(B, nz, generator=g, dtype=f64) for _ in range(K)] + [None]
    uniforms = [None] + [torch.rand(B, generator=g, dtype=f64).clamp_min(2.0 ** -25) for _ in range(K)]
    ru = [None] + [torch.rand(B, generator=g, dtype=f64) for _ in range(K)]
    ms = 1.0 / (4.0 * K) if min_step is None else min_step
    tr = adaptive_chain(TR.flow_parts(space, p, A.Stacked(quads, chains)), x0, torch.full((B,), step, dtype=f64), torch.ones(B, nz, dtype=f64),
                        L, noises, uniforms, K, particles, cess_target, ms, ess_threshold, ru)
    logz, ess = A.reduce(tr.log_w[0] - tr.log_w[1], chains)
    return logz, ess, tr.acc.double().mean().item(), tr


def experiment(seed, space, max_steps=EXP_MAX_STEPS, cess_target=EXP_TARGET):
    """The experiment at one seed: (errors log Z_hat - closed form (N), final ess (N), mean acceptance, steps used per group)."""
    import ais_restated as A
    p = A.affine_flow()
    quads = [A.datum(s) for s in A.EXP_DATA]
    logz, ess, acc, tr = run(p, quads, space, max_steps, A.EXP_L, A.EXP_CHAINS, A.EXP_STEP, seed, cess_target=cess_target)
    exact = torch.tensor([A.closed_form(p, q) for q in quads], dtype=torch.float64)
    return logz - exact, ess, acc, tr.steps_used


# The figures over seeds 0 .. 7 at max_steps = 40, cess_target = 0.98 (profiles/smc_adaptive_cpu.txt has every seed's figures and the
# arithmetic; tests/test_smc_adaptive_cpu.py holds one seed to them), made as smc_restated.BAND was made: the observed range over the
# 16 estimates (error, ess) or the 8 runs (accept) or the 64 groups (steps) widened by 3 standard deviations of them.
BAND = {
    "z": {"error": (-0.897, 1.122), "ess": (13.6, 68.8), "accept": (0.948, 0.973), "steps": (14.0, 37.0)},
    "eps": {"error": (-0.732, 0.756), "ess": (18.4, 72.4), "accept": (0.865, 0.902), "steps": (14.9, 37.1)},
}

"""TEST INFRASTRUCTURE (CPU; float64 and float32): the resampling move of `lsnf_hmc_step_resample` /
`lsnf_reverse_hmc_step_resample` (include/lsnf_flow_mcmc.h), restated on tests/hmc_tempered_restated.py.

Rows [k P, (k + 1) P) are the particles of group k, rung r = row % P.  After an annealing end call's weight increment, with {w_i, c_i}
the rows' Kahan pairs and i, j over the group's rungs in rung order:
    l_i = w_i - c_i;   m = max_i l_i;   e_i = exp(l_i - m);   S1 = sum_i e_i;   S2 = sum_i e_i * e_i;   ess = (S1 * S1) / S2
    the group resamples iff ess < ess_frac * P                       (a NaN anywhere: it does not)
    tau_k = ((k + u) / P) * S1;   cum_j = e_0 + .. + e_j;   a_k = min(#{ j : cum_j <= tau_k }, P - 1)
    log_w <- { m + log(S1 / P), 0 } on every row of a resampling group
and a row with a_k != k takes its ancestor a's state at its OWN temperature (d_own = beta_k - beta_a, both after the anneal):
    z <- z_a;  gl <- gl_a;  el <- el_a;  g <- g_a + (d_own * gl_a);  u <- u_a + (d_own * el_a)
`decide`: those lines on tensors of any dtype (fp32: every operation a torch fp32 operation in the header's order); `gather`: the move
of the state; `margins`: how far a float64 decision is from flipping; `bounds`: what fp32 may differ from float64 in ess and log_w;
`offspring`: the counts; `smc_chain`: the float64 sampler over any `parts(x) -> Parts`.

The fp32 error of the device's decision quantities, relative to S1 (S1 >= 1 since the largest e is 1): one rounding of l - m moves
e_i by at most 2^-24 |l_i - m| e_i <= 2^-24 * 2 max|l| * e_i, expf by EXP_ULP ulps, and the P - 1 additions by 2^-24 each, so a
cumulative sum or a threshold is within  ERR(P, max|l|) = 2^-24 * (2 max|l| + 2 EXP_ULP + P + 2)  of its exact value relative to S1
(the + 2: the two roundings of tau).  `margins` reports distances in units of that figure.

EXP_ULP / LOG_ULP: the error of the device's expf / logf in units in the last place.  No OCML accuracy table ships with the toolchain;
they are the figures tools/micro/ocml_ulp.hip measures on an MI355X over the tests' argument ranges (x in [-140, 0] for expf, [2^-5, 1]
for logf), rounded up to the next whole ulp: profiles/hmc_resample_geometries.txt."""
import types

import torch

GROUPS = (2, 4, 8, 16)
EXP_ULP = 1.0
LOG_ULP = 3.0
U32 = 2.0 ** -24


def err(P, lmax):
    """The fp32 error of a cumulative sum or a threshold relative to S1 (module docstring)."""
    return U32 * (2.0 * lmax + 2.0 * EXP_ULP + P + 2.0)


def decide(l, u, P, ess_frac):
    """The group's decision in l's dtype.  l (B): the rows' log weights; u (B): the groups' uniforms, read at the group's first row.
    Returns on (B) bool, ancestor (B) long -- the ROW the state comes from --, rung (B) long -- its rung, ancestor_out's number --,
    ess (B), lw (B) -- the new log weight of a resampling group's rows --, and per group s1 (G), cum (G, P), tau (G, P), m (G)."""
    assert P in GROUPS and l.shape[0] % P == 0
    dt, dev = l.dtype, l.device
    L = l.view(-1, P)
    G = L.shape[0]
    m = L[:, 0]
    for j in range(1, P):
        m = torch.fmax(m, L[:, j])                           # (fmaxf: a NaN is passed over)
    e = torch.exp(L - m[:, None])
    s1, s2, cum = torch.zeros(G, dtype=dt, device=dev), torch.zeros(G, dtype=dt, device=dev), []
    for j in range(P):
        q = e[:, j] * e[:, j]
        s1 = s1 + e[:, j]
        s2 = s2 + q
        cum.append(s1)
    cum = torch.stack(cum, dim=1)
    ess = (s1 * s1) / s2
    fp = torch.tensor(float(P), dtype=dt, device=dev)
    on = ess < torch.tensor(ess_frac, dtype=dt, device=dev) * fp
    k = torch.arange(P, device=dev)
    ug = u.view(-1, P)[:, 0].to(dt)
    tau = ((k.to(dt)[None, :] + ug[:, None]) / fp) * s1[:, None]
    cnt = (cum[:, None, :] <= tau[:, :, None]).sum(dim=2)    # [group, rung k]: #{ j : cum_j <= tau_k }
    rung = torch.where(on[:, None], cnt.clamp(max=P - 1), k[None, :].expand(G, P))
    first = (torch.arange(G, device=dev) * P)[:, None]
    lw = m + torch.log(s1 / fp)
    rows = lambda t: t[:, None].expand(G, P).reshape(-1)
    return types.SimpleNamespace(on=rows(on), ancestor=(first + rung).reshape(-1), rung=rung.reshape(-1), ess=rows(ess), lw=rows(lw),
                                 s1=s1, cum=cum, tau=tau, m=m, e=e, group_on=on)


def gather(beta, z, g, u, gl, el, ancestor):
    """(z, g, u, gl, el) after the move, in the tensors' dtype: a row whose ancestor is another row takes that row's state, its
    gradient and potential re-tempered to the row's own beta (both temperatures after the anneal); other rows keep theirs to the bit."""
    a = ancestor.to(beta.device)
    moved = a != torch.arange(a.shape[0], device=a.device)
    d = beta - beta[a]
    g2 = g[a] + (d[:, None] * gl[a])
    u2 = u[a] + (d * el[a])
    mv = moved[:, None]
    return torch.where(mv, z[a], z), torch.where(mv, g2, g), torch.where(moved, u2, u), torch.where(mv, gl[a], gl), torch.where(moved, el[a], el)


def margins(d, P, ess_frac, lmax):
    """(the least |cum_j - tau_k| / S1 over the resampling groups' rungs, the least |ess - ess_frac P| / P over all groups), both in
    units of err(P, lmax) -- the second times 4: ess is a ratio of a square and a sum of squares, four times the relative error."""
    unit = err(P, lmax)
    on = d.group_on
    gap = ((d.cum[:, None, :] - d.tau[:, :, None]).abs() / d.s1[:, None, None]).flatten(1).min(dim=1).values
    gap = gap[on].min().item() / unit if bool(on.any()) else float("inf")
    ess = d.ess.view(-1, P)[:, 0]
    edge = ((ess - ess_frac * P).abs() / ess).min().item() / (4.0 * unit)
    return gap, edge


def bounds(d64, P, lmax):
    """What the device's fp32 ess and new log_w may differ from the float64 ones by, from the operation sequence: (rel_ess (B),
    abs_lw (B)).  With de = 2^-24 (2 lmax + 2 EXP_ULP) the relative error of an e_i (the rounding of l - m, expf): S1 carries de and
    P - 1 additions; q_i = e_i^2 carries 2 de + 1 rounding, S2 that and P - 1 additions; ess one product and one quotient more.
    log_w: S1 / P is exact, logf moves by S1's relative error and LOG_ULP ulps of its value, m + . is one rounding.  1 % is added
    for the second-order terms."""
    de = U32 * (2.0 * lmax + 2.0 * EXP_ULP)
    r1 = de + (P - 1) * U32
    r2 = 2.0 * de + U32 + (P - 1) * U32
    rel_ess = 1.01 * (2.0 * r1 + U32 + r2 + U32) * torch.ones_like(d64.ess)
    lg = torch.log(d64.s1 / P)
    lg = lg[:, None].expand(-1, P).reshape(-1)
    abs_lw = 1.01 * (r1 + 2.0 * LOG_ULP * U32 * lg.abs() + U32 * d64.lw.abs())
    return rel_ess, abs_lw


def offspring(rung, P):
    """(G, P) long: how many rows of each group descend from each rung."""
    r = rung.view(-1, P)
    return torch.stack([(r == j).sum(dim=1) for j in range(P)], dim=1)


def smc_chain(parts_fn, x0, step, sd, L, noises, uniforms, beta0, anneals, P, ess_frac, resample_u):
    """hmc_tempered_restated.chain with the move after end call k's anneal, k = 1 .. K - 1 (the init call and the last end call do not
    resample): the float64 SMC sampler.  resample_u[k] (B): the groups' uniforms of end call k, read at the group's first row.
    Returns that chain's record plus resampled (K - 1, G) bool and ess (K - 1, G)."""
    import hmc_restated as H
    import hmc_metric_restated as MR
    import hmc_tempered_restated as TR
    f64 = torch.float64
    K, B = len(noises) - 1, x0.shape[0]
    s, sd = step.to(f64).reshape(B, 1), sd.to(f64)
    beta = beta0.to(f64).reshape(B).clone()
    w, c = torch.zeros(B, dtype=f64), torch.zeros(B, dtype=f64)
    x_acc = x0.to(f64)
    Pt = parts_fn(x_acc)
    u_acc, g_acc = TR.tempered(Pt, beta)
    el_acc, gl_acc = Pt.el, Pt.gl
    out = types.SimpleNamespace(acc=[], resampled=[], ess=[])

    def anneal(bn):
        nonlocal w, c, u_acc, g_acc, beta
        if bn is None:
            return
        d = bn.to(f64) - beta
        w, c = TR.weigh(w, c, d, el_acc)
        u_acc, g_acc = TR.retemper(u_acc, g_acc, el_acc, gl_acc, d)
        beta = bn.to(f64).clone()
    anneal(anneals[0])
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
        anneal(anneals[k])
        out.acc.append(acc)
        if k < K and anneals[k] is not None:
            d = decide(w - c, resample_u[k].to(f64), P, ess_frac)
            x_acc, g_acc, u_acc, gl_acc, el_acc = gather(beta, x_acc, g_acc, u_acc, gl_acc, el_acc, d.ancestor)
            w, c = torch.where(d.on, d.lw, w), torch.where(d.on, torch.zeros_like(c), c)
            out.resampled.append(d.group_on); out.ess.append(d.ess.view(-1, P)[:, 0])
    out.acc = torch.stack(out.acc)
    out.resampled = torch.stack(out.resampled) if out.resampled else torch.zeros(0, B // P, dtype=torch.bool)
    out.ess = torch.stack(out.ess) if out.ess else torch.zeros(0, B // P, dtype=f64)
    out.state, out.beta, out.log_w = (x_acc, g_acc, u_acc, gl_acc, el_acc), beta, (w, c)
    return out

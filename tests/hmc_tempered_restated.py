"""TEST INFRASTRUCTURE (CPU; float64 and float32): the likelihood temperature per row of `lsnf_hmc_step_tempered` /
`lsnf_reverse_hmc_step_tempered` (include/lsnf_flow_mcmc.h), restated on tests/hmc_metric_restated.py.

The target at inverse temperature beta is p_flow(z) p(x | G(z))^beta.  A point's potential is kept in its parts (`Parts`): the prior's
(ll in z, 1/2 |eps|^2 in eps; its gradient) and the likelihood's, el and gl (z: energy_g, grad_g; eps: energy_g and the pull-back
J_{f^-1}(eps)^T grad_g).  With row b at beta[b]:
    z:    g = (beta gl) + d(-ll)/dz;    U = (beta el) - ll
    eps:  t = eps + (beta gl);          U = (beta el) + 1/2 sum eps^2
and begin / inner / end, the decision and the state update are the metric chain's.  An anneal to beta' after a decision, with
(g_s, u_s, gl_s, el_s) the state after it and d = beta' - beta:
    inc = -(d el_s);  y = inc - c;  t = w + y;  c' = (t - w) - y;  w' = t          (Kahan's sum of the log importance weight)
    u_s <- u_s + (d el_s);  g_s <- g_s + (d gl_s);  beta <- beta'
`tempered` / `retemper` / `weigh`: those lines on tensors of any dtype (fp32: every operation a torch fp32 operation, the products
formed first).  `chain`: the float64 chain over any `parts(x) -> Parts`."""
import types

import torch

from oracle import flow_oracle as O
import hmc_restated as H
import hmc_metric_restated as MR
import rmala_restated as RM


class Parts:
    """space; a: ll (z) or 1/2 sum eps^2 (eps), (B); pg: the prior's gradient, d(-ll)/dz or eps, (B, nz); el (B), gl (B, nz): the
    likelihood's energy and gradient; x: the point in z (the point itself, or f^-1(eps))."""

    def __init__(self, space, a, pg, el, gl, x):
        self.space, self.a, self.pg, self.el, self.gl, self.x = space, a, pg, el, gl, x


def parts(space, p, point, quad, dtype=torch.float64):
    """The potential's parts at the rows `point`, in `dtype`; mala_restated.potential's / rmala_restated.potential's quantities."""
    if space == "z":
        q, zz = O.to_dtype(p, dtype), point.to(dtype)
        ll = O.flow_log_prob(q, zz)[2].detach()
        gf = O.grad_neg_sum_ll_wrt_z(q, zz)
        e, ge = quad(zz)
        return Parts(space, ll, gf, e, ge, zz)
    ee = point.to(dtype)
    x = RM.reverse_of(p, ee, dtype)
    e, ge = quad(x)
    return Parts(space, 0.5 * (ee * ee).sum(1), ee, e, RM.pull_back(p, ee, ge, dtype), x)


def tempered(P, beta):
    """(U, grad U) of the parts at the rows' beta (B), in the parts' dtype: the header's lines, the products formed first."""
    b = beta.to(P.el.dtype)
    if P.space == "z":
        return (b * P.el) - P.a, (b[:, None] * P.gl) + P.pg
    return (b * P.el) + P.a, P.pg + (b[:, None] * P.gl)


def retemper(u, g, el, gl, d):
    """(u + (d el), g + (d gl)): the kept potential and gradient at beta + d."""
    return u + (d * el), g + (d[:, None] * gl)


def weigh(w, c, d, el):
    """(w', c') of the Kahan pair after the increment -(d el), in the tensors' dtype."""
    inc = -(d * el)
    y = inc - c
    t = w + y
    return t, (t - w) - y


def flow_parts(space, p, quad):
    return lambda x: parts(space, p, x, quad)


def chain(parts_fn, x0, step, sd, L, noises, uniforms, beta0, anneals=None):
    """The float64 chain from x0 (B, nz): K = len(noises) - 1 trajectories of L steps as hmc_metric_restated.chain's (frozen steps and
    scales), row b at beta0[b].  anneals[0]: the rows' next beta after the init call (or None), anneals[k], k = 1 .. K: after end call
    k's decision.  Returns la / acc (K, B), states (K, B, nz), the final state (x, grad, U, gl, el), beta, log_w = (w, c) and
    weights (K + 1, B): w - c after the init call and after every end call."""
    f64 = torch.float64
    K, B = len(noises) - 1, x0.shape[0]
    anneals = [None] * (K + 1) if anneals is None else anneals
    s, sd = step.to(f64).reshape(B, 1), sd.to(f64)
    beta = beta0.to(f64).reshape(B).clone()
    w, c = torch.zeros(B, dtype=f64), torch.zeros(B, dtype=f64)
    x_acc = x0.to(f64)
    P = parts_fn(x_acc)
    u_acc, g_acc = tempered(P, beta)
    el_acc, gl_acc = P.el, P.gl
    out = types.SimpleNamespace(la=[], acc=[], states=[], weights=[])

    def anneal(bn):
        nonlocal w, c, u_acc, g_acc, beta
        if bn is None:
            return
        d = bn.to(f64) - beta
        w, c = weigh(w, c, d, el_acc)
        u_acc, g_acc = retemper(u_acc, g_acc, el_acc, gl_acc, d)
        beta = bn.to(f64).clone()
    anneal(anneals[0])
    out.weights.append(w - c)
    for k in range(1, K + 1):
        qh, x, kin0 = MR.begin(x_acc, g_acc, noises[k - 1].to(f64), s, sd)
        for i in range(1, L):
            qh, x = MR.inner(x, qh, tempered(parts_fn(x), beta)[1], s, sd)
        P = parts_fn(x)
        U_prop, g_prop = tempered(P, beta)
        _, kinL = MR.end(qh, g_prop, s, sd)
        la = H.log_alpha(u_acc, U_prop, kin0, kinL)
        acc = H.accept(la, uniforms[k])
        a = acc[:, None]
        x_acc, g_acc, u_acc = torch.where(a, x, x_acc), torch.where(a, g_prop, g_acc), torch.where(acc, U_prop, u_acc)
        gl_acc, el_acc = torch.where(a, P.gl, gl_acc), torch.where(acc, P.el, el_acc)
        anneal(anneals[k])
        out.la.append(la); out.acc.append(acc); out.states.append(x_acc.clone()); out.weights.append(w - c)
    out.la, out.acc, out.states, out.weights = torch.stack(out.la), torch.stack(out.acc), torch.stack(out.states), torch.stack(out.weights)
    out.state, out.beta, out.log_w = (x_acc, g_acc, u_acc, gl_acc, el_acc), beta, (w, c)
    return out

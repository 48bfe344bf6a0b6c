"""TEST INFRASTRUCTURE (CPU; float64 and float32): the replica-exchange move of `lsnf_hmc_step_exchange` /
`lsnf_reverse_hmc_step_exchange` (include/lsnf_flow_mcmc.h), restated on tests/hmc_tempered_restated.py.

Rows [k R, (k + 1) R) are the rungs of ladder k, rung r = row % R, at whatever beta the rows hold.  A swapping end call pairs rungs
(0,1), (2,3), .. (even) or (1,2), (3,4), .. (odd; rungs 0 and R - 1 idle, nothing at R = 2).  With (z_s, g_s, u_s, gl_s, el_s) a row's
state after the trajectory's decision, for the pair (a, b), a the lower row:
    d = beta_a - beta_b;  e = el_s_a - el_s_b;  log_r = d * e;        the pair swaps iff log(u_a) < log_r
and a row that swaps takes its partner p's state at its OWN temperature (d_own = beta_own - beta_p):
    z <- z_s_p;  gl <- gl_s_p;  el <- el_s_p;  g <- g_s_p + (d_own * gl_s_p);  u <- u_s_p + (d_own * el_s_p)
`pairs` / `partner`: the pairing; `log_ratio` / `exchange`: those lines on tensors of any dtype (fp32: every operation a torch fp32
operation in the header's order, each product formed first); `chain`: the float64 chain with swaps over any `parts(x) -> Parts`."""
import types

import torch

import hmc_restated as H
import hmc_metric_restated as MR
import hmc_tempered_restated as TR

LADDERS = (2, 4, 8, 16)


def pairs(R, parity):
    """The rung pairs (a, a + 1) of a swap call of `parity` ("even" | "odd") on a ladder of R rungs."""
    assert R in LADDERS and parity in ("even", "odd")
    return [(a, a + 1) for a in range(0 if parity == "even" else 1, R - 1, 2)]


def partner(B, R, parity):
    """(B) long: every row's partner row, the row itself on an idle rung.  Pairs never cross a ladder's border."""
    assert B % R == 0
    p = torch.arange(B)
    for k in range(0, B, R):
        for a, b in pairs(R, parity):
            p[k + a], p[k + b] = k + b, k + a
    return p


def log_ratio(beta, el, prt):
    """(B): log_r of every row's pair in the tensors' dtype, formed by both rows as the lower row forms it; 0 on an idle rung."""
    rows = torch.arange(beta.shape[0], device=beta.device)
    prt = prt.to(beta.device)
    lo, hi = torch.minimum(rows, prt), torch.maximum(rows, prt)
    d = beta[lo] - beta[hi]
    e = el[lo] - el[hi]
    return torch.where(prt != rows, d * e, torch.zeros_like(d))


def decide(log_r, u, prt):
    """(B) bool: both rows of a pair swap iff log(u[lower row]) < log_r (a NaN log_r rejects); an idle rung never does."""
    rows = torch.arange(log_r.shape[0], device=log_r.device)
    prt = prt.to(log_r.device)
    return (prt != rows) & (torch.log(u[torch.minimum(rows, prt)]) < log_r)


def exchange(beta, z, g, u, gl, el, prt, sw):
    """(z, g, u, gl, el) after the exchange, in the tensors' dtype: rows with sw take the partner's state, its gradient and potential
    re-tempered to the row's own beta."""
    prt = prt.to(beta.device)
    d = beta - beta[prt]
    g2 = g[prt] + (d[:, None] * gl[prt])
    u2 = u[prt] + (d * el[prt])
    m = sw[:, None]
    return torch.where(m, z[prt], z), torch.where(m, g2, g), torch.where(sw, u2, u), torch.where(m, gl[prt], gl), torch.where(sw, el[prt], el)


def chain(parts_fn, x0, step, sd, L, noises, uniforms, beta, R, swaps=None, swap_uniforms=None):
    """The float64 chain from x0 (B, nz): K = len(noises) - 1 trajectories of L steps as hmc_tempered_restated.chain's without anneals,
    row b at beta[b] throughout.  swaps[k - 1] in (None, "even", "odd"): what end call k does after its decision, with the pairs'
    uniforms swap_uniforms[k - 1] (B, read at the lower row).  Returns la / acc (K, B), states (K, B, nz) after every end call (the
    exchange included), swapped / log_swap (K, B) (zeros where the call does not swap) and the final state (x, grad, U, gl, el)."""
    f64 = torch.float64
    K, B = len(noises) - 1, x0.shape[0]
    swaps = [None] * K if swaps is None else swaps
    s, sd = step.to(f64).reshape(B, 1), sd.to(f64)
    beta = beta.to(f64).reshape(B)
    x_acc = x0.to(f64)
    P = parts_fn(x_acc)
    u_acc, g_acc = TR.tempered(P, beta)
    el_acc, gl_acc = P.el, P.gl
    out = types.SimpleNamespace(la=[], acc=[], states=[], swapped=[], log_swap=[])
    for k in range(1, K + 1):
        qh, x, kin0 = MR.begin(x_acc, g_acc, noises[k - 1].to(f64), s, sd)
        for i in range(1, L):
            qh, x = MR.inner(x, qh, TR.tempered(parts_fn(x), beta)[1], s, sd)
        P = parts_fn(x)
        U_prop, g_prop = TR.tempered(P, beta)
        _, kinL = MR.end(qh, g_prop, s, sd)
        la = H.log_alpha(u_acc, U_prop, kin0, kinL)
        acc = H.accept(la, uniforms[k])
        a = acc[:, None]
        x_acc, g_acc, u_acc = torch.where(a, x, x_acc), torch.where(a, g_prop, g_acc), torch.where(acc, U_prop, u_acc)
        gl_acc, el_acc = torch.where(a, P.gl, gl_acc), torch.where(acc, P.el, el_acc)
        sw, lr = torch.zeros(B, dtype=torch.bool), torch.zeros(B, dtype=f64)
        if swaps[k - 1] is not None:
            prt = partner(B, R, swaps[k - 1])
            lr = log_ratio(beta, el_acc, prt)
            sw = decide(lr, swap_uniforms[k - 1].to(f64), prt)
            x_acc, g_acc, u_acc, gl_acc, el_acc = exchange(beta, x_acc, g_acc, u_acc, gl_acc, el_acc, prt, sw)
        out.la.append(la); out.acc.append(acc); out.states.append(x_acc.clone()); out.swapped.append(sw); out.log_swap.append(lr)
    for f in ("la", "acc", "states", "swapped", "log_swap"):
        setattr(out, f, torch.stack(getattr(out, f)))
    out.state = (x_acc, g_acc, u_acc, gl_acc, el_acc)
    return out


# ---- the two-mode experiment of tests/test_hmc_exchange_cpu.py, stated once -------------------------------------------------------
class TwoMode:
    """el(z) = -log(exp(-E_1(z)) + exp(-E_2(z))) for two of the tests' axis-aligned quadratic energies (hmc_metric_restated.Diagonal
    at ais_restated's a = 0.3 .. 3.0) whose centres differ by `gap` along the stiffest coordinate: on ais_restated's affine flow the
    posterior p_flow(z) exp(-el(z)) is a mixture of two Gaussians with the closed-form weights Z_i / (Z_1 + Z_2)."""

    def __init__(self, nz, gap, seed=21):
        self.quads = [MR.Diagonal(nz, lo=0.3, hi=3.0, seed=seed) for _ in range(2)]
        self.axis = nz - 1
        self.mid = self.quads[0].t[self.axis].item()
        self.quads[0].t[self.axis] += 0.5 * gap
        self.quads[1].t[self.axis] -= 0.5 * gap

    def __call__(self, z):
        (e1, g1), (e2, g2) = (q(z) for q in self.quads)
        el = -torch.logsumexp(torch.stack([-e1, -e2]), 0)
        w1 = torch.exp(-e1 - (-el))[:, None]                 # the responsibility of mode 1
        return el, w1 * g1 + (1.0 - w1) * g2

    def in_mode_1(self, z):
        return z[..., self.axis] > self.mid

"""TEST INFRASTRUCTURE (CPU; float64 and float32): the base-space Metropolis-adjusted Langevin step of include/lsnf_flow_mcmc.h
(lsnf_reverse_mala_step) restated on oracle.flow_oracle (flow_reverse under autograd) and oracle.philox_oracle.

The chain runs on eps with x = f^-1(eps).  Target pi(eps) ~ exp(-U), U = |eps|^2 / 2 + e(x); the "generator" is the closed-form
quadratic e(x) = 1/2 |A (x - t)|^2 of mala_restated (`Quadratic`; None = the prior alone: N(0, I)).  grad U = eps + g,
g = J_{f^-1}(eps)^T grad e(x) by autograd of O.flow_reverse.  One call DECIDES a proposal against the kept state
(eps_acc, grad_acc, u_acc) and PROPOSES the next:
    t_prop = eps_prop + g_prop,  U_prop = e + 1/2 sum eps_prop^2,  d = eps_prop - eps_acc,  coef = s^2 / 2
    A = sum_c (coef t_prop - d)^2,  Bq = sum_c (d + coef grad_acc)^2,  log_alpha = (u_acc - U_prop) - (A - Bq) / (2 s^2)
    accept iff ln(u) < log_alpha;  eps_next = eps_state - coef grad_state + s xi
`uniform_draws` (the in-kernel uniform) and `Quadratic` are mala_restated's."""
import numpy as np
import torch

from oracle import flow_oracle as O
from oracle.philox_oracle import philox4x32_10  # noqa: F401  (the generator uniform_draws restates)
from mala_restated import Quadratic, uniform_draws, coef_of  # noqa: F401


def reverse_of(p, eps, dtype):
    """x = f^-1(eps) in `dtype` (detached)."""
    e = eps.to(dtype)
    return O.flow_reverse(O.to_dtype(p, dtype), e, torch.zeros(e.shape[0], dtype=dtype))[0].detach()


def pull_back(p, eps, gx, dtype):
    """J_{f^-1}(eps)^T gx by autograd of O.flow_reverse in `dtype`; gx (B, nz)."""
    e = eps.to(dtype).clone().requires_grad_(True)
    x = O.flow_reverse(O.to_dtype(p, dtype), e, torch.zeros(e.shape[0], dtype=dtype))[0]
    return torch.autograd.grad((x * gx.to(dtype)).sum(), e)[0]


def potential(p, eps, quad, dtype):
    """(U, grad U, e, grad_x e, x) at the rows eps, computed in `dtype`."""
    ee = eps.to(dtype)
    x = reverse_of(p, ee, dtype)
    if quad is None:
        e, ge, g = torch.zeros(ee.shape[0], dtype=dtype), torch.zeros_like(ee), torch.zeros_like(ee)
    else:
        e, ge = quad(x)
        g = pull_back(p, ee, ge, dtype)
    return 0.5 * (ee * ee).sum(1) + e, ee + g, e, ge, x


def decide(e_acc, t_acc, u_acc, e_prop, t_prop, U_prop, u, s):
    """(log_alpha, accept, A, Bq) of one decision, in the tensors' dtype; u (B,) in (0, 1)."""
    dtype = e_prop.dtype
    coef = coef_of(s, dtype)
    d = e_prop - e_acc
    A = ((coef * t_prop - d) ** 2).sum(1)
    Bq = ((d + coef * t_acc) ** 2).sum(1)
    two_s2 = float(np.float32(2.0) * np.float32(s) * np.float32(s)) if dtype == torch.float32 else 2.0 * s * s
    la = (u_acc - U_prop) - (A - Bq) / two_s2
    return la, torch.log(u.to(torch.float64)) < la.to(torch.float64), A, Bq


def propose(e_state, t_state, noise, s):
    return e_state - coef_of(s, e_state.dtype) * t_state + s * noise.to(e_state.dtype)


class Step:
    """One call of the teacher-forcing record: what the device is given (the float64 state BEFORE the call, the proposal, grad_g,
    energy_g, noise, uniform) and the float64 answers (log_alpha, accept, A, Bq, the state after, eps_next)."""


def smooth_proposal(p, e_state, t_state, noise, s, redraw, margin=2e-5, max_rounds=100):
    """The proposal from (e_state, t_state) with `noise`; redraw (a torch.Generator, or None): rows for which x = f^-1(proposal)
    lands within `margin` of a ReLU kink (oracle.relu_margin at x, where the pull-back is discontinuous) get a new noise row
    from it, IN PLACE in `noise`, until none does."""
    nxt = propose(e_state, t_state, noise.to(torch.float64), s)
    if redraw is None:
        return nxt
    near = lambda e: O.relu_margin(p, reverse_of(p, e, torch.float64)) <= margin
    bad = torch.nonzero(near(nxt)).flatten()
    for _ in range(max_rounds):
        if bad.numel() == 0:
            return nxt
        noise[bad] = torch.randn(int(bad.numel()), noise.shape[1], generator=redraw, dtype=noise.dtype)
        nxt[bad] = propose(e_state[bad], t_state[bad], noise[bad].to(torch.float64), s)
        bad = bad[near(nxt[bad])]
    raise RuntimeError(f"smooth_proposal: {bad.numel()} proposals still within {margin} of a ReLU kink after {max_rounds} redraws")


def chain(p, eps0, quad, s, noises, uniforms, redraw=None):
    """The float64 chain from eps0 (B, nz): call 0 starts it (every row accepted) and proposes with noises[0]; call j >= 1 decides
    with uniforms[j] and proposes with noises[j] (None: the last call only decides).  redraw: see smooth_proposal (the noises
    are then updated in place).  Returns the list of `Step` records of calls 1 .. len(noises) - 1 and the final state
    (eps, grad, U)."""
    f64 = torch.float64
    e_acc = eps0.to(f64)
    u_acc, t_acc, _, _, _ = potential(p, e_acc, quad, f64)
    e_prop = smooth_proposal(p, e_acc, t_acc, noises[0], s, redraw)
    steps = []
    for j in range(1, len(noises)):
        st = Step()
        st.e_acc, st.t_acc, st.u_acc, st.e_prop = e_acc, t_acc, u_acc, e_prop
        U_prop, t_prop, st.e, st.ge, st.x = potential(p, e_prop, quad, f64)
        st.U_prop, st.t_prop, st.u = U_prop, t_prop, uniforms[j]
        st.la, st.acc, st.A, st.Bq = decide(e_acc, t_acc, u_acc, e_prop, t_prop, U_prop, uniforms[j], s)
        a = st.acc[:, None]
        e_acc, t_acc, u_acc = torch.where(a, e_prop, e_acc), torch.where(a, t_prop, t_acc), torch.where(st.acc, U_prop, u_acc)
        st.e_after, st.t_after, st.u_after = e_acc, t_acc, u_acc
        st.noise = noises[j]
        st.e_next = None if noises[j] is None else smooth_proposal(p, e_acc, t_acc, noises[j], s, redraw)
        e_prop = st.e_next
        steps.append(st)
    return steps, (e_acc, t_acc, u_acc)


def potential32(p, st):
    """(U_prop, t_prop) of a recorded proposal in fp32, from the fp32 casts the device is given: eps_prop, and grad_g / energy_g
    as the casts of the float64 ones (evaluated at the float64 x)."""
    f32 = torch.float32
    ep = st.e_prop.to(f32)
    g = pull_back(p, ep, st.ge.to(f32), f32)
    return st.e.to(f32) + 0.5 * (ep * ep).sum(1), ep + g


def log_alpha32(p, st, quad, s):
    """The fp32 restatement of one recorded decision (potential32 at the proposal, the casts of the float64 state; `quad` is
    mala_restated.log_alpha32's argument: the record already holds its values)."""
    f32 = torch.float32
    U_prop, t_prop = potential32(p, st)
    return decide(st.e_acc.to(f32), st.t_acc.to(f32), st.u_acc.to(f32), st.e_prop.to(f32), t_prop, U_prop, st.u, s)[0]

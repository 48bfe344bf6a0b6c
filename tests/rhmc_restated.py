"""TEST INFRASTRUCTURE (CPU; float64 and float32): Hamiltonian Monte Carlo in the flow's base space (`lsnf_reverse_hmc_step`,
include/lsnf_flow_mcmc.h) restated on tests/rmala_restated.py (`potential` / `pull_back`: U, eps + g, e, grad e, x by autograd of
oracle.flow_oracle.flow_reverse) and tests/hmc_restated.py (`begin` / `inner` / `end` / `log_alpha` / `accept`: the leapfrog
arithmetic, which does not know which space it runs in).

The chain runs on eps with x = f^-1(eps).  Target pi(eps) ~ exp(-U), U = |eps|^2 / 2 + e(x), grad U = t = eps + g,
g = J_{f^-1}(eps)^T grad e(x); momentum ~ N(0, I), step s, L leapfrog steps per trajectory.  From a state (e_s, t_s, u_s):
    begin   kin0 = 1/2 sum xi^2;  ph = xi - (s/2) t_s;  eps_1 = e_s + s ph
    inner   at eps_i, i = 1 .. L-1:  ph = ph - s t(eps_i);  eps_{i+1} = eps_i + s ph
    end     at eps_L:  pL = ph - (s/2) t(eps_L);  kinL = 1/2 sum pL^2;  log_alpha = (u_s - U(eps_L)) + (kin0 - kinL);  accept iff ln u < log_alpha
One device call finishes the work at the point it is given and produces the next point; `chain` returns one `Call` record per device
call, exactly as hmc_restated.chain does, so the GPU tests can teacher-force every call.  Momentum rows for which x = f^-1(eps) at ANY
point of the trajectory lies within 2e-5 of a ReLU kink (oracle.relu_margin at x, where the pull-back is discontinuous) are redrawn."""
import torch

from oracle import flow_oracle as O
import hmc_restated as H
import rmala_restated as RM

Quadratic, uniform_draws = RM.Quadratic, RM.uniform_draws
potential, pull_back, reverse_of = RM.potential, RM.pull_back, RM.reverse_of
begin, inner, end, log_alpha, accept = H.begin, H.inner, H.end, H.log_alpha, H.accept


class Call:
    """One device call of the teacher-forcing record.  phase "init" | "inner" | "end"; e_prop, x, e, ge, g (= grad U = eps + pull-back),
    U_prop at the call's point; e_acc, g_acc, u_acc, mom_in, kin_in: the state before (None for init); noise, u; la, acc, pL, kinL
    (end); e_after, g_after, u_after, mom_out, kin_out, e_next: the float64 state after and the next point (None if nothing is
    proposed)."""


class Trajectory:
    """e[i], pot[i] = rmala_restated.potential at e[i] for i = 1 .. L (index 0 unused), ph[i] = the half-step momentum that leads from
    e[i] to e[i+1] (ph[0]: after the first half kick), kin0."""


def trajectory(p, quad, e_s, t_s, xi, s, L):
    f64 = torch.float64
    t = Trajectory()
    ph, e1, t.kin0 = begin(e_s, t_s, xi.to(f64), s)
    t.e, t.ph, t.pot = [None, e1], [ph], [None]
    for i in range(1, L + 1):
        t.pot.append(potential(p, t.e[i], quad, f64))
        if i < L:
            ph, en = inner(t.e[i], t.ph[i - 1], t.pot[i][1], s)
            t.ph.append(ph)
            t.e.append(en)
    return t


def smooth_trajectory(p, quad, e_s, t_s, noise, s, L, redraw, margin=2e-5, max_rounds=100):
    """The trajectory from (e_s, t_s) with the momentum draw `noise`; redraw (a torch.Generator, or None): rows of which ANY of the L
    points has its x = f^-1(eps) within `margin` of a ReLU kink get a new noise row from it, IN PLACE in `noise`, until none does."""
    t = trajectory(p, quad, e_s, t_s, noise, s, L)
    if redraw is None:
        return t

    def near(tr):
        return torch.stack([O.relu_margin(p, pot[4]) <= margin for pot in tr.pot[1:]]).any(0)
    bad = torch.nonzero(near(t)).flatten()
    for _ in range(max_rounds):
        if bad.numel() == 0:
            return t
        noise[bad] = torch.randn(int(bad.numel()), noise.shape[1], generator=redraw, dtype=noise.dtype)
        sub = trajectory(p, quad, e_s[bad], t_s[bad], noise[bad], s, L)
        t.kin0[bad] = sub.kin0
        for i in range(1, L + 1):
            t.e[i][bad] = sub.e[i]
            for a, b in zip(t.pot[i], sub.pot[i]):
                a[bad] = b
        for i in range(L):
            t.ph[i][bad] = sub.ph[i]
        bad = bad[near(sub)]
    raise RuntimeError(f"smooth_trajectory: {bad.numel()} trajectories still within {margin} of a ReLU kink after {max_rounds} redraws")


def chain(p, eps0, quad, s, L, noises, uniforms, redraw=None):
    """The float64 chain from eps0 (B, nz): K = len(noises) - 1 trajectories of L steps.  noises[t] starts trajectory t + 1 (noises[K]
    None: the last end call proposes nothing), uniforms[t] decides trajectory t (uniforms[0] unused).  Returns the K L + 1 `Call`
    records in call order and the final state (eps, grad, U)."""
    f64 = torch.float64
    K, B = len(noises) - 1, eps0.shape[0]
    e_acc = eps0.to(f64)
    u_acc, g_acc, e0, ge0, x0 = potential(p, e_acc, quad, f64)
    c = Call()
    c.phase, c.e_prop, c.e, c.ge, c.x, c.g, c.U_prop = "init", e_acc, e0, ge0, x0, g_acc, u_acc
    c.e_acc = c.g_acc = c.u_acc = c.mom_in = c.kin_in = c.u = c.kinL = c.pL = None
    c.la, c.acc = torch.zeros(B, dtype=f64), torch.ones(B, dtype=torch.bool)
    c.e_after, c.g_after, c.u_after, c.noise = e_acc, g_acc, u_acc, noises[0]
    tr = smooth_trajectory(p, quad, e_acc, g_acc, noises[0], s, L, redraw)
    c.mom_out, c.kin_out, c.e_next = tr.ph[0], tr.kin0, tr.e[1]
    calls = [c]
    for k in range(1, K + 1):
        for i in range(1, L + 1):
            c = Call()
            c.e_prop = tr.e[i]
            c.U_prop, c.g, c.e, c.ge, c.x = tr.pot[i]
            c.e_acc, c.g_acc, c.u_acc, c.mom_in, c.kin_in = e_acc, g_acc, u_acc, tr.ph[i - 1], tr.kin0
            if i < L:
                c.phase, c.noise, c.u, c.la, c.acc, c.kinL, c.pL = "inner", None, None, None, None, None, None
                c.e_after, c.g_after, c.u_after = e_acc, g_acc, u_acc
                c.mom_out, c.kin_out, c.e_next = tr.ph[i], tr.kin0, tr.e[i + 1]
            else:
                c.phase, c.noise, c.u = "end", noises[k], uniforms[k]
                c.pL, c.kinL = end(c.mom_in, c.g, s)
                c.la = log_alpha(u_acc, c.U_prop, c.kin_in, c.kinL)
                c.acc = accept(c.la, c.u)
                a = c.acc[:, None]
                e_acc, g_acc, u_acc = torch.where(a, c.e_prop, e_acc), torch.where(a, c.g, g_acc), torch.where(c.acc, c.U_prop, u_acc)
                c.e_after, c.g_after, c.u_after = e_acc, g_acc, u_acc
                if noises[k] is None:
                    c.mom_out, c.kin_out, c.e_next = c.pL, c.kin_in, None
                else:
                    tr = smooth_trajectory(p, quad, e_acc, g_acc, noises[k], s, L, redraw)
                    c.mom_out, c.kin_out, c.e_next = tr.ph[0], tr.kin0, tr.e[1]
            calls.append(c)
    return calls, (e_acc, g_acc, u_acc)


class Out32:
    """The fp32 restatement of one recorded call: la, U_prop, g, mom_out, e_next, kin_out from the fp32 casts the device is given."""


def potential32(p, c):
    """(U_prop, t_prop) of a recorded point in fp32, from the fp32 casts the device is given: eps_prop, and grad_g / energy_g as the
    casts of the float64 ones (evaluated at the float64 x) -- rmala_restated.potential32's rule."""
    f32 = torch.float32
    ep = c.e_prop.to(f32)
    g = pull_back(p, ep, c.ge.to(f32), f32) if bool((c.ge != 0).any()) else torch.zeros_like(ep)
    return c.e.to(f32) + 0.5 * (ep * ep).sum(1), ep + g


def call32(p, c, s):
    """The fp32 restatement of a recorded call from the fp32 casts of its inputs.  The begin of the next trajectory is restated from
    the float64 decision's state (as the device is compared on decided rows).  Fields: la, U_prop, g, mom_out, e_next, kin_out (None
    where the call has none)."""
    f32 = torch.float32
    ep = c.e_prop.to(f32)
    o = Out32()
    o.U_prop, o.g = potential32(p, c)
    o.la = o.mom_out = o.e_next = o.kin_out = None
    if c.phase == "inner":
        o.mom_out, o.e_next = inner(ep, c.mom_in.to(f32), o.g, s)
        return o
    if c.phase == "end":
        pl, kinl = end(c.mom_in.to(f32), o.g, s)
        o.la = log_alpha(c.u_acc.to(f32), o.U_prop, c.kin_in.to(f32), kinl)
        o.mom_out = pl
    if c.noise is not None:
        if c.phase == "init":
            es, gs = ep, o.g
        else:
            a = c.acc[:, None]
            es, gs = torch.where(a, ep, c.e_acc.to(f32)), torch.where(a, o.g, c.g_acc.to(f32))
        o.mom_out, o.e_next, o.kin_out = begin(es, gs, c.noise.to(f32), s)
    return o

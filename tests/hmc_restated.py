"""TEST INFRASTRUCTURE (CPU; float64 and float32): Hamiltonian Monte Carlo in z (`lsnf_hmc_step`, include/lsnf_flow_mcmc.h) restated
on oracle.flow_oracle, oracle.philox_oracle and tests/mala_restated.py (its `Quadratic` generator, `potential`, `uniform_draws` and the
kink-avoiding redraw, applied here to EVERY point a trajectory visits).

Target p(z) ~ exp(-U(z)), U = e(z) - ll(z), momentum ~ N(0, I), step s, L leapfrog steps per trajectory.  From a state
(z_s, g_s = grad U(z_s), u_s = U(z_s)):
    begin   kin0 = 1/2 sum xi^2;  ph = xi - (s/2) g_s;  z_1 = z_s + s ph
    inner   at z_i, i = 1 .. L-1:  ph = ph - s grad U(z_i);  z_{i+1} = z_i + s ph
    end     at z_L:  pL = ph - (s/2) grad U(z_L);  kinL = 1/2 sum pL^2;  log_alpha = (u_s - U(z_L)) + (kin0 - kinL);  accept iff ln u < log_alpha
One device call finishes the work at the point it is given and produces the next point; `chain` returns one `Call` record per device
call -- what the device is given (the float64 state, momentum and kin0 BEFORE the call, the point, grad_g, energy_g, noise, uniform)
and the float64 answers -- so the GPU tests can teacher-force every call."""
import torch

from oracle import flow_oracle as O
import mala_restated as M

Quadratic, potential, uniform_draws = M.Quadratic, M.potential, M.uniform_draws


def begin(z_s, g_s, xi, s):
    """(ph, z_1, kin0) in the tensors' dtype."""
    xi = xi.to(z_s.dtype)
    ph = xi - (0.5 * s) * g_s
    return ph, z_s + s * ph, 0.5 * (xi * xi).sum(1)


def inner(z, mom, g, s):
    """(ph, z_next) of a leapfrog step inside a trajectory."""
    ph = mom - s * g
    return ph, z + s * ph


def end(mom, g_prop, s):
    """(pL, kinL): the last half kick."""
    pl = mom - (0.5 * s) * g_prop
    return pl, 0.5 * (pl * pl).sum(1)


def log_alpha(u_acc, U_prop, kin0, kinL):
    return (u_acc - U_prop) + (kin0 - kinL)


def accept(la, u):
    return torch.log(u.to(torch.float64)) < la.to(torch.float64)


class Call:
    """One device call of the teacher-forcing record.  phase "init" | "inner" | "end"; z_prop, e, ge, ll, g (= grad U), U_prop at the
    call's point; z_acc, g_acc, u_acc, mom_in, kin_in: the state before (None for init); noise, u; la, acc, kinL (end); z_after,
    g_after, u_after, mom_out, kin_out, z_next: the float64 state after and the next point (None if nothing is proposed)."""


class Trajectory:
    """z[i], pot[i] = potential at z[i] for i = 1 .. L (index 0 unused), ph[i] = the half-step momentum that leads from z[i] to z[i+1]
    (ph[0]: after the first half kick), kin0."""


def trajectory(p, quad, z_s, g_s, xi, s, L):
    f64 = torch.float64
    t = Trajectory()
    ph, z1, t.kin0 = begin(z_s, g_s, xi.to(f64), s)
    t.z, t.ph, t.pot = [None, z1], [ph], [None]
    for i in range(1, L + 1):
        t.pot.append(potential(p, t.z[i], quad, f64))
        if i < L:
            ph, zn = inner(t.z[i], t.ph[i - 1], t.pot[i][1], s)
            t.ph.append(ph)
            t.z.append(zn)
    return t


def smooth_trajectory(p, quad, z_s, g_s, noise, s, L, redraw, margin=2e-5, max_rounds=100):
    """The trajectory from (z_s, g_s) with the momentum draw `noise`; redraw (a torch.Generator, or None): rows of which ANY of the L
    points lands within `margin` of a ReLU kink get a new noise row from it, IN PLACE in `noise`, until none does
    (mala_restated.smooth_proposal's rule for every point visited)."""
    t = trajectory(p, quad, z_s, g_s, noise, s, L)
    if redraw is None:
        return t

    def near(tr):
        return torch.stack([O.relu_margin(p, z.float()) <= margin for z in tr.z[1:]]).any(0)
    bad = torch.nonzero(near(t)).flatten()
    for _ in range(max_rounds):
        if bad.numel() == 0:
            return t
        noise[bad] = torch.randn(int(bad.numel()), noise.shape[1], generator=redraw, dtype=noise.dtype)
        sub = trajectory(p, quad, z_s[bad], g_s[bad], noise[bad], s, L)
        t.kin0[bad] = sub.kin0
        for i in range(1, L + 1):
            t.z[i][bad] = sub.z[i]
            for a, b in zip(t.pot[i], sub.pot[i]):
                a[bad] = b
        for i in range(L):
            t.ph[i][bad] = sub.ph[i]
        bad = bad[near(sub)]
    raise RuntimeError(f"smooth_trajectory: {bad.numel()} trajectories still within {margin} of a ReLU kink after {max_rounds} redraws")


def chain(p, z0, quad, s, L, noises, uniforms, redraw=None):
    """The float64 chain from z0 (B, nz): K = len(noises) - 1 trajectories of L steps.  noises[t] starts trajectory t + 1 (noises[K]
    None: the last end call proposes nothing), uniforms[t] decides trajectory t (uniforms[0] unused).  Returns the K L + 1 `Call`
    records in call order and the final state (z, grad, U)."""
    f64 = torch.float64
    K, B = len(noises) - 1, z0.shape[0]
    z_acc = z0.to(f64)
    u_acc, g_acc, e0, ge0, ll0 = potential(p, z_acc, quad, f64)
    c = Call()
    c.phase, c.z_prop, c.e, c.ge, c.ll, c.g, c.U_prop = "init", z_acc, e0, ge0, ll0, g_acc, u_acc
    c.z_acc = c.g_acc = c.u_acc = c.mom_in = c.kin_in = c.u = c.kinL = None
    c.la, c.acc = torch.zeros(B, dtype=f64), torch.ones(B, dtype=torch.bool)
    c.z_after, c.g_after, c.u_after, c.noise = z_acc, g_acc, u_acc, noises[0]
    tr = smooth_trajectory(p, quad, z_acc, g_acc, noises[0], s, L, redraw)
    c.mom_out, c.kin_out, c.z_next = tr.ph[0], tr.kin0, tr.z[1]
    calls = [c]
    for k in range(1, K + 1):
        for i in range(1, L + 1):
            c = Call()
            c.z_prop = tr.z[i]
            c.U_prop, c.g, c.e, c.ge, c.ll = tr.pot[i]
            c.z_acc, c.g_acc, c.u_acc, c.mom_in, c.kin_in = z_acc, g_acc, u_acc, tr.ph[i - 1], tr.kin0
            if i < L:
                c.phase, c.noise, c.u, c.la, c.acc, c.kinL = "inner", None, None, None, None, None
                c.z_after, c.g_after, c.u_after = z_acc, g_acc, u_acc
                c.mom_out, c.kin_out, c.z_next = tr.ph[i], tr.kin0, tr.z[i + 1]
            else:
                c.phase, c.noise, c.u = "end", noises[k], uniforms[k]
                c.pL, c.kinL = end(c.mom_in, c.g, s)
                c.la = log_alpha(u_acc, c.U_prop, c.kin_in, c.kinL)
                c.acc = accept(c.la, c.u)
                a = c.acc[:, None]
                z_acc, g_acc, u_acc = torch.where(a, c.z_prop, z_acc), torch.where(a, c.g, g_acc), torch.where(c.acc, c.U_prop, u_acc)
                c.z_after, c.g_after, c.u_after = z_acc, g_acc, u_acc
                if noises[k] is None:
                    c.mom_out, c.kin_out, c.z_next = c.pL, c.kin_in, None
                else:
                    tr = smooth_trajectory(p, quad, z_acc, g_acc, noises[k], s, L, redraw)
                    c.mom_out, c.kin_out, c.z_next = tr.ph[0], tr.kin0, tr.z[1]
            calls.append(c)
    return calls, (z_acc, g_acc, u_acc)


class Out32:
    """The fp32 restatement of one recorded call: la, acc-independent outputs from the fp32 casts the device is given."""


def call32(p, c, quad, s):
    """The fp32 restatement of a recorded call from the fp32 casts of its inputs (the potential at the point is recomputed in fp32;
    grad_g / energy_g are the casts of the float64 ones, as the device gets them).  The begin of the next trajectory is restated
    from the float64 decision's state (as the device is compared on decided rows).  Fields: la, U_prop, g, mom_out, z_next, kin_out
    (None where the call has none)."""
    f32 = torch.float32
    q, zp = O.to_dtype(p, f32), c.z_prop.to(f32)
    o = Out32()
    o.g = c.ge.to(f32) + O.grad_neg_sum_ll_wrt_z(q, zp)
    o.U_prop = c.e.to(f32) - O.flow_log_prob(q, zp)[2].detach()
    o.la = o.mom_out = o.z_next = o.kin_out = None
    if c.phase == "inner":
        o.mom_out, o.z_next = inner(zp, c.mom_in.to(f32), o.g, s)
        return o
    if c.phase == "end":
        pl, kinl = end(c.mom_in.to(f32), o.g, s)
        o.la = log_alpha(c.u_acc.to(f32), o.U_prop, c.kin_in.to(f32), kinl)
        o.mom_out = pl
    if c.noise is not None:
        if c.phase == "init":
            zs, gs = zp, o.g
        else:
            a = c.acc[:, None]
            zs, gs = torch.where(a, zp, c.z_acc.to(f32)), torch.where(a, o.g, c.g_acc.to(f32))
        o.mom_out, o.z_next, o.kin_out = begin(zs, gs, c.noise.to(f32), s)
    return o

"""TEST INFRASTRUCTURE (CPU; float64 and float32): the Metropolis-adjusted Langevin step of include/lsnf_flow_mcmc.h restated on
oracle.flow_oracle (flow_log_prob, grad_neg_sum_ll_wrt_z) and oracle.philox_oracle (philox4x32_10).

Target p(z) ~ exp(-U(z)), U = e(z) - ll(z); the "generator" is the closed-form quadratic e(z) = 1/2 |A (z - t)|^2 (`Quadratic`; None =
the prior alone).  One call DECIDES a proposal against the kept state (z_acc, grad_acc, u_acc) and PROPOSES the next:
    g_prop = grad e(z_prop) + grad(-ll)(z_prop),  U_prop = e(z_prop) - ll(z_prop),  d = z_prop - z_acc,  coef = s^2 / 2
    A = sum_c (coef g_prop - d)^2,  Bq = sum_c (d + coef grad_acc)^2,  log_alpha = u_acc - U_prop - (A - Bq) / (2 s^2)
    accept iff ln(u) < log_alpha;  z_next = z_state - coef g_state + s xi
The uniform of the in-kernel generator is restated with its fp32 arithmetic in np.float32 (`uniform_draws`)."""
import numpy as np
import torch

from oracle import flow_oracle as O
from oracle.philox_oracle import philox4x32_10

_MASK = np.uint64(0xFFFFFFFF)


def uniform_draws(B, seed, offset=0, row0=0):
    """(B,) np.float32: u = ((x0 >> 8) + 0.5) * 2^-24 in fp32, x0 = word 0 of Philox4x32-10 at counter
    (2 << 16, row_lo, offset_lo, offset_hi ^ row_hi), key (seed_lo, seed_hi), row = row0 + sample."""
    rows = np.arange(B, dtype=np.uint64) + np.uint64(row0)
    c3 = np.uint64((offset >> 32) & 0xFFFFFFFF) ^ (rows >> np.uint64(32))
    x0 = philox4x32_10(np.uint64(2 << 16), rows & _MASK, np.uint64(offset & 0xFFFFFFFF), c3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return ((x0 >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


class Quadratic:
    """e(z) = 1/2 |A (z - t)|^2 per row, grad e = A^T A (z - t); A (nz, nz) and t (nz) float64, evaluated in z's dtype."""

    def __init__(self, nz, scale, seed):
        g = torch.Generator().manual_seed(seed)
        self.A = scale * torch.randn(nz, nz, generator=g, dtype=torch.float64)
        self.t = torch.randn(nz, generator=g, dtype=torch.float64)

    def __call__(self, z):
        A, t = self.A.to(z.dtype), self.t.to(z.dtype)
        r = (z - t) @ A.T
        return 0.5 * (r * r).sum(1), r @ A


def potential(p, z, quad, dtype):
    """(U, grad U, e, grad e, ll) at the rows z, computed in `dtype`."""
    q, zz = O.to_dtype(p, dtype), z.to(dtype)
    ll = O.flow_log_prob(q, zz)[2].detach()
    gf = O.grad_neg_sum_ll_wrt_z(q, zz)
    if quad is None:
        e, ge = torch.zeros_like(ll), torch.zeros_like(zz)
    else:
        e, ge = quad(zz)
    return e - ll, ge + gf, e, ge, ll


def coef_of(s, dtype):
    """0.5 s^2 as the kernel forms it (fp32: two roundings) or exactly."""
    if dtype == torch.float32:
        return float(np.float32(0.5) * np.float32(s) * np.float32(s))
    return 0.5 * s * s


def decide(z_acc, g_acc, u_acc, z_prop, g_prop, U_prop, u, s):
    """(log_alpha, accept, A, Bq) of one decision, in the tensors' dtype; u (B,) in (0, 1)."""
    dtype = z_prop.dtype
    coef = coef_of(s, dtype)
    d = z_prop - z_acc
    A = ((coef * g_prop - d) ** 2).sum(1)
    Bq = ((d + coef * g_acc) ** 2).sum(1)
    two_s2 = float(np.float32(2.0) * np.float32(s) * np.float32(s)) if dtype == torch.float32 else 2.0 * s * s
    la = (u_acc - U_prop) - (A - Bq) / two_s2
    return la, torch.log(u.to(torch.float64)) < la.to(torch.float64), A, Bq


def propose(z_state, g_state, noise, s):
    return z_state - coef_of(s, z_state.dtype) * g_state + s * noise.to(z_state.dtype)


class Step:
    """One call of the teacher-forcing record: what the device is given (the float64 state BEFORE the call, the proposal, grad_g,
    energy_g, noise, uniform) and the float64 answers (log_alpha, accept, A, Bq, the state after, z_next)."""


def smooth_proposal(p, z_state, g_state, noise, s, redraw, margin=2e-5, max_rounds=100):
    """The proposal from (z_state, g_state) with `noise`; redraw (a torch.Generator, or None): rows whose proposal lands within
    `margin` of a ReLU kink (oracle.relu_margin, where d ll/dz is discontinuous) get a new noise row from it, IN PLACE in `noise`,
    until none does -- oracle.smooth_batch's rule, applied to the proposals."""
    z_next = propose(z_state, g_state, noise.to(torch.float64), s)
    if redraw is None:
        return z_next
    bad = torch.nonzero(O.relu_margin(p, z_next.float()) <= margin).flatten()
    for _ in range(max_rounds):
        if bad.numel() == 0:
            return z_next
        noise[bad] = torch.randn(int(bad.numel()), noise.shape[1], generator=redraw, dtype=noise.dtype)
        z_next[bad] = propose(z_state[bad], g_state[bad], noise[bad].to(torch.float64), s)
        bad = bad[O.relu_margin(p, z_next[bad].float()) <= margin]
    raise RuntimeError(f"smooth_proposal: {bad.numel()} proposals still within {margin} of a ReLU kink after {max_rounds} redraws")


def chain(p, z0, quad, s, noises, uniforms, redraw=None):
    """The float64 chain from z0 (B, nz): call 0 starts it (every row accepted) and proposes with noises[0]; call j >= 1 decides
    with uniforms[j] and proposes with noises[j] (None: the last call only decides).  redraw: see smooth_proposal (the noises
    are then updated in place).  Returns the list of `Step` records of calls 1 .. len(noises) - 1 and the final state
    (z, grad, U)."""
    f64 = torch.float64
    z_acc = z0.to(f64)
    u_acc, g_acc, _, _, _ = potential(p, z_acc, quad, f64)
    z_prop = smooth_proposal(p, z_acc, g_acc, noises[0], s, redraw)
    steps = []
    for j in range(1, len(noises)):
        st = Step()
        st.z_acc, st.g_acc, st.u_acc, st.z_prop = z_acc, g_acc, u_acc, z_prop
        U_prop, g_prop, st.e, st.ge, st.ll = potential(p, z_prop, quad, f64)
        st.U_prop, st.g_prop, st.u = U_prop, g_prop, uniforms[j]
        st.la, st.acc, st.A, st.Bq = decide(z_acc, g_acc, u_acc, z_prop, g_prop, U_prop, uniforms[j], s)
        a = st.acc[:, None]
        z_acc, g_acc, u_acc = torch.where(a, z_prop, z_acc), torch.where(a, g_prop, g_acc), torch.where(st.acc, U_prop, u_acc)
        st.z_after, st.g_after, st.u_after = z_acc, g_acc, u_acc
        st.noise = noises[j]
        st.z_next = None if noises[j] is None else smooth_proposal(p, z_acc, g_acc, noises[j], s, redraw)
        z_prop = st.z_next
        steps.append(st)
    return steps, (z_acc, g_acc, u_acc)


def log_alpha32(p, st, quad, s):
    """The fp32 restatement of one recorded decision, from the fp32 casts the device is given (the potential at the proposal is
    recomputed in fp32; grad_g / energy_g are the casts of the float64 ones, as the device gets them)."""
    f32 = torch.float32
    q, zp = O.to_dtype(p, f32), st.z_prop.to(f32)
    ll = O.flow_log_prob(q, zp)[2].detach()
    g_prop = st.ge.to(f32) + O.grad_neg_sum_ll_wrt_z(q, zp)
    U_prop = st.e.to(f32) - ll
    return decide(st.z_acc.to(f32), st.g_acc.to(f32), st.u_acc.to(f32), zp, g_prop, U_prop, st.u, s)[0]

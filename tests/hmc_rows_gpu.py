"""TEST INFRASTRUCTURE (GPU): what tests/test_gpu_hmc_rows.py (`lsnf_hmc_step_rows`, the chain on z) and tests/test_gpu_rhmc_rows.py
(`lsnf_reverse_hmc_step_rows`, the chain on eps) check, written once for both.  A `Space` holds what differs: the scalar tests' module
(tests/test_gpu_hmc.py or test_gpu_rhmc.py -- its cases, teacher-forcing records, plans and `state_for` are reused, and shared with it in a
whole-suite run through its caches), the names of a record's point and next point, and how a call is made.  Nothing here compares
against float64 but the adaptation arithmetic: everything else is bit identity with the scalar call or the device against itself."""
import numpy as np
import torch

import hmc_rows_restated as R

FIELDS = ("z", "grad", "energy", "mom", "kin")
C3, C5, TINY = (128, 64, 5, 1), (100, 128, 5, 1), (8, 4, 5, 1)            # tests/test_gpu_reverse_keep.py's
# Per-row against scalar.  By the dispatch rule (16 rows per workgroup up to 4096 rows, 32 up to 8192, then 64; <HT, WT> by the
# geometry) these launch every instantiation of a per-row kernel: C3 <2, 2> at ST 1 / 2 / 4, TINY <1, 1> at ST 1 / 2 / 4, C5 <2, 4> at
# ST 1 / 2.
IDENTITY = [C3 + (B,) for B in (1, 17, 33, 100, 4100, 8200, 16400)] + [TINY + (B,) for B in (33, 4100, 8200)] + \
           [C5 + (33,), C5 + (4100,), (66, 33, 2, 1, 33), (20, 12, 5, 0, 33)]
ARITHMETIC = [c for c in IDENTITY if c[4] <= 100]
fig = lambda t: t.max().item() if t.numel() else 0.0


def bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Space:
    """name "z" | "eps"; T: the scalar tests' module."""

    def __init__(self, name, T):
        self.name, self.T = name, T

    def step_of(self, c):
        return c.s                                           # the case's fp32 step (the module's step_of of its geometry)

    def point(self, r):
        return r.z_prop if self.name == "z" else r.e_prop

    def proposes(self, r):
        return (r.z_next if self.name == "z" else r.e_next) is not None

    def run(self, lsnf, s, r, step, noise, uniform, rows=slice(None), state=None, adapt=None, propose=True):
        """The recorded call r on its rows from its inputs' casts at `step` (a float: the scalar wrapper; an HmcRowSteps: the per-row
        one): (state after, [next point, accepted, log_alpha])."""
        F, dev = lsnf.flow, s.dev
        cut = lambda t: None if t is None else t[rows].float().to(dev).contiguous()
        state = self.T.state_for(lsnf, s, r, rows) if state is None else state
        per_row = isinstance(step, F.HmcRowSteps)
        kw = dict(phase=r.phase, uniform=uniform, propose=propose)
        if per_row:
            kw["adapt"] = adapt
        point = cut(self.point(r))
        if self.name == "z":
            fn = F.hmc_step_rows if per_row else F.hmc_step
            out = fn(s.plan, point, cut(r.ge), cut(r.e), state, noise, step, **kw)[:3]
        else:
            saved, act = self.T.stash_at(lsnf, s.plan, point)
            fn = F.reverse_hmc_step_rows if per_row else F.reverse_hmc_step
            out = fn(s.plan, point, saved, act, cut(r.ge), cut(r.e), state, noise, step, **kw)
        return state, list(out)

    def end_calls(self, c):
        return [r for r in c.calls if r.phase == "end"]


def flat(res):
    state, out = res
    return [getattr(state, f) for f in FIELDS] + [t for t in out if t is not None]


def three_steps(lsnf, c, B, dev):
    """The three step values cycled over the rows (the case's, 0.5 x and 1.25 x of it, as the fp32 numbers the kernels see) and the
    HmcRowSteps holding them."""
    vals = [float(np.float32(v * c.s)) for v in (1.0, 0.5, 1.25)]
    step = torch.tensor([vals[b % 3] for b in range(B)], dtype=torch.float32)
    return vals, lsnf.flow.new_hmc_row_steps(B, dev, step)


def draws(lsnf, sp, c, r, how, dev, propose, rows=slice(None), row0=0):
    """(noise, uniform) of a call: the record's tensors (an end call that proposes where the record did not: the init call's noise), or
    a PhiloxNoise."""
    if r.phase == "inner":
        return None, None
    if how == "philox":
        return lsnf.flow.PhiloxNoise(11, 5, row0), None
    noise = (r.noise if r.noise is not None else c.calls[0].noise)[rows].float().to(dev).contiguous() if propose else None
    return noise, None if r.u is None else r.u[rows].float().to(dev).contiguous()


# ---- 1 ----
def check_per_row_is_the_scalar_call(lsnf, sp, s):
    c, dev, B = s.c, s.dev, s.c.B
    end = next(r for r in c.calls if r.phase == "end")
    forms = [(c.calls[0], True), (c.calls[1], True), (end, True), (end, False)]
    for r, propose in forms:
        for how in ("tensors", "philox"):
            vals, steps = three_steps(lsnf, c, B, dev)
            before = (steps.step.clone(), steps.adapt.clone())
            noise, uniform = draws(lsnf, sp, c, r, how, dev, propose)
            got = flat(sp.run(lsnf, s, r, steps, noise, uniform, propose=propose))
            assert bits(steps.step, before[0]) and bits(steps.adapt, before[1])                  # only an adapting end call writes them
            for i, v in enumerate(vals):
                ref = flat(sp.run(lsnf, s, r, v, noise, uniform, propose=propose))
                pick = torch.arange(B, device=dev) % 3 == i
                assert len(got) == len(ref)
                for k, (a, b) in enumerate(zip(got, ref)):
                    # (NaN sentinels of state the call must not touch compare as bits too)
                    assert bits(a[pick], b[pick]), f"{sp.name} {c.geo} B{B} {r.phase} propose={propose} {how}: output {k} differs at step {v}"
            if B >= 3 and r.phase != "inner" and propose:                                          # the three steps give three different next points
                assert not bits(got[-3][0::3][: B // 3], flat(sp.run(lsnf, s, r, vals[1], noise, uniform, propose=propose))[-3][0::3][: B // 3])


# ---- 2 ----
def adapt_state(steps, count, dev):
    """Put the rows of `steps` at `count` earlier updates: a running average and an hbar of both signs, of the size they have there."""
    B = steps.step.shape[0]
    if count:
        g = torch.Generator().manual_seed(100 + count)
        steps.adapt[:, 0] = (torch.log(steps.step.cpu()) + 0.3 * torch.randn(B, generator=g)).to(dev)
        steps.adapt[:, 1] = (0.1 * torch.randn(B, generator=g) / np.sqrt(count)).to(dev)
        steps.adapt[:, 2] = float(count)
    return steps


def check_adaptation_arithmetic(lsnf, sp, s):
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    da = R.DualAvg()
    for r in sp.end_calls(c):
        propose = sp.proposes(r)
        noise, uniform = draws(lsnf, sp, c, r, "tensors", dev, propose)
        for mode in ("update", "last"):
            for count in (0, 1, 50):
                _, plain = three_steps(lsnf, c, B, dev)
                ref_state, ref_out = sp.run(lsnf, s, r, adapt_state(plain, count, dev), noise, uniform, propose=propose)
                _, steps = three_steps(lsnf, c, B, dev)
                adapt_state(steps, count, dev)
                old_step, old_adapt = steps.step.clone(), steps.adapt.clone()
                state, out = sp.run(lsnf, s, r, steps, noise, uniform, propose=propose, adapt=mode)
                tag = f"[{sp.name} rows] {c.geo} B{B} end (propose={propose}) {mode} count={count}"
                # the trajectory is finished and decided at the old step
                assert bits(out[1], ref_out[1]) and bits(out[2], ref_out[2])
                for f in ("z", "grad", "energy", "kin"):
                    assert bits(getattr(state, f), getattr(ref_state, f)), f"{tag}: state.{f}"
                # the update, against float64 applied to the device's own log_alpha
                la = out[2].cpu()
                ad64, s64 = R.dual_average(old_adapt.cpu().double(), la.double(), da, mode == "last")
                ad32, s32 = R.dual_average(old_adapt.cpu(), la, da, mode == "last", dtype=torch.float32)
                scale = R.update_scale(ad64, da)
                amp = torch.sqrt(ad64[:, 2]) / da.gamma                                           # hbar enters the log step times this
                errs = lambda ad, st: torch.stack([(ad[:, 0].double() - ad64[:, 0]).abs(), amp * (ad[:, 1].double() - ad64[:, 1]).abs(),
                                                   (st.double() / s64 - 1.0).abs()])
                own = errs(ad32, s32).max(0).values
                bound, wide = sp.T.widened(1e-5 * scale, own)
                err = errs(steps.adapt.cpu(), steps.step.cpu()).max(0).values
                print(f"{tag}: worst update error / bound = {fig(err / bound):.3f} ({wide} rows widened by the fp32 restatement, whose worst is "
                      f"{fig(own / (1e-5 * scale)):.3f}), new steps {steps.step.min().item():.3g} .. {steps.step.max().item():.3g}")
                assert bool((err <= bound).all())
                assert bits(steps.adapt[:, 2], old_adapt[:, 2] + 1.0) and bits(steps.adapt[:, 3], old_adapt[:, 3])
                assert bool(torch.isfinite(steps.adapt).all()) and bool((steps.step > 0).all())
                if count == 0:                               # w = 1: the average is the first iterate, and "last" writes it
                    assert bool(((torch.log(steps.step.double()) - steps.adapt[:, 0].double()).abs() <= 1e-5 * scale.to(dev)).all())
                if not propose:                              # nothing begun: the full-step momentum at the old step, as without adaptation
                    assert out[0] is None and bits(state.mom, ref_state.mom)
                    continue
                # the next trajectory begins at the new step: fp32, the header's operations in the header's order, nothing contracted
                sn = steps.step[:, None]
                ph = noise - (0.5 * sn) * state.grad
                assert bits(state.mom, ph), f"{tag}: mom is not xi - (0.5 s') g_state"
                assert bits(out[0], state.z + sn * ph), f"{tag}: the next point is not z_state + s' ph"
                assert not bits(steps.step, old_step)


# ---- 3 ----
def check_rows_do_not_depend_on_the_batch(lsnf, sp, s):
    """The first 33 rows of the case's batch against 33 rows alone (another workgroup shape), and against two shards with their row0."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = next(x for x in c.calls if x.phase == "end")

    def go(rows, row0, mode):
        n = len(range(*rows.indices(B)))
        _, whole = three_steps(lsnf, c, B, dev)
        adapt_state(whole, 7, dev)
        steps = F.HmcRowSteps(whole.step[rows].clone(), whole.adapt[rows].clone())
        res = sp.run(lsnf, s, r, steps, F.PhiloxNoise(99, 7, row0), None, rows=rows, propose=True, adapt=mode)
        assert steps.step.shape == (n,)
        return flat(res) + [steps.step, steps.adapt]
    for mode in ("update", "last"):
        whole, part = go(slice(0, B), 0, mode), go(slice(0, 33), 0, mode)
        lo, hi = go(slice(0, 20), 0, mode), go(slice(20, 33), 20, mode)
        for a, b, x, y in zip(whole, part, lo, hi):
            assert bits(a[:33], b) and bits(b, torch.cat([x, y]))
        wrong = go(slice(20, 33), 0, mode)
        assert not bits(wrong[5], hi[5])                     # (the draws are a function of the global row)


# ---- 4 ----
def check_a_nan_row(lsnf, sp, s):
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = sp.end_calls(c)[0]
    da = R.DualAvg()
    bad, keep = 18, torch.arange(B, device=dev) != 18

    def steps_at_50():
        """Rows that have settled at their step: mu and the average at log(step), hbar 0, 50 updates behind them."""
        _, st = three_steps(lsnf, c, B, dev)
        st.adapt[:, 0] = torch.log(st.step); st.adapt[:, 1] = 0.0; st.adapt[:, 2] = 50.0; st.adapt[:, 3] = torch.log(st.step)
        return st
    rng = F.PhiloxNoise(3, 4, 0)
    clean_steps = steps_at_50()
    clean = flat(sp.run(lsnf, s, r, clean_steps, rng, None, propose=True, adapt="update")) + [clean_steps.step, clean_steps.adapt]
    steps = steps_at_50()
    old = steps.step.clone()
    state = sp.T.state_for(lsnf, s, r)
    state.mom[bad] = float("nan")
    got_state, out = sp.run(lsnf, s, r, steps, rng, None, state=state, propose=True, adapt="update")
    got = flat((got_state, out)) + [steps.step, steps.adapt]
    assert out[1][bad].item() == 0.0 and bool(torch.isnan(out[2][bad]))
    # a NaN log_alpha counts as a = 0: the row's step shrinks, by the float64 update at a = 0
    ad64, s64 = R.dual_average(torch.tensor([[np.log(old[bad].item()), 0.0, 50.0, np.log(old[bad].item())]], dtype=torch.float64),
                               torch.tensor([float("nan")], dtype=torch.float64), da, False)
    assert steps.step[bad].item() < old[bad].item() and abs(steps.step[bad].item() / s64.item() - 1.0) <= 1e-5 * R.update_scale(ad64, da).item()
    assert bool(torch.isfinite(steps.adapt[bad]).all()) and bool(torch.isfinite(out[0][bad]).all()) and bool(torch.isfinite(got_state.mom[bad]).all())
    for a, b in zip(got, clean):
        assert bits(a[keep], b[keep])                        # every other row: the bits of the run without the NaN
    # rows pinned at step_min / step_max stay there, finite
    _, pinned = three_steps(lsnf, c, B, dev)
    lo, hi = 0.4 * c.s, 1.3 * c.s
    pinned = F.HmcRowSteps(pinned.step, pinned.adapt, step_min=lo, step_max=hi)
    pinned.adapt[:, 0], pinned.adapt[:, 2] = torch.log(pinned.step), 20.0      # (the running average inside the clamp's range, like every iterate)
    pinned.adapt[0::2, 1], pinned.adapt[1::2, 1] = 1e4, -1e4       # hbar far on either side: the log step is clamped
    for mode in ("update", "update", "last"):
        sp.run(lsnf, s, r, pinned, rng, None, propose=True, adapt=mode)
        assert bool(torch.isfinite(pinned.adapt).all()) and bool(torch.isfinite(pinned.step).all())
        if mode == "update":
            assert bool(((pinned.step[0::2] / lo - 1.0).abs() <= 1e-5).all()) and bool(((pinned.step[1::2] / hi - 1.0).abs() <= 1e-5).all())
    assert bool((pinned.step >= lo * (1 - 1e-5)).all()) and bool((pinned.step <= hi * (1 + 1e-5)).all())


# ---- 6: the samplers' target in the warm-up experiment's configuration ----
class LinearG(torch.nn.Module):
    """netG(z) = A z: with x = A t and sigma = 1 the sampler's energy |x - G(z)|^2 / (2 sigma^2) is hmc_restated.Quadratic's 1/2 |A (z - t)|^2."""

    def __init__(self, quad):
        super().__init__()
        self.A = torch.nn.Parameter(quad.A.float(), requires_grad=False)

    def forward(self, z):
        return z.flatten(1) @ self.A.T


def warmup_problem(lsnf, K, dev, space):
    """(net, netG, x, start (B, nz, 1, 1), first steps (B)) of hmc_rows_restated's warm-up experiment on the device."""
    from oracle import flow_oracle as O
    nz, B = R.WARMUP_GEO[0], R.WARMUP_B
    p, quad = R.warmup_target(space)
    net = K.module_of(lsnf, p, dev, False)
    netG = LinearG(quad).to(dev)
    x = (quad.t @ quad.A.T).float().to(dev).expand(B, nz).contiguous()
    z0, _ = O.smooth_batch(p, B, nz, seed=2000)
    if space == "eps":
        z0 = torch.randn(B, nz, generator=torch.Generator().manual_seed(2000))
    return net, netG, x, z0.float().view(B, nz, 1, 1).to(dev), R.warmup_start(space).float().to(dev)


def check_frozen_phase_acceptance(sp, rate, steps):
    band, half = R.BAND[sp.name], R.BAND_HALF[sp.name]
    m, big, small = rate.mean().item(), rate[0::2].mean().item(), rate[1::2].mean().item()
    print(f"[{sp.name} rows] sampler, warm-up {R.WARMUP_K} + {R.FROZEN_K} trajectories, B={R.WARMUP_B}: frozen-phase acceptance {m:.4f} (band "
          f"{band}), rows started at 10 x: {big:.4f}, at 0.1 x: {small:.4f} (band {half}), frozen steps {steps.step.min().item():.3f} .. "
          f"{steps.step.max().item():.3f}")
    assert band[0] <= m <= band[1] and half[0] <= big <= half[1] and half[0] <= small <= half[1]
    assert bool((steps.adapt[:, 2] == R.WARMUP_K).all())

"""TEST INFRASTRUCTURE (GPU): what tests/test_gpu_hmc_metric.py (`lsnf_hmc_step_metric`, the chain on z) and
tests/test_gpu_rhmc_metric.py (`lsnf_reverse_hmc_step_metric`, the chain on eps) check, written once for both on tests/hmc_rows_gpu.py's
`Space`: the scalar tests' cases, teacher-forcing records, plans and `state_for` are reused (and shared with them in a whole-suite run
through their caches).  Bit identities are against the per-row call or the device against itself; float64 enters in the teacher-forced
calls at a column-varying scale, in the fold and in the close.

A teacher-forced call is given a recorded point of the scalar chain (clear of a ReLU kink, with its float64 potential) and ANY scale:
one device call sees one point, so the float64 answer of that call at scale sd is the header's lines applied to the record's float64
state, momentum and gradient (`expected`); the gates are the scalar modules' own, with sd inside the magnitudes they are made of."""
import types

import numpy as np
import torch

import chain_geometries as G
import hmc_restated as H
import hmc_rows_gpu as HG
import hmc_rows_restated as R
import hmc_metric_restated as MR

bits, fig, FIELDS = HG.bits, HG.fig, HG.FIELDS
C3, C5, TINY = HG.C3, HG.C5, HG.TINY
IDENTITY = HG.IDENTITY                       # every instantiation of a metric kernel, by the dispatch rule
POWER_OF_TWO = HG.ARITHMETIC                 # IDENTITY's cases of at most 100 rows
COLUMN = G.CASES + G.LARGE                   # the nine geometries of tests/chain_geometries.py at 33 rows, (66, 33) at 4100, (10, 40) at 8200
FORMS = G.FORMS
WINDOW = [C3 + (33,), TINY + (33,), (66, 33, 2, 1, 33), (10, 40, 2, 1, 33)]        # fold and close: whole tiles, TINY, a ragged half, scalar row access
METRIC = ("scale", "mean", "m2", "count")


def column_scale(B, nz, seed=0, spread=3.0):
    """2^U(-spread, spread) per row and column, as the fp32 numbers the kernels see."""
    g = torch.Generator().manual_seed(4000 + seed)
    return torch.exp2(2.0 * spread * torch.rand(B, nz, generator=g) - spread).float()


def new_metric(lsnf, s, B, scale=1.0, sentinel=True, **reg):
    """An HmcRowMetric of B rows on the case's device; sentinel: the accumulators hold NaN (a call that does not fold must not touch
    them, and NaN compares as bits)."""
    m = lsnf.flow.new_hmc_row_metric(s.plan, B, s.dev, scale)
    if sentinel:
        m.mean.fill_(float("nan")); m.m2.fill_(float("nan")); m.count.fill_(float("nan"))
    for k, v in reg.items():
        setattr(m, k, v)
    return m


def same_steps(lsnf, sp, c, B, dev, count=0):
    """tests/hmc_rows_gpu.py's three steps cycled over the rows, `count` earlier updates behind them."""
    return HG.adapt_state(HG.three_steps(lsnf, c, B, dev)[1], count, dev)


def run(lsnf, sp, s, r, steps, metric, noise, uniform, rows=slice(None), state=None, adapt=None, window=None, propose=True, inplace=False,
        point=None, ge="record", e="record"):
    """The recorded call r on its rows from its inputs' casts through the metric wrapper: (state after, [next point, accepted,
    log_alpha])."""
    F, dev = lsnf.flow, s.dev
    cut = lambda t: None if t is None else t[rows].float().to(dev).contiguous()
    state = sp.T.state_for(lsnf, s, r, rows) if state is None else state
    kw = dict(phase=r.phase, uniform=uniform, propose=propose, adapt=adapt, window=window, inplace=inplace)
    point = cut(sp.point(r)) if point is None else point
    ge = cut(r.ge) if isinstance(ge, str) else ge
    e = cut(r.e) if isinstance(e, str) else e
    if sp.name == "z":
        out = F.hmc_step_metric(s.plan, point, ge, e, state, noise, steps, metric, **kw)[:3]
    else:
        saved, act = sp.T.stash_at(lsnf, s.plan, point)
        out = F.reverse_hmc_step_metric(s.plan, point, saved, act, ge, e, state, noise, steps, metric, **kw)
    return state, list(out)


def flat(res, steps, metric):
    return HG.flat(res) + [steps.step, steps.adapt] + [getattr(metric, f) for f in METRIC]


def clone_metric(lsnf, m):
    return lsnf.flow.HmcRowMetric(m.scale.clone(), m.mean.clone(), m.m2.clone(), m.count.clone(), m.n0, m.var0, m.scale_min, m.scale_max)


def untouched(m, before, fields=METRIC):
    return all(bits(getattr(m, f), getattr(before, f)) for f in fields)


def forms_of(sp, c):
    """(record, propose) of the four phases: init, inner, an end call that begins the next trajectory, one that does not."""
    end = next(r for r in c.calls if r.phase == "end")
    return [(c.calls[0], True), (c.calls[1], True), (end, True), (end, False)]


# ---- 1 ----
def check_unit_scale_is_the_per_row_call(lsnf, sp, s):
    c, dev, B = s.c, s.dev, s.c.B
    for r, propose in forms_of(sp, c):
        for how in ("tensors", "philox"):
            for adapt in (None, "update") if r.phase == "end" else (None,):
                noise, uniform = HG.draws(lsnf, sp, c, r, how, dev, propose)
                ref_steps = same_steps(lsnf, sp, c, B, dev, 7)
                ref = HG.flat(sp.run(lsnf, s, r, ref_steps, noise, uniform, propose=propose, adapt=adapt)) + [ref_steps.step, ref_steps.adapt]
                steps, metric = same_steps(lsnf, sp, c, B, dev, 7), new_metric(lsnf, s, B)
                before = clone_metric(lsnf, metric)
                got = HG.flat(run(lsnf, sp, s, r, steps, metric, noise, uniform, propose=propose, adapt=adapt)) + [steps.step, steps.adapt]
                assert len(got) == len(ref)
                for k, (a, b) in enumerate(zip(got, ref)):
                    assert bits(a, b), f"{sp.name} {c.geo} B{B} {r.phase} propose={propose} {how} adapt={adapt}: output {k} differs"
                assert untouched(metric, before)             # scale, mean, m2 and count are written by folding calls alone


# ---- 2 ----
def check_power_of_two_scale_is_the_step_times_it(lsnf, sp, s):
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    k = torch.tensor([(-2.0, 0.0, 3.0)[b % 3] for b in range(B)])
    sd = torch.exp2(k)[:, None].expand(B, c.nz).contiguous()
    for r, propose in forms_of(sp, c):
        for how in ("tensors", "philox"):
            noise, uniform = HG.draws(lsnf, sp, c, r, how, dev, propose)
            scaled = F.new_hmc_row_steps(B, dev, torch.full((B,), c.s) * torch.exp2(k))       # (an exact scaling of the fp32 step)
            ref = HG.flat(sp.run(lsnf, s, r, scaled, noise, uniform, propose=propose))
            steps, metric = F.new_hmc_row_steps(B, dev, c.s), new_metric(lsnf, s, B, sd)
            got = HG.flat(run(lsnf, sp, s, r, steps, metric, noise, uniform, propose=propose))
            assert len(got) == len(ref)
            for j, (a, b) in enumerate(zip(got, ref)):
                assert bits(a, b), f"{sp.name} {c.geo} B{B} {r.phase} propose={propose} {how}: output {j} differs"
            if B >= 3 and propose:                           # (and the scale is not ignored: at 2^3 the next point is another)
                plain = HG.flat(sp.run(lsnf, s, r, F.new_hmc_row_steps(B, dev, c.s), noise, uniform, propose=propose))
                assert bits(got[5][1::3], plain[5][1::3]) and not bits(got[5][2::3], plain[5][2::3])


# ---- 3 ----
def acc_point(sp, r):
    return r.z_acc if sp.name == "z" else r.e_acc


def expected(sp, r, sd, s, dtype=torch.float64, acc=None):
    """The header's lines for the recorded call r at scale sd in `dtype`: float64 from the record's float64 quantities, or fp32 from
    their casts and the fp32 restatement's potential (r.o32) -- the begin then from the float64 decision `acc`, as the device is
    compared on decided rows.  Fields: la, acc, kinL, mom, nxt, kin (None where the call has none), xs / gs the state after."""
    f64 = dtype == torch.float64
    t = lambda v: None if v is None else v.to(dtype)
    x, g, U = t(sp.point(r)), t(r.g if f64 else r.o32.g), t(r.U_prop if f64 else r.o32.U_prop)
    sd = sd.to(dtype)
    o = types.SimpleNamespace(la=None, acc=None, kinL=None, mom=None, nxt=None, kin=None)
    if r.phase == "inner":
        o.mom, o.nxt = MR.inner(x, t(r.mom_in), g, s, sd)
        return o
    if r.phase == "end":
        o.mom, o.kinL = MR.end(t(r.mom_in), g, s, sd)
        o.la = H.log_alpha(t(r.u_acc), U, t(r.kin_in), o.kinL)
        o.acc = H.accept(o.la, r.u) if acc is None else acc
        a = o.acc[:, None]
        o.xs, o.gs = torch.where(a, x, t(acc_point(sp, r))), torch.where(a, g, t(r.g_acc))
    else:
        o.acc, o.xs, o.gs = torch.ones(x.shape[0], dtype=torch.bool), x, g
    if r.noise is not None:
        o.mom, o.nxt, o.kin = MR.begin(o.xs, o.gs, r.noise.to(dtype), s, sd)
    return o


def gates(sp, T, r, sd, s):
    """The float64 answer of the call at scale sd with the scalar module's gates around it (tests/test_gpu_hmc.py Case)."""
    o, o32 = expected(sp, r, sd, s), None
    o32 = expected(sp, r, sd, s, torch.float32, acc=o.acc)
    B, sd64 = sd.shape[0], sd.double()
    o.decided = r.smooth
    if r.phase == "end":
        o.scale = r.u_acc.abs() + r.U_prop.abs() + r.kin_in + o.kinL
        o.gate = torch.maximum(1e-5 * o.scale, 3.0 * (o32.la.double() - o.la).abs())
        o.decided = r.smooth & ((o.la - torch.log(r.u.double())).abs() > o.gate)
    if o.mom is not None:
        src = r.noise.double() if r.noise is not None else r.mom_in
        gg = o.gs if r.noise is not None else r.g
        o.mom_bound, o.mom_wide = T.widened(1e-5 * (src.norm(dim=1) + s * (sd64 * gg).norm(dim=1)), (o32.mom.double() - o.mom).norm(dim=1))
    if o.nxt is not None:
        o.nxt_bound, o.nxt_wide = T.widened(torch.full((B,), 1e-5, dtype=torch.float64), T.rel_rows(o32.nxt, o.nxt))
    if o.kin is not None:
        o.kin_bound, o.kin_wide = T.widened(1e-5 * o.kin, (o32.kin.double() - o.kin).abs())
    return o


def check_column_scale_follows_float64(lsnf, sp, s):
    # 2^U(-3, 3): at steps chosen for a unit scale nearly every such trajectory is rejected, so a second draw, 2^U(-1/2, 1/2), has
    # the device decide both ways
    for spread in (3.0, 0.5):
        column_scale_calls(lsnf, sp, s, column_scale(s.c.B, s.c.nz, 0, spread), spread)


def column_scale_calls(lsnf, sp, s, sd, spread):
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    tag = f"[{sp.name} metric] {c.geo} B{B} scale 2^U(-{spread:g}, {spread:g})"
    for j, r in enumerate(c.device_calls):
        o = gates(sp, sp.T, r, sd, c.s)
        propose = r.noise is not None or r.phase == "inner"
        noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, propose)
        steps, metric = F.new_hmc_row_steps(B, dev, c.s), new_metric(lsnf, s, B, sd)
        state = sp.T.state_for(lsnf, s, r)
        before = sp.T.clone_state(lsnf, state)
        state, (nxt, acc, la) = run(lsnf, sp, s, r, steps, metric, noise, uniform, state=state, propose=propose)
        torch.cuda.synchronize()
        xa, ga, ua, mom, kin = (getattr(state, f).cpu() for f in FIELDS)
        name = f"{tag} call {j} {r.phase}"
        d = o.decided
        if r.phase == "inner":
            assert acc is None and la is None
            for f in ("z", "grad", "energy", "kin"):
                assert bits(getattr(state, f), getattr(before, f))
        else:
            acc_c = acc.cpu()
            assert bool(((acc_c == 1.0) | (acc_c == 0.0)).all())
            if r.phase == "init":
                assert bool((acc_c == 1.0).all()) and bits(la, torch.zeros_like(la))
            else:
                aside = int((~d).sum())
                err = (la.cpu().double() - o.la).abs()
                print(f"{name}: float64 accepts {int(o.acc.sum())}/{B}, set aside {aside} (allowed {c.allowed}), worst |log_alpha - fp64| / gate = "
                      f"{fig((err / o.gate)[r.smooth]):.3f}")
                assert aside <= c.allowed
                assert bool((err <= o.gate)[r.smooth].all())
                assert torch.equal(acc_c[d] == 1.0, o.acc[d])
            yes, no = d & o.acc, d & ~o.acc
            assert bits(xa[yes], sp.point(r).float()[yes])
            if r.phase == "end":
                bz, bg, bu = before.z.cpu(), before.grad.cpu(), before.energy.cpu()
                assert bits(xa[no], bz[no]) and bits(ga[no], bg[no]) and bits(ua[no], bu[no])
        if o.mom is not None:
            e = (mom.double() - o.mom).norm(dim=1)
            print(f"{name}: worst |mom - fp64| / bound = {fig((e / o.mom_bound)[d]):.3f} ({o.mom_wide} rows widened by the fp32 restatement)")
            assert bool((e <= o.mom_bound)[d].all())
        if o.nxt is not None:
            e = sp.T.rel_rows(nxt.cpu(), o.nxt)
            print(f"{name}: worst next-point rel-L2 / bound = {fig((e / o.nxt_bound)[d]):.3f} ({o.nxt_wide} rows widened)")
            assert bool((e <= o.nxt_bound)[d].all())
        else:
            assert nxt is None
        if o.kin is not None:
            e = (kin.double() - o.kin).abs()
            print(f"{name}: worst kin0 error / bound = {fig(e / o.kin_bound):.3f} ({o.kin_wide} rows widened)")
            assert bool((e <= o.kin_bound).all())
            # the begin, to the bit, from the device's own stored state: fp32, the header's operations in the header's order
            st, sdd = steps.step[:, None], metric.scale
            ph = noise - (0.5 * st) * (sdd * state.grad)
            assert bits(state.mom, ph), f"{name}: mom is not xi - (0.5 s) (sd grad_state)"
            assert bits(nxt, state.z + st * (sdd * ph)), f"{name}: the next point is not z_state + s (sd mom)"
        assert bits(metric.scale, sd.to(dev))


def check_forms(lsnf, sp, s):
    """In place, every tensor 4 bytes off a 16-byte boundary and NULL optionals, at a column-varying scale with a closing end call."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    sd = column_scale(B, c.nz, 1)

    def off4(t):
        if t is None:
            return None
        t = t.float().to(dev)
        b = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
        v = b[1: 1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    def window_state(m):
        g = torch.Generator().manual_seed(9)
        m.mean.copy_(torch.randn(B, c.nz, generator=g)); m.m2.copy_(3.0 * torch.rand(B, c.nz, generator=g)); m.count.fill_(3.0)
        return m
    for r, _ in forms_of(sp, c)[:3]:
        end = r.phase == "end"
        kw = dict(adapt="update", window="close") if end else {}
        noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, True)
        fresh = lambda: (same_steps(lsnf, sp, c, B, dev, 5), window_state(new_metric(lsnf, s, B, sd)))
        steps, metric = fresh()
        ref = flat(run(lsnf, sp, s, r, steps, metric, noise, uniform, **kw), steps, metric)
        # in place: the next point over the point
        steps, metric = fresh()
        point = sp.point(r).float().to(dev)
        res = run(lsnf, sp, s, r, steps, metric, noise, uniform, point=point, inplace=True, **kw)
        assert res[1][0].data_ptr() == point.data_ptr()
        assert all(bits(a, b) for a, b in zip(flat(res, steps, metric), ref))
        # every tensor 4 bytes off a 16-byte boundary (the stash and the rows' quads apart: they stay 16-byte aligned)
        steps, metric = fresh()
        steps = F.HmcRowSteps(off4(steps.step), steps.adapt)
        metric = F.HmcRowMetric(off4(metric.scale), off4(metric.mean), off4(metric.m2), off4(metric.count))
        st = sp.T.state_for(lsnf, s, r)
        state = F.HmcState(*(off4(getattr(st, f)) for f in FIELDS))
        res = run(lsnf, sp, s, r, steps, metric, off4(noise), off4(uniform), state=state, point=off4(sp.point(r)), ge=off4(r.ge), e=off4(r.e),
                  inplace=True, **kw)
        assert all(bits(a, b) for a, b in zip(flat(res, steps, metric), ref))
        # NULL gradient and energy are zeros
        rng = None if r.phase == "inner" else F.PhiloxNoise(8, 9, 0)
        both = []
        for gg, e in ((None, None), (torch.zeros(B, c.nz, device=dev), torch.zeros(B, device=dev))):
            steps, metric = fresh()
            both.append(flat(run(lsnf, sp, s, r, steps, metric, rng, None, ge=gg, e=e, **kw), steps, metric))
        assert all(bits(a, b) for a, b in zip(*both))
    steps, metric = fresh()                                  # the scales are an output: they may not be the point
    try:
        run(lsnf, sp, s, r, steps, F.HmcRowMetric(point, metric.mean, metric.m2, metric.count), noise, uniform, point=point)
    except lsnf.LsnfError:
        pass
    else:
        raise AssertionError("scale_rows over the point was not refused")


# ---- 4, 5 ----
def window_at(lsnf, sp, s, state_z, sd=1.0, **reg):
    """A metric whose rows cycle through windows of 0, 1 and 50 folded states: a mean near the row's state and an m2 of the size it
    has there (count 0: an empty window; count 1: m2 = 0)."""
    B, nz, dev = state_z.shape[0], state_z.shape[1], s.dev
    m = new_metric(lsnf, s, B, sd, sentinel=False, **reg)
    g = torch.Generator().manual_seed(77)
    count = torch.tensor([(0.0, 1.0, 50.0)[b % 3] for b in range(B)])
    spread = 0.2 + torch.rand(B, nz, generator=g)
    m.mean.copy_(torch.where(count[:, None] > 0, state_z.cpu() + spread * torch.randn(B, nz, generator=g), torch.zeros(B, nz)))
    m.m2.copy_(torch.where(count[:, None] > 1, count[:, None] * spread * spread, torch.zeros(B, nz)))
    m.count.copy_(count)
    return m


def fold64(mean, m2, count, x):
    """(mean', m2', n) in float64 from the device's own inputs, with the gates: 1e-5 of the magnitudes entering each quantity."""
    mean, m2, count, x = (t.cpu().double() for t in (mean, m2, count, x))
    mn, q, n = MR.fold(mean, m2, count, x)
    d = (x - mean).abs()
    return mn, q, n, 1e-5 * (mean.abs() + d / n[:, None]), 1e-5 * (m2.abs() + d * (x.abs() + mn.abs()))


def check_fold(lsnf, sp, s):
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    tag = f"[{sp.name} metric] {c.geo} B{B} fold"
    for r in sp.end_calls(c):
        propose = sp.proposes(r)
        noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, propose)
        steps, plain_m = F.new_hmc_row_steps(B, dev, c.s), new_metric(lsnf, s, B)
        plain_state, plain = run(lsnf, sp, s, r, steps, plain_m, noise, uniform, propose=propose)
        # from an empty window: the folded point IS the state after the decision -- the proposal on accepted rows, the kept state on
        # rejected ones --, to the bit
        metric = new_metric(lsnf, s, B, sentinel=False)
        state, out = run(lsnf, sp, s, r, steps, metric, noise, uniform, propose=propose, window="fold")
        assert all(bits(a, b) for a, b in zip(HG.flat((state, out)), HG.flat((plain_state, plain))))      # a fold changes nothing else
        accepted = int(out[1].sum().item())
        assert 0 < accepted < B, f"{tag}: the case needs accepted and rejected rows (got {accepted}/{B})"
        point, kept = sp.point(r).float().to(dev), sp.T.state_for(lsnf, s, r).z
        assert bits(state.z, torch.where(out[1][:, None] == 1.0, point, kept))
        assert bits(metric.mean, state.z) and bits(metric.m2, torch.zeros_like(metric.m2)) and bits(metric.count, torch.ones_like(metric.count))
        assert bits(metric.scale, torch.ones_like(metric.scale))
        # from windows of 0, 1 and 50 states: against float64 on the device's own inputs
        metric = window_at(lsnf, sp, s, state.z)
        before = clone_metric(lsnf, metric)
        state, out = run(lsnf, sp, s, r, steps, metric, noise, uniform, propose=propose, window="fold")
        mn, q, n, gm, gq = fold64(before.mean, before.m2, before.count, state.z)
        m32, q32, _ = MR.fold(before.mean.cpu(), before.m2.cpu(), before.count.cpu(), state.z.cpu())
        gm, wm = sp.T.widened(gm.flatten(), (m32.double() - mn).abs().flatten())
        gq, wq = sp.T.widened(gq.flatten(), (q32.double() - q).abs().flatten())
        em, eq = (metric.mean.cpu().double() - mn).abs().flatten(), (metric.m2.cpu().double() - q).abs().flatten()
        ok = gm > 0                                           # (an empty window's zeros: exact, checked below)
        print(f"{tag} (propose={propose}): worst mean error / gate = {fig((em / gm.clamp_min(1e-300))[ok]):.3f} ({wm} entries widened by the fp32 "
              f"restatement), worst m2 error / gate = {fig((eq / gq.clamp_min(1e-300))[gq > 0]):.3f} ({wq} widened)")
        assert bool((em <= gm).all()) and bool((eq <= gq).all())
        assert bits(metric.count, before.count + 1.0) and untouched(metric, before, ("scale",))
        empty = (before.count == 0)
        assert bits(metric.mean[empty], state.z[empty]) and not metric.m2[empty].any()


def check_close(lsnf, sp, s):
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    tag = f"[{sp.name} metric] {c.geo} B{B} close"
    reg = MR.Reg()
    for r in sp.end_calls(c):
        propose = sp.proposes(r)
        noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, propose)
        kept = sp.T.state_for(lsnf, s, r).z
        sd = column_scale(B, c.nz, 2).clamp(0.5, 2.0)
        for mode in (None, "update", "last"):
            steps = same_steps(lsnf, sp, c, B, dev, 7)
            ref_steps, ref_m = same_steps(lsnf, sp, c, B, dev, 7), new_metric(lsnf, s, B, sd)
            ref_state, ref = run(lsnf, sp, s, r, ref_steps, ref_m, noise, uniform, propose=propose, adapt=mode)      # the same call without a window
            metric = window_at(lsnf, sp, s, kept, sd)
            before = clone_metric(lsnf, metric)
            state, out = run(lsnf, sp, s, r, steps, metric, noise, uniform, propose=propose, adapt=mode, window="close")
            name = f"{tag} (propose={propose}, adapt={mode})"
            # the trajectory is finished and decided at the old step and the old scale
            assert bits(out[1], ref[1]) and bits(out[2], ref[2]) and bits(steps.step, ref_steps.step)
            for f in ("z", "grad", "energy", "kin"):
                assert bits(getattr(state, f), getattr(ref_state, f)), f"{name}: state.{f}"
            # sd' against float64 on the device's own inputs; the gate: 1e-5 of sd' and what the fold's gate on m2' moves it by
            mn, q, n, gm, gq = fold64(before.mean, before.m2, before.count, state.z)
            new64 = MR.close(before.scale.cpu(), q, n, reg)
            _, q32, n32 = MR.fold(before.mean.cpu(), before.m2.cpu(), before.count.cpu(), state.z.cpu())
            new32 = MR.close(before.scale.cpu(), q32, n32, reg, dtype=torch.float32)
            wn = (n / (n + 5.0) / (n - 1.0).clamp_min(1.0))[:, None]
            gate = 1e-5 * new64 + wn * gq / (2.0 * new64)
            gate, wide = sp.T.widened(gate.flatten(), (new32.double() - new64).abs().flatten())
            err = (metric.scale.cpu().double() - new64).abs().flatten()
            print(f"{name}: worst |sd' - fp64| / gate = {fig(err / gate):.3f} ({wide} entries widened by the fp32 restatement), scales "
                  f"{metric.scale.min().item():.3g} .. {metric.scale.max().item():.3g}")
            assert bool((err <= gate).all())
            one = (before.count == 0)                        # n < 2: the scale's bits are kept
            assert bool(one.any()) and bits(metric.scale[one], before.scale[one]) and not bits(metric.scale[~one], before.scale[~one])
            for f in ("mean", "m2", "count"):                # exactly zero afterwards
                assert bits(getattr(metric, f), torch.zeros_like(getattr(metric, f))), f"{name}: {f} is not zero"
            # the dual-averaging state: restarted at log(10 s') by "update", the per-row call's with "last"
            if mode == "update":
                assert not bits(steps.step, same_steps(lsnf, sp, c, B, dev, 7).step)
                assert bits(steps.adapt[:, :3], torch.zeros_like(steps.adapt[:, :3]))
                mu = torch.log(10.0 * steps.step.cpu().double())
                e = (steps.adapt[:, 3].cpu().double() - mu).abs()
                print(f"{name}: worst |mu - log(10 s')| / (1e-5 (1 + |mu|)) = {fig(e / (1e-5 * (1.0 + mu.abs()))):.3f}")
                assert bool((e <= 1e-5 * (1.0 + mu.abs())).all())
            else:
                assert bits(steps.adapt, ref_steps.adapt)
            if not propose:                                  # nothing begun: the full-step momentum at the old step and the old scale
                assert out[0] is None and bits(state.mom, ref_state.mom)
                continue
            # the next trajectory begins with sd' and s': fp32, the header's operations in the header's order, nothing contracted
            st, sdd = steps.step[:, None], metric.scale
            ph = noise - (0.5 * st) * (sdd * state.grad)
            assert bits(state.mom, ph), f"{name}: mom is not xi - (0.5 s') (sd' grad_state)"
            assert bits(out[0], state.z + st * (sdd * ph)), f"{name}: the next point is not z_state + s' (sd' mom)"
            assert not bits(state.mom[~one], ref_state.mom[~one])
        # clamped rows sit at scale_min / scale_max
        lo, hi = 0.9, 1.1
        metric = window_at(lsnf, sp, s, kept, sd, scale_min=lo, scale_max=hi)
        before = clone_metric(lsnf, metric)
        run(lsnf, sp, s, r, F.new_hmc_row_steps(B, dev, c.s), metric, noise, uniform, propose=propose, window="close")
        f32 = lambda v: float(np.float32(v))
        closed = metric.scale[before.count > 0]
        assert bool(((closed >= f32(lo)) & (closed <= f32(hi))).all()) and bool((closed == f32(lo)).any()) and bool((closed == f32(hi)).any())


# ---- 6 ----
def check_rows_do_not_depend_on_the_batch(lsnf, sp, s):
    """The first 33 rows of the case's batch against 33 rows alone (another workgroup shape), and against two shards with their row0,
    on an end call that adapts, folds and closes: scale and accumulators among the compared outputs."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = next(x for x in c.calls if x.phase == "end")
    kept = sp.T.state_for(lsnf, s, r).z
    sd = column_scale(B, c.nz, 3)

    def go(rows, row0, mode, window):
        whole, wm = same_steps(lsnf, sp, c, B, dev, 7), window_at(lsnf, sp, s, kept, sd)
        steps = F.HmcRowSteps(whole.step[rows].clone(), whole.adapt[rows].clone())
        metric = F.HmcRowMetric(*(getattr(wm, f)[rows].clone() for f in METRIC))
        res = run(lsnf, sp, s, r, steps, metric, F.PhiloxNoise(99, 7, row0), None, rows=rows, propose=True, adapt=mode, window=window)
        return flat(res, steps, metric)
    for mode, window in (("update", "close"), ("last", "fold"), (None, None)):
        whole, part = go(slice(0, B), 0, mode, window), go(slice(0, 33), 0, mode, window)
        lo, hi = go(slice(0, 20), 0, mode, window), go(slice(20, 33), 20, mode, window)
        for a, b, x, y in zip(whole, part, lo, hi):
            assert bits(a[:33], b) and bits(b, torch.cat([x, y]))
        wrong = go(slice(20, 33), 0, mode, window)
        assert not bits(wrong[5], hi[5])                     # (the draws are a function of the global row)


# ---- 7 ----
def check_a_nan_row(lsnf, sp, s):
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = sp.end_calls(c)[0]
    bad, keep = 18, torch.arange(B, device=dev) != 18
    sd = column_scale(B, c.nz, 4).clamp(0.5, 2.0)
    rng = F.PhiloxNoise(3, 4, 0)
    fresh = lambda: (same_steps(lsnf, sp, c, B, dev, 7), new_metric(lsnf, s, B, sd, sentinel=False))
    steps, metric = fresh()
    clean = flat(run(lsnf, sp, s, r, steps, metric, rng, None, propose=True, adapt="update", window="fold"), steps, metric)
    steps, metric = fresh()
    state = sp.T.state_for(lsnf, s, r)
    state.mom[bad] = float("nan")
    before = sp.T.clone_state(lsnf, state)
    state, out = run(lsnf, sp, s, r, steps, metric, rng, None, state=state, propose=True, adapt="update", window="fold")
    got = flat((state, out), steps, metric)
    assert out[1][bad].item() == 0.0 and bool(torch.isnan(out[2][bad]))
    for f in ("z", "grad", "energy"):
        assert bits(getattr(state, f)[bad], getattr(before, f)[bad])
    # the row folds its KEPT state, and goes on from it with finite numbers
    assert bits(metric.mean[bad], before.z[bad]) and not metric.m2[bad].any() and metric.count[bad].item() == 1.0
    assert bool(torch.isfinite(out[0][bad]).all()) and bool(torch.isfinite(state.mom[bad]).all()) and bool(torch.isfinite(steps.adapt[bad]).all())
    for a, b in zip(got, clean):
        assert bits(a[keep], b[keep])                        # every other row: the bits of the run without the NaN


# ---- 9: the samplers on the experiment's problem ----
def experiment_problem(lsnf, K, dev, space, seed=0):
    """(net, netG, x, start (B, nz, 1, 1)) of hmc_metric_restated's experiment on the device: LinearG with the diagonal A, sigma = 1."""
    nz, B = MR.EXP_GEO[0], MR.EXP_B
    p, quad = MR.experiment_target()
    net = K.module_of(lsnf, p, dev, False)
    netG = HG.LinearG(quad).to(dev)
    x = (quad.t @ quad.A.T).float().to(dev).expand(B, nz).contiguous()
    return net, netG, x, MR.experiment_start(space, seed).float().view(B, nz, 1, 1).to(dev), quad


def check_sampler_figures(sp, rate, steps, metric, quad):
    acc, step, dev = MR.figures(rate.cpu(), steps.step.cpu(), metric.scale.cpu(), quad)
    band = MR.BAND[sp.name]
    print(f"[{sp.name} metric] sampler, warm-up {MR.EXP_W} (windows {MR.EXP_WINDOWS}) + {MR.EXP_FROZEN} trajectories, B={MR.EXP_B}: frozen mean "
          f"acceptance {acc:.4f} (band {band['accept']}), frozen median step {step:.4f} (band {band['step']}), median |log(scale / closed "
          f"form)| {dev:.4f} (band {band['scale']})")
    assert band["accept"][0] <= acc <= band["accept"][1]
    assert band["step"][0] <= step <= band["step"][1]
    assert band["scale"][0] <= dev <= band["scale"][1]
    # every window is closed, and the step adaptation has run since the last close
    assert not metric.count.any() and not metric.mean.any() and not metric.m2.any()
    assert bool((steps.adapt[:, 2] == MR.EXP_W - MR.EXP_WINDOWS[1][-1]).all())

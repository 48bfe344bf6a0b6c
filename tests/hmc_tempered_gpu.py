"""TEST INFRASTRUCTURE (GPU): what tests/test_gpu_hmc_tempered.py (`lsnf_hmc_step_tempered`, the chain on z) and
tests/test_gpu_rhmc_tempered.py (`lsnf_reverse_hmc_step_tempered`, the chain on eps) check, written once for both on
tests/hmc_rows_gpu.py's `Space`: the scalar tests' cases, teacher-forcing records, plans and `state_for` and tests/hmc_metric_gpu.py's
helpers are reused by import.  Bit identities are against the metric call or the device against itself (torch fp32 operations in the
header's order on the device's own stored values); float64 enters in the teacher-forced calls at a general beta per row and in the sum
of a 50-call anneal sequence.

A teacher-forced call at beta is given a recorded point of the scalar chain and the record's grad_g / energy_g UNSCALED; its float64
answer is the metric call's at (beta grad_g, beta energy_g): `tempered_record` restates the record there (the kept state evaluated at
beta as well) and hmc_metric_gpu.gates builds the scalar modules' gates around it, with beta inside the magnitudes they are made of."""
import copy
import types

import torch

from oracle import flow_oracle as O
import ais_restated as A
import chain_geometries as G
import hmc_metric_gpu as MG
import hmc_rows_gpu as HG
import hmc_tempered_restated as TR
import rmala_restated as RM

bits, fig, FIELDS, METRIC = HG.bits, HG.fig, HG.FIELDS, MG.METRIC
TEMPER = ("beta", "like_grad", "like_energy", "log_w")
IDENTITY = HG.IDENTITY                       # every instantiation of a tempered kernel, by the dispatch rule
POWER_OF_TWO = HG.ARITHMETIC
GENERAL = G.CASES + G.LARGE
FORMS = G.FORMS
ANNEAL = MG.WINDOW


def new_temper(lsnf, s, B, beta=1.0, kept="old", seed=0):
    """An HmcRowTemper of B rows on the case's device.  kept "old": like_grad / like_energy hold recognisable values (a kept state's,
    which a rejected row must keep to the bit); "nan": NaN, for calls that must not read them.  log_w holds NaN (a call that does not
    anneal must not touch it, and NaN compares as bits)."""
    t = lsnf.flow.new_hmc_row_temper(s.plan, B, s.dev, beta)
    if kept == "old":
        g = torch.Generator().manual_seed(6000 + seed)
        t.like_grad.copy_(torch.randn(B, s.c.nz, generator=g)); t.like_energy.copy_(3.0 * torch.rand(B, generator=g))
    else:
        t.like_grad.fill_(float("nan")); t.like_energy.fill_(float("nan"))
    t.log_w.fill_(float("nan"))
    return t


def weights_at(temper, seed=0):
    """Put a running Kahan pair into temper.log_w: a sum of order 10 and a compensation of the size it has there."""
    B = temper.log_w.shape[0]
    g = torch.Generator().manual_seed(6100 + seed)
    temper.log_w[:, 0] = (10.0 * torch.randn(B, generator=g)).to(temper.log_w.device)
    temper.log_w[:, 1] = (1e-6 * torch.randn(B, generator=g)).to(temper.log_w.device)
    return temper


def clone_temper(lsnf, t):
    return lsnf.flow.HmcRowTemper(*(getattr(t, f).clone() for f in TEMPER))


def beta_rows(B, seed=0, lo=0.0, hi=1.0):
    """U(lo, hi) per row as the fp32 numbers the kernels see; row 0 at 0.0 and row 1 above 1 (1.5)."""
    g = torch.Generator().manual_seed(6200 + seed)
    b = (lo + (hi - lo) * torch.rand(B, generator=g)).float()
    if B >= 2 and lo == 0.0:
        b[0], b[1] = 0.0, 1.5
    return b


def run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, rows=slice(None), state=None, adapt=None, window=None, propose=True,
        inplace=False, point=None, ge="record", e="record", anneal=None):
    """The recorded call r on its rows from its inputs' casts through the tempered wrapper: (state after, [next point, accepted,
    log_alpha])."""
    F, dev = lsnf.flow, s.dev
    cut = lambda t: None if t is None else t[rows].float().to(dev).contiguous()
    state = sp.T.state_for(lsnf, s, r, rows) if state is None else state
    kw = dict(phase=r.phase, uniform=uniform, propose=propose, adapt=adapt, window=window, inplace=inplace, anneal=anneal)
    point = cut(sp.point(r)) if point is None else point
    ge = cut(r.ge) if isinstance(ge, str) else ge
    e = cut(r.e) if isinstance(e, str) else e
    if sp.name == "z":
        out = F.hmc_step_tempered(s.plan, point, ge, e, state, noise, steps, metric, temper, **kw)[:3]
    else:
        saved, act = sp.T.stash_at(lsnf, s.plan, point)
        out = F.reverse_hmc_step_tempered(s.plan, point, saved, act, ge, e, state, noise, steps, metric, temper, **kw)
    return state, list(out)


def like_of(lsnf, sp, s, r, rows=slice(None), ge="record", e="record"):
    """(gl, el) of the recorded point as the device forms them: z: grad_g and energy_g themselves (None: zeros); eps: the
    reverse-backward's own J^T grad_g (`reverse_backward_z`'s bits) and energy_g."""
    F, dev = lsnf.flow, s.dev
    cut = lambda t: None if t is None else t[rows].float().to(dev).contiguous()
    point = cut(sp.point(r))
    ge = cut(r.ge) if isinstance(ge, str) else ge
    e = cut(r.e) if isinstance(e, str) else e
    B = point.shape[0]
    el = torch.zeros(B, device=dev) if e is None else e
    if ge is None:
        return torch.zeros_like(point), el
    if sp.name == "z":
        return ge, el
    saved, act = sp.T.stash_at(lsnf, s.plan, point)
    return F.reverse_backward_z(s.plan, point, saved, act, ge), el


def flat(res, steps, metric, temper):
    return MG.flat(res, steps, metric) + [getattr(temper, f) for f in TEMPER]


# ---- 1 ----
def check_unit_temperature_is_the_metric_call(lsnf, sp, s):
    c, dev, B = s.c, s.dev, s.c.B
    for r, propose in MG.forms_of(sp, c):
        end = r.phase == "end"
        kept = sp.T.state_for(lsnf, s, r).z if end else None
        gl, el = like_of(lsnf, sp, s, r)
        for how in ("tensors", "philox"):
            for adapt, window in [(None, None)] + ([("update", None), ("update", "close"), (None, "fold")] if end else []):
                noise, uniform = HG.draws(lsnf, sp, c, r, how, dev, propose)
                new_m = lambda: MG.window_at(lsnf, sp, s, kept) if window else MG.new_metric(lsnf, s, B)
                ref_steps, ref_m = MG.same_steps(lsnf, sp, c, B, dev, 7), new_m()
                ref = MG.flat(MG.run(lsnf, sp, s, r, ref_steps, ref_m, noise, uniform, propose=propose, adapt=adapt, window=window), ref_steps, ref_m)
                steps, metric, temper = MG.same_steps(lsnf, sp, c, B, dev, 7), new_m(), new_temper(lsnf, s, B, 1.0, "old" if end else "nan")
                before = clone_temper(lsnf, temper)
                state, out = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, propose=propose, adapt=adapt, window=window)
                got = MG.flat((state, out), steps, metric)
                name = f"{sp.name} {c.geo} B{B} {r.phase} propose={propose} {how} adapt={adapt} window={window}"
                assert len(got) == len(ref)
                for k, (a, b) in enumerate(zip(got, ref)):
                    assert bits(a, b), f"{name}: output {k} differs"
                # beta and log_w are written by annealing calls alone; the likelihood's parts wherever the accepted point is written
                assert bits(temper.beta, before.beta) and bits(temper.log_w, before.log_w)
                if r.phase == "inner":
                    assert bits(temper.like_grad, before.like_grad) and bits(temper.like_energy, before.like_energy)
                    continue
                acc = out[1] == 1.0
                assert bits(temper.like_grad, torch.where(acc[:, None], gl, before.like_grad)), f"{name}: like_grad"
                assert bits(temper.like_energy, torch.where(acc, el, before.like_energy)), f"{name}: like_energy"


# ---- 2 ----
def check_power_of_two_temperature_is_the_scaled_likelihood(lsnf, sp, s):
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    k = torch.tensor([(-2.0, 0.0, 3.0)[b % 3] for b in range(B)])
    bt = torch.exp2(k).to(dev)
    for r, propose in MG.forms_of(sp, c):
        ge, e = r.ge.float().to(dev).contiguous(), r.e.float().to(dev).contiguous()
        for how in ("tensors", "philox"):
            noise, uniform = HG.draws(lsnf, sp, c, r, how, dev, propose)
            fresh = lambda: (F.new_hmc_row_steps(B, dev, c.s), MG.new_metric(lsnf, s, B))
            steps, metric = fresh()
            ref = HG.flat(MG.run(lsnf, sp, s, r, steps, metric, noise, uniform, propose=propose, ge=bt[:, None] * ge, e=bt * e))      # (exact scalings)
            steps, metric = fresh()
            temper = new_temper(lsnf, s, B, bt, "old" if r.phase == "end" else "nan")
            got = HG.flat(run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, propose=propose))
            assert len(got) == len(ref)
            for j, (a, b) in enumerate(zip(got, ref)):
                assert bits(a, b), f"{sp.name} {c.geo} B{B} {r.phase} propose={propose} {how}: output {j} differs"
            if B >= 3 and propose:                           # (and the temperature is not ignored: at 2^3 the next point is another)
                steps, metric = fresh()
                plain = HG.flat(MG.run(lsnf, sp, s, r, steps, metric, noise, uniform, propose=propose))
                assert bits(got[5][1::3], plain[5][1::3]) and not bits(got[5][2::3], plain[5][2::3])


# ---- 3 ----
def tempered_record(sp, c, r, beta):
    """The record r restated at the rows' beta (B, fp32 values), on the CPU: g / U_prop at the point, the kept state (g_acc, u_acc)
    evaluated at beta from its own parts, and the fp32 restatement's g / U_prop from the fp32 casts the device is given; gl64 / el64:
    the likelihood's parts at the point in float64."""
    f32, f64 = torch.float32, torch.float64
    b = beta.double()
    r2 = copy.copy(r)
    point = sp.point(r)
    r2.el64 = r.e
    r2.gl64 = r.ge if sp.name == "z" else r.g - point
    r2.g = r.g + (b - 1.0)[:, None] * r2.gl64
    r2.U_prop = r.U_prop + (b - 1.0) * r.e
    if r.phase == "end":
        P = TR.parts(sp.name, c.p, MG.acc_point(sp, r), c.quad)
        r2.u_acc, r2.g_acc = TR.tempered(P, b)
    o = types.SimpleNamespace()
    b32 = beta.to(f32)
    if sp.name == "z":
        q, zp = O.to_dtype(c.p, f32), point.to(f32)
        o.g = (b32[:, None] * r.ge.to(f32)) + O.grad_neg_sum_ll_wrt_z(q, zp)
        o.U_prop = (b32 * r.e.to(f32)) - O.flow_log_prob(q, zp)[2].detach()
    else:
        ep = point.to(f32)
        o.g = ep + (b32[:, None] * RM.pull_back(c.p, ep, r.ge.to(f32), f32))
        o.U_prop = (b32 * r.e.to(f32)) + 0.5 * (ep * ep).sum(1)
    r2.o32 = o
    return r2


def general_gates(sp, c, r, beta):
    """(the tempered record, hmc_metric_gpu.gates' answer for it at a unit scale)."""
    r2 = tempered_record(sp, c, r, beta)
    return r2, MG.gates(sp, sp.T, r2, torch.ones(c.B, c.nz), c.s)


def cpu_set_aside(sp, c):
    """The rows every end call of the case sets aside at the test's beta, from float64 and the fp32 restatement alone."""
    beta = beta_rows(c.B)
    return [int((~general_gates(sp, c, r, beta)[1].decided).sum()) for r in c.device_calls if r.phase == "end"]


def check_general_temperature_follows_float64(lsnf, sp, s):
    c, dev, B, F, T = s.c, s.dev, s.c.B, lsnf.flow, sp.T
    beta = beta_rows(B)
    tag = f"[{sp.name} tempered] {c.geo} B{B} beta U(0, 1) with 0 and 1.5"
    cut = lambda t: t.float().to(dev).contiguous()
    for j, r in enumerate(c.device_calls):
        r2, o = general_gates(sp, c, r, beta)
        propose = r.noise is not None or r.phase == "inner"
        noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, propose)
        steps, metric = F.new_hmc_row_steps(B, dev, c.s), MG.new_metric(lsnf, s, B)
        temper = new_temper(lsnf, s, B, beta, "old" if r.phase == "end" else "nan")
        kept = clone_temper(lsnf, temper)
        state = T.state_for(lsnf, s, r2)                     # (the kept state at beta)
        before = T.clone_state(lsnf, state)
        gl, el = like_of(lsnf, sp, s, r)
        state, (nxt, acc, la) = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, state=state, propose=propose)
        torch.cuda.synchronize()
        xa, ga, ua, mom, kin = (getattr(state, f).cpu() for f in FIELDS)
        name = f"{tag} call {j} {r.phase}"
        d = o.decided
        assert bits(temper.beta, kept.beta) and bits(temper.log_w, kept.log_w)
        if r.phase == "inner":
            assert acc is None and la is None
            for f in ("z", "grad", "energy", "kin"):
                assert bits(getattr(state, f), getattr(before, f))
            assert bits(temper.like_grad, kept.like_grad) and bits(temper.like_energy, kept.like_energy)
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
            # the accepted state against float64: U within 1e-5 of the magnitudes it is made of, grad U rel-L2 1e-5, each widened to
            # 3 x the fp32 restatement's own error where that exceeds a third of it
            prior = (r2.U_prop - beta.double() * r.e).abs()
            ub, uw = T.widened(1e-5 * (beta.double() * r.e.abs() + prior), (r2.o32.U_prop.double() - r2.U_prop).abs())
            gb, gw = T.widened(torch.full((B,), 1e-5, dtype=torch.float64), T.rel_rows(r2.o32.g, r2.g))
            eu, eg = (ua.double() - r2.U_prop).abs(), T.rel_rows(ga, r2.g)
            print(f"{name}: worst u_acc error / bound = {fig((eu / ub)[yes]):.3f} ({uw} rows widened by the fp32 restatement), worst grad_acc rel-L2 / "
                  f"bound = {fig((eg / gb)[yes]):.3f} ({gw} widened)")
            assert bool((eu <= ub)[yes].all()) and bool((eg <= gb)[yes].all())
            if r.phase == "end":
                bz, bg, bu = before.z.cpu(), before.grad.cpu(), before.energy.cpu()
                assert bits(xa[no], bz[no]) and bits(ga[no], bg[no]) and bits(ua[no], bu[no])
            # the likelihood's parts: gl / el on the rows the device accepted, the old bits on the others
            a = acc == 1.0
            assert bits(temper.like_grad, torch.where(a[:, None], gl, kept.like_grad)) and bits(temper.like_energy, torch.where(a, el, kept.like_energy))
        if o.mom is not None:
            e = (mom.double() - o.mom).norm(dim=1)
            print(f"{name}: worst |mom - fp64| / bound = {fig((e / o.mom_bound)[d]):.3f} ({o.mom_wide} rows widened by the fp32 restatement)")
            assert bool((e <= o.mom_bound)[d].all())
        if o.nxt is not None:
            e = T.rel_rows(nxt.cpu(), o.nxt)
            print(f"{name}: worst next-point rel-L2 / bound = {fig((e / o.nxt_bound)[d]):.3f} ({o.nxt_wide} rows widened)")
            assert bool((e <= o.nxt_bound)[d].all())
        else:
            assert nxt is None
        if o.kin is not None:
            e = (kin.double() - o.kin).abs()
            print(f"{name}: worst kin0 error / bound = {fig(e / o.kin_bound):.3f} ({o.kin_wide} rows widened)")
            assert bool((e <= o.kin_bound).all())


# ---- 4 ----
def next_beta(beta, seed=0):
    """beta + U(0, 0.4) per row as fp32; row 2 unchanged (d = 0), row 3 cooled."""
    g = torch.Generator().manual_seed(6300 + seed)
    bn = (beta.cpu() + 0.4 * torch.rand(beta.shape[0], generator=g)).float()
    if bn.shape[0] >= 4:
        bn[2], bn[3] = beta[2].item(), 0.5 * beta[3].item()
    return bn.to(beta.device)


def kahan32(w, c, inc):
    """The header's Kahan lines as torch fp32 operations: (w', c')."""
    y = inc - c
    t = w + y
    return t, (t - w) - y


def check_anneal_lines(lsnf, sp, s):
    """From the device's own stored state after the same call WITHOUT the anneal, the header's fp32 lines hold to the bit."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    end = sp.end_calls(c)
    forms = [(c.calls[0], True, None, None)] + [(r, sp.proposes(r), None, None) for r in end] + [(end[0], True, "update", "close")]
    assert any(p for _, p, _, _ in forms[1:]) and any(not p for _, p, _, _ in forms[1:])
    beta = beta_rows(B, 1).to(dev)
    bn = next_beta(beta)
    for r, propose, adapt, window in forms:
        name = f"[{sp.name} tempered] {c.geo} B{B} anneal {r.phase} propose={propose} adapt={adapt} window={window}"
        noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, propose)
        kept = sp.T.state_for(lsnf, s, r).z if r.phase == "end" else None

        def call(anneal):
            steps = MG.same_steps(lsnf, sp, c, B, dev, 7)
            metric = MG.window_at(lsnf, sp, s, kept) if window else MG.new_metric(lsnf, s, B)
            temper = new_temper(lsnf, s, B, beta, "old" if r.phase == "end" else "nan")
            if anneal is not None:
                weights_at(temper)
            start = clone_temper(lsnf, temper)
            state, out = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, propose=propose, adapt=adapt, window=window, anneal=anneal)
            return state, out, steps, metric, temper, start
        sa, oa, steps_a, metric_a, ta, _ = call(None)
        sb, ob, steps_b, metric_b, tb, start = call(bn)
        acc = ob[1] == 1.0
        if r.phase == "end":
            assert 0 < int(acc.sum()) < B, f"{name}: the case needs accepted and rejected rows"
        # the decision, the accepted points, the likelihood's parts, the adaptation and the window are the plain call's
        assert bits(ob[1], oa[1]) and bits(ob[2], oa[2]) and bits(sb.z, sa.z) and bits(sb.kin, sa.kin)
        assert bits(tb.like_grad, ta.like_grad) and bits(tb.like_energy, ta.like_energy)
        assert bits(steps_b.step, steps_a.step) and bits(steps_b.adapt, steps_a.adapt) and MG.untouched(metric_b, metric_a)
        # the header's lines on the state after the decision (the plain call's stored arrays): EVERY row
        d = bn - beta
        assert bits(tb.beta, bn), f"{name}: beta"
        assert bits(sb.energy, sa.energy + (d * ta.like_energy)), f"{name}: u_acc is not u_s + (d el_s)"
        assert bits(sb.grad, sa.grad + (d[:, None] * ta.like_grad)), f"{name}: grad_acc is not g_s + (d gl_s)"
        w1, c1 = kahan32(start.log_w[:, 0], start.log_w[:, 1], -(d * ta.like_energy))
        assert bits(tb.log_w[:, 0], w1) and bits(tb.log_w[:, 1], c1), f"{name}: the Kahan pair"
        moved = d != 0
        assert bits(sb.grad[~moved], sa.grad[~moved]) and not bits(sb.grad[moved], sa.grad[moved])
        if not propose:                                      # nothing begun: the full-step momentum of the plain call
            assert ob[0] is None and bits(sb.mom, sa.mom)
            continue
        # the next trajectory begins from the RE-TEMPERED gradient: fp32, the header's operations in the header's order
        st, sdd = steps_b.step[:, None], metric_b.scale
        ph = noise - (0.5 * st) * (sdd * sb.grad)
        assert bits(sb.mom, ph), f"{name}: mom is not xi - (0.5 s) (sd grad_acc')"
        assert bits(ob[0], sb.z + st * (sdd * ph)), f"{name}: the next point is not z_state + s (sd mom)"
        assert bits(sb.mom[~moved], sa.mom[~moved]) and not bits(sb.mom[moved], sa.mom[moved])


def check_anneal_sum(lsnf, sp, s, calls=50):
    """A 50-call ANNEAL sequence teacher-forced at one record with increasing beta: log_weight() against the float64 sum of the
    increments the device's own stored values give, within 1e-6 of the sum of their magnitudes (what the compensated sum is for)."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = sp.end_calls(c)[0]
    noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, False)
    sched = A.schedule(calls)
    rows = (0.5 + torch.arange(B, dtype=torch.float64) / B)                       # every row its own schedule, 0 .. (0.5 .. 1.5)
    betas = (sched[:, None] * rows[None, :]).float().to(dev)
    steps, metric = F.new_hmc_row_steps(B, dev, c.s), MG.new_metric(lsnf, s, B)
    temper = new_temper(lsnf, s, B, betas[0], "old")
    old = clone_temper(lsnf, temper)
    temper.log_w.zero_()
    total, mag, plain = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, device=dev)
    accepted = 0
    for t in range(calls):
        temper.like_grad.copy_(old.like_grad); temper.like_energy.copy_(old.like_energy)       # (teacher-forced: the same kept state)
        state, out = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, propose=False, anneal=betas[t + 1])
        assert bits(temper.beta, betas[t + 1])
        inc = -(betas[t + 1].double() - betas[t].double()) * temper.like_energy.double()      # el_s of every row, as the device stored it
        total, mag, plain = total + inc, mag + inc.abs(), plain + inc.float()
        accepted += int(out[1].sum().item())
    err = (temper.log_weight() - total).abs()
    gate = 1e-6 * mag
    print(f"[{sp.name} tempered] {c.geo} B{B}: {calls} annealing calls, {accepted} acceptances of {calls * B}: worst |log_weight - float64 sum| / "
          f"(1e-6 sum |inc|) = {fig(err / gate):.3f}; a plain fp32 sum: {fig((plain.double() - total).abs() / gate):.3f}; sums of "
          f"{total.abs().min().item():.3g} .. {total.abs().max().item():.3g}")
    assert 0 < accepted < calls * B and bool((mag > 0).all())
    assert bool((err <= gate).all())


# ---- 5 ----
def check_rows_do_not_depend_on_the_batch(lsnf, sp, s):
    """The first 33 rows of the case's batch against 33 rows alone (another workgroup shape), and against two shards with their row0,
    on an end call that adapts, closes and anneals: the five new arrays among the compared outputs."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = next(x for x in c.calls if x.phase == "end")
    kept = sp.T.state_for(lsnf, s, r).z
    sd = MG.column_scale(B, c.nz, 3)
    beta = beta_rows(B, 2).to(dev)
    bn = next_beta(beta, 2)

    def go(rows, row0, mode, window, anneal):
        whole, wm, wt = MG.same_steps(lsnf, sp, c, B, dev, 7), MG.window_at(lsnf, sp, s, kept, sd), weights_at(new_temper(lsnf, s, B, beta, "old"))
        steps = F.HmcRowSteps(whole.step[rows].clone(), whole.adapt[rows].clone())
        metric = F.HmcRowMetric(*(getattr(wm, f)[rows].clone() for f in METRIC))
        temper = F.HmcRowTemper(*(getattr(wt, f)[rows].clone() for f in TEMPER))
        res = run(lsnf, sp, s, r, steps, metric, temper, F.PhiloxNoise(99, 7, row0), None, rows=rows, propose=True, adapt=mode, window=window,
                  anneal=bn[rows].clone() if anneal else None)
        return flat(res, steps, metric, temper)
    for mode, window, anneal in (("update", "close", True), (None, None, True), ("last", "fold", False)):
        whole, part = go(slice(0, B), 0, mode, window, anneal), go(slice(0, 33), 0, mode, window, anneal)
        lo, hi = go(slice(0, 20), 0, mode, window, anneal), go(slice(20, 33), 20, mode, window, anneal)
        for a, b, x, y in zip(whole, part, lo, hi):
            assert bits(a[:33], b) and bits(b, torch.cat([x, y]))
        wrong = go(slice(20, 33), 0, mode, window, anneal)
        assert not bits(wrong[5], hi[5])                     # (the draws are a function of the global row)


# ---- 6 ----
def check_a_nan_row(lsnf, sp, s):
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = sp.end_calls(c)[0]
    bad, keep = 18, torch.arange(B, device=dev) != 18
    sd = MG.column_scale(B, c.nz, 4).clamp(0.5, 2.0)
    rng = F.PhiloxNoise(3, 4, 0)
    beta = beta_rows(B, 3).to(dev)
    bn = next_beta(beta, 3)
    fresh = lambda: (MG.same_steps(lsnf, sp, c, B, dev, 7), MG.new_metric(lsnf, s, B, sd, sentinel=False), weights_at(new_temper(lsnf, s, B, beta, "old")))
    steps, metric, temper = fresh()
    clean = flat(run(lsnf, sp, s, r, steps, metric, temper, rng, None, propose=True, adapt="update", window="fold", anneal=bn), steps, metric, temper)
    steps, metric, temper = fresh()
    start = clone_temper(lsnf, temper)
    state = sp.T.state_for(lsnf, s, r)
    state.mom[bad] = float("nan")
    before = sp.T.clone_state(lsnf, state)
    state, out = run(lsnf, sp, s, r, steps, metric, temper, rng, None, state=state, propose=True, adapt="update", window="fold", anneal=bn)
    got = flat((state, out), steps, metric, temper)
    assert out[1][bad].item() == 0.0 and bool(torch.isnan(out[2][bad]))
    # the row rejects and anneals from its KEPT state: the header's lines on the arrays it was given
    d = bn - beta
    assert bits(state.z[bad], before.z[bad]) and bits(temper.like_grad[bad], start.like_grad[bad]) and bits(temper.like_energy[bad], start.like_energy[bad])
    assert bits(state.grad[bad], (before.grad + d[:, None] * start.like_grad)[bad]) and bits(state.energy[bad], (before.energy + d * start.like_energy)[bad])
    w1, c1 = kahan32(start.log_w[:, 0], start.log_w[:, 1], -(d * start.like_energy))
    assert bits(temper.log_w[bad, 0], w1[bad]) and bits(temper.log_w[bad, 1], c1[bad]) and bits(temper.beta, bn)
    assert bool(torch.isfinite(out[0][bad]).all()) and bool(torch.isfinite(state.mom[bad]).all()) and bool(torch.isfinite(temper.log_w[bad]).all())
    for a, b in zip(got, clean):
        assert bits(a[keep], b[keep])                        # every other row: the bits of the run without the NaN


# ---- 7 ----
def check_forms(lsnf, sp, s):
    """In place, every tensor 4 bytes off a 16-byte boundary (log_w 8 bytes off: it stays 8-byte aligned; the stash and the quads stay
    16-byte aligned) and NULL optionals, at a general beta with an end call that adapts, closes and anneals."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    sd = MG.column_scale(B, c.nz, 1)
    beta = beta_rows(B, 4).to(dev)
    bn = next_beta(beta, 4)

    def off(t, floats=1):
        if t is None:
            return None
        t = t.float().to(dev)
        b = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
        v = b[floats: floats + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 * floats
        return v

    def window_state(m):
        g = torch.Generator().manual_seed(9)
        m.mean.copy_(torch.randn(B, c.nz, generator=g)); m.m2.copy_(3.0 * torch.rand(B, c.nz, generator=g)); m.count.fill_(3.0)
        return m
    for r, _ in MG.forms_of(sp, c)[:3]:
        end = r.phase == "end"
        kw = dict(adapt="update", window="close", anneal=bn) if end else dict(anneal=bn) if r.phase == "init" else {}
        noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, True)
        fresh = lambda: (MG.same_steps(lsnf, sp, c, B, dev, 5), window_state(MG.new_metric(lsnf, s, B, sd)),
                         weights_at(new_temper(lsnf, s, B, beta, "old" if end else "nan")))
        steps, metric, temper = fresh()
        ref = flat(run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, **kw), steps, metric, temper)
        # in place: the next point over the point
        steps, metric, temper = fresh()
        point = sp.point(r).float().to(dev)
        res = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, point=point, inplace=True, **kw)
        assert res[1][0].data_ptr() == point.data_ptr()
        assert all(bits(a, b) for a, b in zip(flat(res, steps, metric, temper), ref))
        # every tensor off its 16-byte boundary
        steps, metric, temper = fresh()
        steps = F.HmcRowSteps(off(steps.step), steps.adapt)
        metric = F.HmcRowMetric(off(metric.scale), off(metric.mean), off(metric.m2), off(metric.count))
        temper = F.HmcRowTemper(off(temper.beta), off(temper.like_grad), off(temper.like_energy), off(temper.log_w, 2))
        assert temper.log_w.data_ptr() % 16 == 8
        st = sp.T.state_for(lsnf, s, r)
        state = F.HmcState(*(off(getattr(st, f)) for f in FIELDS))
        kw4 = dict(kw, anneal=off(bn)) if "anneal" in kw else kw
        res = run(lsnf, sp, s, r, steps, metric, temper, off(noise), off(uniform), state=state, point=off(sp.point(r)), ge=off(r.ge), e=off(r.e),
                  inplace=True, **kw4)
        assert all(bits(a, b) for a, b in zip(flat(res, steps, metric, temper), ref))
        # NULL gradient and energy are zeros
        rng = None if r.phase == "inner" else F.PhiloxNoise(8, 9, 0)
        both = []
        for gg, e in ((None, None), (torch.zeros(B, c.nz, device=dev), torch.zeros(B, device=dev))):
            steps, metric, temper = fresh()
            both.append(flat(run(lsnf, sp, s, r, steps, metric, temper, rng, None, ge=gg, e=e, **kw), steps, metric, temper))
        assert all(bits(a, b) for a, b in zip(*both))
    steps, metric, temper = fresh()                          # the likelihood's kept gradient is an output: it may not be the point
    for bad in (F.HmcRowTemper(temper.beta, point, temper.like_energy, temper.log_w), F.HmcRowTemper(temper.beta, temper.like_grad, temper.like_energy, off(temper.log_w))):
        try:
            run(lsnf, sp, s, r, steps, metric, bad, noise, uniform, point=point, anneal=bn)
        except lsnf.LsnfError:
            pass
        else:
            raise AssertionError("like_grad_acc over the point, or a log_w 4 bytes off, was not refused")


# ---- 9: both samplers on the CPU experiment's problem ----
class DiagonalG(torch.nn.Module):
    """netG(z) = A z with A = diag(a): with x = A t and sigma = 1 the samplers' energy is ais_restated's 1/2 |A (z - t)|^2."""

    def __init__(self, quad):
        super().__init__()
        self.a = torch.nn.Parameter(quad.a.float(), requires_grad=False)

    def forward(self, z):
        return z.flatten(1) * self.a


def ais_problem(lsnf, K, dev):
    """(net, netG, x (N, nz), the closed forms (N), the energy of rows (B, nz) -> (B) in float64) of ais_restated's experiment."""
    p = A.affine_flow()
    quads = [A.datum(sd) for sd in A.EXP_DATA]
    net = K.module_of(lsnf, p, dev, False)
    netG = DiagonalG(quads[0]).to(dev)
    x = torch.stack([q.t * q.a for q in quads]).float().to(dev)
    exact = torch.tensor([A.closed_form(p, q) for q in quads], dtype=torch.float64)
    stacked = A.Stacked(quads, A.EXP_CHAINS)
    return net, netG, x, exact, lambda z: stacked(z.detach().cpu().double().reshape(-1, A.GEO[0]))[0]


def check_samplers(lsnf, sp, K, dev):
    import math
    F, Lv = lsnf.flow, lsnf.langevin
    net, netG, x, exact, energy = ais_problem(lsnf, K, dev)
    fn = Lv.estimate_log_px_ais_z_with_flow if sp.name == "z" else Lv.estimate_log_px_ais_eps_with_flow
    N, C, D = x.shape[0], A.EXP_CHAINS, x[0].numel()
    kw = dict(chains=C, leapfrog_steps=A.EXP_L, g_l_step_size=A.EXP_STEP, g_llhd_sigma=1.0)
    ph = F.PhiloxNoise(5, 10, 0)
    log_px, log_w, ess, rate, z_T, temper = fn(x, netG, net, betas=Lv.ais_schedule(A.EXP_T), philox=ph, **kw)
    torch.cuda.synchronize()
    band = A.BAND[sp.name]
    err = log_px.cpu() + 0.5 * D * math.log(2.0 * math.pi) - exact
    acc = rate.double().mean().item()
    print(f"[{sp.name} tempered] AIS sampler, T={A.EXP_T}, L={A.EXP_L}, {C} chains, step {A.EXP_STEP}: errors log Z_hat - closed form "
          + " ".join(f"{e:+.4f}" for e in err.tolist()) + f" (band {band['error']}), ess " + " ".join(f"{e:.2f}" for e in ess.tolist())
          + f" (band {band['ess']}), mean acceptance {acc:.4f} (band {band['accept']})")
    assert log_px.dtype == torch.float64 and log_px.shape == (N,) and log_w.shape == (N, C) and rate.shape == (N * C,) and z_T.shape == (N * C, D, 1, 1)
    assert bool(((err >= band["error"][0]) & (err <= band["error"][1])).all())
    assert bool(((ess.cpu() >= band["ess"][0]) & (ess.cpu() <= band["ess"][1])).all())
    assert band["accept"][0] <= acc <= band["accept"][1]
    assert bool((temper.beta == 1.0).all()) and ph.offset == 10 + A.EXP_T + 1
    assert bits(log_w.cpu(), temper.log_weight().view(N, C).cpu())
    # betas = [0, 1] is plain importance sampling: log_w = -E(z_0) of the sample's own draws, to fp32
    ph = F.PhiloxNoise(5, 10, 0)
    z0, eps0 = net.sample(N * C, ph.step(0), return_eps=True)
    _, lw1, _, _, _, t1 = fn(x, netG, net, betas=[0.0, 1.0], philox=ph, **kw)
    e0 = energy(z0)
    assert bool(((lw1.cpu().reshape(-1) + e0).abs() <= 1e-5 * (1.0 + e0)).all()) and ph.offset == 12
    # the hand-written loop of netF.*_tempered calls reproduces the sampler, bit for bit
    T, L = 3, 2
    betas = Lv.ais_schedule(T)
    got = fn(x, netG, net, betas=betas, philox=F.PhiloxNoise(7, 3, 0), **dict(kw, leapfrog_steps=L))
    ph, B, nz, plan = F.PhiloxNoise(7, 3, 0), N * C, D, net._plan()
    xs = x.repeat_interleave(C, dim=0)
    z0, eps0 = net.sample(B, ph.step(0), return_eps=True)
    point = (z0 if sp.name == "z" else eps0).detach().reshape(B, nz).contiguous().clone()
    steps, metric, temper = F.new_hmc_row_steps(B, dev, A.EXP_STEP), F.new_hmc_row_metric(plan, B, dev), F.new_hmc_row_temper(plan, B, dev, 0.0)
    state, act = F.new_hmc_state(plan, B, dev), F.new_act_saved(plan, B, dev)
    rows = lambda t: torch.full((B,), float(betas[t]), dtype=torch.float32, device=dev)
    for j in range(T * L + 1):
        t, inner = j // L, j % L != 0
        phase = "inner" if inner else "end" if j else "init"
        anneal = rows(t + 1) if not inner and t < T else None
        noise = None if inner else ph.step(t + 1)
        if sp.name == "z":
            z, saved = point, None
        elif F.reverse_keep_supported(plan, B):
            z, _, saved = F.reverse(plan, point, None, save_for_backward=True, act_saved=act)
        else:
            z = F.reverse(plan, point, None)[0]
            saved = F.forward(plan, z, None, want_ll=False, save_for_backward=True, act_saved=act)[3]
        zr = z.view(B, nz, 1, 1).detach().requires_grad_(True)
        e = 0.5 * ((netG(zr) - xs) ** 2).flatten(1).sum(1)
        gg = torch.autograd.grad(e.sum(), zr)[0].reshape(B, nz).contiguous()
        with torch.no_grad():
            if sp.name == "z":
                net.hmc_step_tempered(point, gg, e.detach(), state, noise, steps, metric, temper, phase=phase, propose=j < T * L, inplace=True,
                                      anneal=anneal)
            else:
                net.reverse_hmc_step_tempered(point, saved, act, gg, e.detach(), state, noise, steps, metric, temper, phase=phase,
                                              propose=j < T * L, inplace=True, anneal=anneal)
    z_T = state.z if sp.name == "z" else F.reverse(plan, state.z, None)[0]
    assert bits(got[1], temper.log_weight().view(N, C)) and bits(got[4].reshape(B, nz), z_T)
    for f in TEMPER:
        assert bits(getattr(got[5], f), getattr(temper, f)), f

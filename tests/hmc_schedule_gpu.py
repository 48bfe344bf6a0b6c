"""TEST INFRASTRUCTURE (GPU): what tests/test_gpu_hmc_schedule.py (`lsnf_hmc_step_schedule`, the chain on z) and
tests/test_gpu_rhmc_schedule.py (`lsnf_reverse_hmc_step_schedule`, the chain on eps) check, written once for both on
tests/hmc_rows_gpu.py's `Space`, in the style of tests/hmc_resample_gpu.py, whose cases, `run` and helpers are reused by import.

Bit identities are against the resampling call or the device against itself: the scheduling call's every output is the resampling
call's from the same inputs with beta_next = the beta' the scheduling call left in beta_rows.  float64 enters where beta' itself is
held to the root of cess64(delta) = cess_frac under the bound of tests/hmc_schedule_restated.py.

How a launch gets its three kinds of group (`design`).  Everything the search reads is an input of the call: beta_rows, beta_next,
the Kahan pairs, and el_s: energy_g on a row that accepts (every row of an INIT call) and the kept like_energy on one that does not,
so the designed energies are given as both and el_s is known whatever the trajectory decides.  Group k of a launch is, by k % 3: SEARCH (b in U(0, 0.3), ceiling 1, energies 5 + s t with s
in U(8, 12) and t in [0, 1] reaching both ends, log weights within a few tenths of each other), WHOLE (ceiling b + 2^-8, energies 5 + 3 t: cess(D) is 1 to within 1e-3), IDLE (ceiling
= b, or below it on every other such group).  D is the fp32 difference the kernel forms.  Before the launch the float64 cess at D is
asserted to be clear of cess_frac by eps_c on the right side for every SEARCH and WHOLE group, and the SEARCH groups' cess to fall
monotonically.  Nothing is chosen from a device's answer."""
import math

import torch

import hmc_metric_gpu as MG
import hmc_resample_gpu as SG
import hmc_rows_gpu as HG
import hmc_schedule_restated as S
import hmc_tempered_gpu as TG

bits, FIELDS, TEMPER = HG.bits, HG.FIELDS, TG.TEMPER
C3, TINY = HG.C3, HG.TINY
IDENTITY = HG.IDENTITY                       # every instantiation of a scheduling kernel, by the dispatch rule
MOVE, FORMS = SG.MOVE, SG.FORMS              # tests/hmc_exchange_gpu.py's SWAP (geometry, B, P) and call-form cases
EDGE = [C3 + (64, 8), TINY + (32, 4), TINY + (32, 2), C3 + (16400, 16)]       # at least five groups each
FRAC = 0.9
SEARCH, WHOLE, IDLE = 0, 1, 2


def run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, rows=slice(None), state=None, propose=True, anneal=None, resample=None,
        ess_threshold=0.5, resample_uniform=None, schedule=None, cess_target=FRAC, min_step=0.0, e="record", ge="record", point=None,
        inplace=False, reuse_buffers=False, adapt=None, window=None):
    """The recorded call r on its rows through the scheduling wrapper: (state after, [next point, accepted, log_alpha, ancestor, ess])."""
    F, dev = lsnf.flow, s.dev
    cut = lambda t: None if t is None else t[rows].float().to(dev).contiguous()
    state = sp.T.state_for(lsnf, s, r, rows) if state is None else state
    kw = dict(phase=r.phase, uniform=uniform, propose=propose, adapt=adapt, window=window, anneal=anneal, resample=resample,
              ess_threshold=ess_threshold, resample_uniform=resample_uniform, inplace=inplace, reuse_buffers=reuse_buffers,
              schedule=schedule, cess_target=cess_target, min_step=min_step)
    point = cut(sp.point(r)) if point is None else point
    e = cut(r.e) if isinstance(e, str) else e
    ge = cut(r.ge) if isinstance(ge, str) else ge
    if sp.name == "z":
        out = F.hmc_step_schedule(s.plan, point, ge, e, state, noise, steps, metric, temper, **kw)
        out = out[:3] + out[4:]
    else:
        saved, act = sp.T.stash_at(lsnf, s.plan, point)
        out = F.reverse_hmc_step_schedule(s.plan, point, saved, act, ge, e, state, noise, steps, metric, temper, **kw)
    return state, list(out)


def everything(res, steps, metric, temper):
    state, out = res
    return TG.flat((state, out[:3]), steps, metric, temper) + [t for t in out[3:] if t is not None]


# ---- 1 ----
def check_no_schedule_is_the_resample_call(lsnf, sp, s):
    """Without the flag every phase and form has the resampling call's bits (which are the tempered call's: tests/hmc_resample_gpu.py)."""
    c, dev, B = s.c, s.dev, s.c.B
    beta = TG.beta_rows(B).to(dev)
    bn = TG.next_beta(beta)
    for r, propose in MG.forms_of(sp, c):
        end = r.phase == "end"
        kept = sp.T.state_for(lsnf, s, r).z if end else None
        variants = [(None, None, None)]
        variants += [("update", "close", bn), (None, "fold", None), (None, None, bn)] if end else [(None, None, bn)] if r.phase == "init" else []
        for how in ("tensors", "philox"):
            for adapt, window, anneal in variants:
                noise, uniform = HG.draws(lsnf, sp, c, r, how, dev, propose)

                def fresh():
                    steps = MG.same_steps(lsnf, sp, c, B, dev, 7)
                    metric = MG.window_at(lsnf, sp, s, kept) if window else MG.new_metric(lsnf, s, B)
                    temper = TG.new_temper(lsnf, s, B, beta, "old" if end else "nan")
                    return steps, metric, TG.weights_at(temper) if anneal is not None else temper
                steps, metric, temper = fresh()
                ref = everything(SG.run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, propose=propose, adapt=adapt, window=window,
                                        anneal=anneal), steps, metric, temper)
                steps, metric, temper = fresh()
                # (the search's scalars are not looked at without the flag)
                got = everything(run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, propose=propose, adapt=adapt, window=window,
                                     anneal=anneal, cess_target=0.5, min_step=0.25), steps, metric, temper)
                name = f"{sp.name} {c.geo} B{B} {r.phase} propose={propose} {how} adapt={adapt} window={window} anneal={anneal is not None}"
                assert len(got) == len(ref)
                for k, (a, b) in enumerate(zip(got, ref)):
                    assert bits(a, b), f"{name}: output {k} differs"


# ---- the design of a launch ----
def design(B, P, seed):
    """(beta, cap, pair (B, 2), energy (B)) fp32 on the CPU and kind (G) of a launch (module docstring)."""
    g = torch.Generator().manual_seed(8300 + seed)
    G = B // P
    kind = torch.arange(G) % 3
    u = lambda *shape: torch.rand(*shape, generator=g)
    b = torch.where(kind == SEARCH, 0.3 * u(G), 0.2 + 0.6 * u(G)).float()
    past = (torch.arange(G) % 6 == 5)
    cap = torch.where(kind == SEARCH, torch.ones(G), torch.where(kind == WHOLE, b + 2.0 ** -8, torch.where(past, b - 0.125, b))).float()
    t = u(G, P)
    t[:, 0], t[:, 1] = 0.0, 1.0
    t = torch.gather(t, 1, u(G, P).argsort(dim=1))            # (the ends at random rungs)
    spread = torch.where(kind == SEARCH, 8.0 + 4.0 * u(G), torch.full((G,), 3.0))
    energy = (5.0 + spread[:, None] * t).float()
    l = ((-10.0 + 20.0 * u(G))[:, None] + 0.25 * torch.randn(G, P, generator=g)).float()
    comp = (1e-6 * torch.randn(G, P, generator=g)).float()
    pair = torch.stack([(l + comp).reshape(-1), comp.reshape(-1)], dim=1).float()
    rows = lambda v: v[:, None].expand(G, P).reshape(-1).contiguous()
    return rows(b), rows(cap), pair, energy.reshape(-1), kind


def expected(beta, cap, pair, energy, kind, P, frac):
    """The float64 side of a designed launch, from the call's stored fp32 inputs: D (G) as the kernel forms it, the SEARCH groups'
    root and slack, after asserting every group's kind is clear in float64."""
    G = beta.shape[0] // P
    b0, c0 = beta.view(G, P)[:, 0], cap.view(G, P)[:, 0]
    D = (c0 - b0).double()                                   # (the fp32 difference, exactly)
    l = pair[:, 0].double() - pair[:, 1].double()
    assert float(l.abs().max()) <= 24.0
    idle = ~(D > 0)
    assert torch.equal(idle, kind == IDLE)
    end = S.cess64(D.clamp_min(0.0), l, energy, P)
    e = S.eps_c(P, 24.0, 12.0)
    assert bool((end[kind == WHOLE] >= frac * (1.0 + e)).all()) and bool((end[kind == SEARCH] <= frac * (1.0 - e)).all())
    idx = (kind == SEARCH).nonzero()[:, 0]
    rows = (idx[:, None] * P + torch.arange(P)[None, :]).reshape(-1)
    ls, es, Ds = l[rows], energy[rows].double(), D[idx]
    assert bool(S.monotone(Ds, ls, es, P, points=129).all())
    root = S.root64(Ds, ls, es, P, frac)
    return D, idx, root, S.slack(Ds, b0[idx].double(), ls, es, P, frac, root)


def held(name, got_beta, beta, cap, kind, P, D, idx, root, slack):
    """beta' of a designed launch: equal on the rows of a group, b on IDLE groups and the ceiling on WHOLE ones to the bit, within the
    bound of the float64 root on SEARCH groups."""
    G = beta.shape[0] // P
    got = got_beta.cpu().view(G, P)
    assert bits(got, got[:, :1].expand(-1, P).contiguous()), f"{name}: beta' differs between the rows of a group"
    b0, c0, g0 = beta.view(G, P)[:, 0], cap.view(G, P)[:, 0], got[:, 0]
    assert bits(g0[kind == IDLE], b0[kind == IDLE]), f"{name}: a group at or past its ceiling moved"
    assert bits(g0[kind == WHOLE], c0[kind == WHOLE]), f"{name}: a group that meets the target at its ceiling did not reach it exactly"
    if idx.numel():
        h = D[idx] * 2.0 ** -S.HALVINGS
        err = ((g0[idx].double() - b0[idx].double()) - root) / h
        print(f"{name}: {idx.numel()} searching groups of {G}, delta32 - delta* in [{err.min():+.3f}, {err.max():+.3f}] brackets, "
              f"s up to {slack.max():.3g}")
        assert bool((err >= -(1.0 + slack)).all()) and bool((err <= slack).all()), f"{name}: beta' outside the bound of the float64 root"
        assert bool((g0[idx] > b0[idx]).all()) and bool((g0[idx] < c0[idx]).all())


# ---- 2 and 3 ----
def check_schedule_against_itself_and_float64(lsnf, sp, s, P):
    """On INIT and on end calls, with and without RESAMPLE, from a designed launch: beta' is held to float64 (`held`), and the
    resampling entry called from the same inputs with beta_next = beta' gives every output bit for bit."""
    c, dev, B = s.c, s.dev, s.c.B
    G = B // P
    init, end = c.calls[0], sp.end_calls(c)[0]
    frac_r = SG.threshold_of(P)
    sd = MG.column_scale(B, c.nz, 3, spread=1.0)
    ru = torch.rand(B, generator=torch.Generator().manual_seed(8400 + P)).to(dev)
    for r, resample, propose in ((init, None, True), (end, None, True), (end, P, True), (end, P, False)):
        name = f"[{sp.name} schedule] {c.geo} B{B} P{P} {r.phase} resample={resample} propose={propose}"
        beta, cap, pair, energy, kind = design(B, P, P + (1 if r is end else 0))
        noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, propose)
        D, idx, root, slack = expected(beta, cap, pair, energy, kind, P, FRAC)      # BEFORE the launch
        if G >= 3:
            assert all(bool((kind == k).any()) for k in (SEARCH, WHOLE, IDLE))

        def fresh():
            steps, metric = MG.same_steps(lsnf, sp, c, B, dev, 7), MG.new_metric(lsnf, s, B, sd)
            temper = TG.new_temper(lsnf, s, B, beta.to(dev), "old")
            temper.log_w.copy_(pair)
            temper.like_energy.copy_(energy)                  # (a row that rejects keeps the designed energy: module docstring)
            return steps, metric, temper
        kw = dict(propose=propose, e=energy.to(dev), resample=resample, ess_threshold=frac_r,
                  resample_uniform=ru if resample else None)
        steps, metric, temper = fresh()
        res = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, anneal=cap.to(dev), schedule=P, cess_target=FRAC, min_step=0.0, **kw)
        torch.cuda.synchronize()
        got = [t.clone() for t in everything(res, steps, metric, temper)]
        chosen = temper.beta.clone()
        held(name, chosen, beta, cap, kind, P, D, idx, root, slack)
        steps, metric, temper = fresh()
        ref = everything(SG.run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, anneal=chosen, **kw), steps, metric, temper)
        assert len(got) == len(ref)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert bits(a, b), f"{name}: output {k} differs from the resampling entry at beta_next = beta'"
        # and the scheduling entry itself without SCHEDULE, with RESAMPLE: the resampling entry's bits
        if resample:
            steps, metric, temper = fresh()
            same = everything(run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, anneal=chosen, **kw), steps, metric, temper)
            for k, (a, b) in enumerate(zip(same, ref)):
                assert bits(a, b), f"{name}: output {k} of the flagless call differs from the resampling entry"


# ---- 4 ----
def check_edge_groups(lsnf, sp, s, P):
    """The hand-made groups of tests/test_hmc_schedule_cpu.py on the device, as the first five groups of an INIT call: equal energies
    (the ceiling exactly), at the ceiling and past it (left alone), a huge spread and a NaN row (b + min_step); the other groups are a
    designed launch's and do not notice."""
    c, dev, B = s.c, s.dev, s.c.B
    r = c.calls[0]
    assert B >= 5 * P
    beta, cap, pair, energy, kind = design(B, P, 40 + P)
    ramp = torch.arange(P, dtype=torch.float32)
    blk = lambda v: torch.full((P,), v)
    beta[:5 * P] = torch.cat([blk(0.25), blk(0.75), blk(0.875), blk(0.125), blk(0.5)])
    cap[:5 * P] = torch.cat([blk(1.0), blk(0.75), blk(0.75), blk(1.0), blk(1.0)])
    pair[:5 * P, 0] = torch.cat([-0.5 * ramp, ramp, -ramp, 0.25 * ramp, -0.125 * ramp])
    pair[:5 * P, 1] = 0.0
    nan_row = 3.0 + ramp
    nan_row[P - 1] = float("nan")
    energy[:5 * P] = torch.cat([blk(7.5), 2.0 * ramp, 3.0 * ramp, 1.0e6 * ramp, nan_row])
    ms = 2.0 ** -6
    want = S.search(beta, cap, pair[:, 0] - pair[:, 1], energy, P, FRAC, ms).beta
    assert want[:5 * P].view(5, P)[:, 0].tolist() == [1.0, 0.75, 0.875, 0.125 + ms, 0.5 + ms]
    noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, True)

    def go(bt, cp, pr, en):
        steps, metric = MG.same_steps(lsnf, sp, c, B, dev, 7), MG.new_metric(lsnf, s, B)
        temper = TG.new_temper(lsnf, s, B, bt.to(dev), "nan")
        temper.log_w.copy_(pr)
        run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, anneal=cp.to(dev), schedule=P, cess_target=FRAC, min_step=ms, e=en.to(dev))
        torch.cuda.synchronize()
        return temper
    t = go(beta, cap, pair, energy)
    got = t.beta.cpu()
    assert bits(got[:5 * P], want[:5 * P]), f"[{sp.name} schedule] {c.geo} B{B} P{P}: the hand-made groups: {got[:5 * P].view(5, P)[:, 0].tolist()}"
    assert bool(torch.isnan(t.log_w[4 * P + P - 1, 0])) and not bool(torch.isnan(t.log_w[:4 * P]).any())
    # the other groups are what they are without the hand-made ones
    plain = design(B, P, 40 + P)
    other = go(*plain[:4])
    assert bits(t.beta[5 * P:], other.beta[5 * P:]) and bits(t.log_w[5 * P:], other.log_w[5 * P:])
    # rung 0's temperatures are the group's: other rungs' entries are not read
    beta2, cap2 = beta.clone(), cap.clone()
    beta2[1::P] += 0.0625
    cap2[1::P] -= 0.0625
    assert bits(go(beta2, cap2, pair, energy).beta, t.beta)


# ---- 5 ----
def check_schedule_forms(lsnf, sp, s, P):
    """The call forms of a scheduling, resampling end call that proposes, each against the plain form of the same call bit for bit: in
    place; every tensor 4 bytes off a 16-byte boundary, log_w 8 bytes off; grad_g = energy_g = None against zeros with a PhiloxNoise;
    reuse_buffers=True, two consecutive calls against two with fresh buffers; a group alone at row0 = k P against group k of the batch."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = sp.end_calls(c)[0]
    name = f"[{sp.name} schedule] {c.geo} B{B} P{P} forms"
    sd = MG.column_scale(B, c.nz, 5, spread=1.0)
    beta, cap, pair, energy, kind = design(B, P, 90 + P)
    beta_d, cap_d, e_d = beta.to(dev), cap.to(dev), energy.to(dev)
    noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, True)
    u = torch.rand(B, generator=torch.Generator().manual_seed(8500 + P)).to(dev)
    kw = dict(resample=P, ess_threshold=SG.threshold_of(P), schedule=P, cess_target=FRAC, min_step=2.0 ** -7)

    def fresh():
        steps, metric = MG.same_steps(lsnf, sp, c, B, dev, 7), MG.new_metric(lsnf, s, B, sd)
        temper = TG.new_temper(lsnf, s, B, beta_d, "old")
        temper.log_w.copy_(pair)
        return steps, metric, temper

    def same(got, ref, form):
        assert len(got) == len(ref)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert bits(a, b), f"{name}: {form}: output {k} differs from the plain form's"

    def off(t, floats=1):
        if t is None:
            return None
        t = t.float().to(dev)
        b = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
        v = b[floats: floats + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 * floats
        return v
    steps, metric, temper = fresh()
    ref = everything(run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, anneal=cap_d, resample_uniform=u, e=e_d, **kw), steps, metric, temper)
    moved = ref[len(ref) - 2 - len(TEMPER)]                   # beta after the call
    assert not bits(moved, beta_d) or B == P
    # in place
    steps, metric, temper = fresh()
    point = sp.point(r).float().to(dev).contiguous()
    res = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, point=point, inplace=True, anneal=cap_d, resample_uniform=u, e=e_d, **kw)
    assert res[1][0].data_ptr() == point.data_ptr()
    same(everything(res, steps, metric, temper), ref, "in place")
    # every tensor off its 16-byte boundary
    steps, metric, temper = fresh()
    steps = F.HmcRowSteps(off(steps.step), steps.adapt)
    metric = F.HmcRowMetric(off(metric.scale), off(metric.mean), off(metric.m2), off(metric.count))
    temper = F.HmcRowTemper(off(temper.beta), off(temper.like_grad), off(temper.like_energy), off(temper.log_w, 2))
    assert temper.log_w.data_ptr() % 16 == 8
    st = sp.T.state_for(lsnf, s, r)
    state = F.HmcState(*(off(getattr(st, f)) for f in FIELDS))
    res = run(lsnf, sp, s, r, steps, metric, temper, off(noise), off(uniform), state=state, point=off(sp.point(r)), ge=off(r.ge), e=off(energy),
              inplace=True, anneal=off(cap), resample_uniform=off(u), **kw)
    same(everything(res, steps, metric, temper), ref, "4 bytes off")
    # NULL gradient and energy are zeros (equal energies: every group that can move reaches its ceiling)
    both = []
    for gg, e in ((None, None), (torch.zeros(B, c.nz, device=dev), torch.zeros(B, device=dev))):
        steps, metric, temper = fresh()
        both.append(everything(run(lsnf, sp, s, r, steps, metric, temper, F.PhiloxNoise(8, 9, 0), None, ge=gg, e=e, anneal=cap_d, **kw),
                               steps, metric, temper))
    same(both[0], both[1], "NULL grad_g / energy_g")

    # reuse_buffers: two consecutive calls (the second from the first one's state, weights and temperatures) against fresh buffers
    def twice(reuse):
        steps, metric, temper = fresh()
        state, outs = sp.T.state_for(lsnf, s, r), []
        for _ in range(2):
            res = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, state=state, anneal=cap_d, resample_uniform=u, e=e_d,
                      reuse_buffers=reuse, **kw)
            outs.append([t.clone() for t in everything(res, steps, metric, temper)])
        return outs
    a1, a2 = twice(True)
    b1, b2 = twice(False)
    same(a1, ref, "reuse_buffers, first call"); same(b1, ref, "fresh buffers, first call")
    same(a2, b2, "reuse_buffers, second call")
    if B // P >= 3:
        assert not bits(a2[len(a2) - 2 - len(TEMPER)], a1[len(a1) - 2 - len(TEMPER)])      # beta advanced between the two calls

    # in-kernel draws, sharded along whole groups: group k alone at row0 = k P is group k of the batch
    def go(rows, row0):
        n = len(range(*rows.indices(B)))
        ws, wm, wt = fresh()
        steps, metric = F.HmcRowSteps(ws.step[rows].clone(), ws.adapt[rows].clone()), MG.new_metric(lsnf, s, n, sd[rows])
        temper = F.HmcRowTemper(*(getattr(wt, f)[rows].clone() for f in TEMPER))
        res = run(lsnf, sp, s, r, steps, metric, temper, F.PhiloxNoise(99, (7 << 32) + 5, row0), None, rows=rows, anneal=cap_d[rows].clone(),
                  e=e_d[rows].clone(), **kw)
        return everything(res, steps, metric, temper)
    batch = go(slice(0, B), 0)
    for k in sorted({0, (B // P) // 2, B // P - 1}):
        alone = go(slice(k * P, (k + 1) * P), k * P)
        for a, b in zip(batch, alone):
            assert bits(a[k * P:(k + 1) * P], b), f"{name}: group {k} alone differs from group {k} of the batch"


# ---- 6 ----
def check_captured_call(lsnf, sp, s, P=8):
    """One scheduling, resampling end call that draws in-kernel, captured in a graph and replayed twice with beta_rows advancing
    between the replays, gives the two eager calls' bits -- state, likelihood parts, weights, temperatures, ancestor and ess included."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = sp.end_calls(c)[0]
    cut = lambda t: t.float().to(dev).contiguous()
    beta, cap, pair, energy, kind = design(B, P, 70)
    point, ge, e, cap = cut(sp.point(r)), cut(r.ge), energy.to(dev), cap.to(dev)
    stash = None if sp.name == "z" else sp.T.stash_at(lsnf, s.plan, point)
    kw = dict(phase="end", propose=True, anneal=cap, resample=P, ess_threshold=0.5, schedule=P, cess_target=FRAC, min_step=2.0 ** -7)

    class Buffers:
        def __init__(self):
            self.state, self.steps, self.metric = sp.T.state_for(lsnf, s, r), F.new_hmc_row_steps(B, dev, c.s), F.new_hmc_row_metric(s.plan, B, dev)
            self.temper = TG.new_temper(lsnf, s, B, beta.to(dev), "old")
            self.temper.log_w.copy_(pair)

        def tensors(self):
            return [getattr(self.state, f) for f in FIELDS] + [self.steps.step, self.metric.scale] + [getattr(self.temper, f) for f in TEMPER]

    def step(b):
        with torch.no_grad():
            if sp.name == "z":
                out = F.hmc_step_schedule(s.plan, point, ge, e, b.state, F.PhiloxNoise(41, 9, 0), b.steps, b.metric, b.temper, **kw)
                return out[:3] + out[4:]
            return F.reverse_hmc_step_schedule(s.plan, point, stash[0], stash[1], ge, e, b.state, F.PhiloxNoise(41, 9, 0), b.steps, b.metric,
                                               b.temper, **kw)
    be = Buffers()
    eager = []
    for _ in range(2):
        out = [t.clone() for t in step(be)]
        eager.append((out, [t.clone() for t in be.tensors()]))
    assert not bits(eager[0][1][-4], eager[1][1][-4])         # beta_rows advanced between the two calls
    bg = Buffers()
    start = [t.clone() for t in bg.tensors()]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                            # warm-up off the capture stream
        step(bg)
    torch.cuda.current_stream(dev).wait_stream(side)
    for t, t0 in zip(bg.tensors(), start):
        t.copy_(t0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(bg)
    for t, t0 in zip(bg.tensors(), start):
        t.copy_(t0)
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(bits(a, b) for a, b in zip(out, eager[k][0])), f"{sp.name} replay {k}: the call's outputs"
        assert all(bits(a, b) for a, b in zip(bg.tensors(), eager[k][1])), f"{sp.name} replay {k}: state, steps, metric, temper"
    assert not bits(be.state.z, start[0])


# ---- 7 ----
def _hand_loop(lsnf, sp, net, netG, x, ph, T, C, P, L, step, thr, target, ms):
    """The adaptive sampler by hand: the same sequence of flow calls.  Returns (temper, state, resampled, steps_used, trace)."""
    F = lsnf.flow
    N, nz, dev = x.shape[0], x.shape[1], x.device
    B, plan = N * C, net._plan()
    xs = x.repeat_interleave(C, dim=0)
    z0, eps0 = net.sample(B, ph.step(0), return_eps=True)
    point = (z0 if sp.name == "z" else eps0).detach().reshape(B, nz).contiguous().clone()
    steps, metric, temper = F.new_hmc_row_steps(B, dev, step), F.new_hmc_row_metric(plan, B, dev), F.new_hmc_row_temper(plan, B, dev, 0.0)
    st, act = F.new_hmc_state(plan, B, dev), F.new_act_saved(plan, B, dev)
    ceiling = torch.ones(B, device=dev)
    used, count, trace = torch.zeros(N, C // P, device=dev), torch.zeros(N, C // P, device=dev), []
    calls = T * L + 1
    for j in range(calls):
        t, inner = j // L, j % L != 0
        phase = "inner" if inner else "end" if j else "init"
        anneals = not inner and t < T
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
        if anneals:
            used += (temper.beta.view(N, C // P, P)[:, :, 0] < 1.0).float()
        move = bool(j) and not inner and t < T
        rkw = dict(phase=phase, propose=j < calls - 1, inplace=True, anneal=ceiling if anneals else None,
                   resample=P if move else None, ess_threshold=thr,
                   schedule=P if anneals and t < T - 1 else None, cess_target=target, min_step=ms)
        with torch.no_grad():
            if sp.name == "z":
                out = net.hmc_step_schedule(point, gg, e.detach(), st, None if inner else ph.step(t + 1), steps, metric, temper, **rkw)
            else:
                out = net.reverse_hmc_step_schedule(point, saved, act, gg, e.detach(), st, None if inner else ph.step(t + 1), steps, metric, temper, **rkw)
        if move:
            count += (out[-1].view(N, C // P, P)[:, :, 0] < thr * P).float()
        else:
            assert out[-1] is None and out[-2] is None
        if anneals:
            trace.append(temper.beta.view(N, C // P, P)[:, :, 0].clone())
    return temper, st, count, used, torch.stack(trace)


def check_samplers(lsnf, sp, K, dev, monkeypatch):
    """The adaptive sampler is the hand-driven sequence of `_netF.*_schedule` calls bit for bit; its launches on the flow's side;
    `resampled` and `steps_used`; the schedule it returns; the Philox offset; `check_every` leaving early; the empty forms."""
    from counting_lib import install
    F, Lv = lsnf.flow, lsnf.langevin
    net, netG, x, _, _ = TG.ais_problem(lsnf, K, dev)
    fn = Lv.estimate_log_px_smc_adaptive_z_with_flow if sp.name == "z" else Lv.estimate_log_px_smc_adaptive_eps_with_flow
    N, C, P, T, L, nz, step, thr, target = x.shape[0], 8, 4, 8, 2, x.shape[1], 0.28, 0.9, 0.8
    B, plan = N * C, net._plan()
    kw = dict(max_steps=T, chains=C, particles=P, leapfrog_steps=L, g_l_step_size=step, g_llhd_sigma=1.0, ess_threshold=thr, cess_target=target)
    ph = F.PhiloxNoise(7, 3, 0)
    stand = install(monkeypatch, lsnf)
    log_px, log_w, ess, rate, z_T, temper, resampled, steps_used, sched = fn(x, netG, net, philox=ph, return_schedule=True, **kw)
    torch.cuda.synchronize()
    entered = dict(stand.entered)
    monkeypatch.undo()
    calls = T * L + 1
    mine = "lsnf_hmc_step_schedule" if sp.name == "z" else "lsnf_reverse_hmc_step_schedule"
    launching = {n: k for n, k in entered.items() if n in stand.launching()}
    if sp.name == "z":
        want = {"lsnf_sample": 1, "lsnf_forward": calls, mine: calls}
    elif F.reverse_keep_supported(plan, B):
        want = {"lsnf_sample": 1, "lsnf_reverse_keep": calls, "lsnf_reverse": 1, mine: calls}
    else:
        want = {"lsnf_sample": 1, "lsnf_reverse": calls + 1, "lsnf_forward": calls, mine: calls}
    assert launching == want, launching
    assert ph.offset == 3 + T + 1 and log_px.shape == (N,) and log_w.shape == (N, C) and steps_used.shape == (N, C // P)
    assert sched.shape == (T, N, C // P) and resampled.shape == (N, C // P)
    mine_t, st, count, used, trace = _hand_loop(lsnf, sp, net, netG, x, F.PhiloxNoise(7, 3, 0), T, C, P, L, step, thr, target, 1.0 / (4.0 * T))
    for f in TEMPER:
        assert bits(getattr(temper, f), getattr(mine_t, f)), f
    top = st.z if sp.name == "z" else F.reverse(plan, st.z, None)[0]
    assert bits(z_T.reshape(B, nz), top) and bits(log_w, mine_t.log_weight().view(N, C)) and bits(steps_used, used) and bits(sched, trace)
    assert bits(resampled, count) and 0 < int(count.sum()) <= (T - 1) * N * (C // P)      # some groups resampled at some steps
    assert bool((temper.beta == 1.0).all()) and bool((sched[-1] == 1.0).all()) and bool((sched[1:] >= sched[:-1]).all())
    assert bool((steps_used >= 1.0).all()) and bool((steps_used <= T).all())
    below = (sched[:-1] < 1.0).float().sum(0) + 1.0           # the annealing calls a group entered below 1: the init call and ..
    assert bits(steps_used, below)
    print(f"[{sp.name} schedule] sampler N={N} chains={C} particles={P} max_steps={T} L={L} target={target}: steps used "
          f"{steps_used.flatten().tolist()}, resampled {resampled.flatten().tolist()} of {T - 1}, final ess {[round(v, 2) for v in ess.tolist()]}")
    # check_every: a target every group meets in the init call; every weight is final after it and the second transition is the last
    easy = dict(kw, cess_target=1e-3, ess_threshold=0.0)
    ph = F.PhiloxNoise(7, 3, 0)
    full = fn(x, netG, net, philox=ph, **easy)
    assert ph.offset == 3 + T + 1 and bool((full[7] == 1.0).all()) and bool((full[6] == 0.0).all())
    ph = F.PhiloxNoise(7, 3, 0)
    stand = install(monkeypatch, lsnf)
    early = fn(x, netG, net, philox=ph, check_every=1, **easy)
    torch.cuda.synchronize()
    entered = dict(stand.entered)
    monkeypatch.undo()
    assert entered[mine] == 2 * L + 1 and ph.offset == 3 + 2 + 1
    assert bits(early[1], full[1]) and bits(early[0], full[0]) and bits(early[6], full[6]) and bits(early[7], full[7])
    ph = F.PhiloxNoise(7, 3, 0)
    late = fn(x, netG, net, philox=ph, check_every=3, **easy)
    assert ph.offset == 3 + 4 + 1 and bits(late[1], full[1])
    # nothing to do
    ph = F.PhiloxNoise(7, 3, 0)
    assert fn(x, netG, net, philox=ph, **dict(kw, max_steps=0)) == (None,) * 8 and ph.offset == 3
    none = fn(x[:0], netG, net, philox=ph, **kw)
    assert none[0].shape == (0,) and none[1].shape == (0, C) and none[3:] == (None,) * 5 and ph.offset == 3


def check_sampler_band(lsnf, sp, K, dev):
    """One seed of tests/hmc_schedule_restated.py's experiment (max_steps = 40, CESS target 0.98, 64 chains in groups of 16, L = 3)
    with the in-kernel draws: the errors against the closed form, the final ess, the mean acceptance and the steps used lie inside the
    CPU bands (profiles/smc_adaptive_cpu.txt)."""
    import ais_restated as A
    F, Lv = lsnf.flow, lsnf.langevin
    net, netG, x, exact, _ = TG.ais_problem(lsnf, K, dev)
    fn = Lv.estimate_log_px_smc_adaptive_z_with_flow if sp.name == "z" else Lv.estimate_log_px_smc_adaptive_eps_with_flow
    N, C, D, T, P = x.shape[0], A.EXP_CHAINS, x[0].numel(), S.EXP_MAX_STEPS, 16
    ph = F.PhiloxNoise(5, 10, 0)
    log_px, log_w, ess, rate, z_T, temper, resampled, steps_used = fn(x, netG, net, max_steps=T, chains=C, particles=P, leapfrog_steps=A.EXP_L,
                                                           g_l_step_size=A.EXP_STEP, g_llhd_sigma=1.0, philox=ph, cess_target=S.EXP_TARGET,
                                                           ess_threshold=0.5)
    torch.cuda.synchronize()
    band = S.BAND[sp.name]
    err = log_px.cpu() + 0.5 * D * math.log(2.0 * math.pi) - exact
    acc = rate.double().mean().item()
    print(f"[{sp.name} schedule] adaptive SMC sampler, max_steps={T}, target {S.EXP_TARGET}, L={A.EXP_L}, {C} chains in groups of {P}: errors "
          + " ".join(f"{e:+.4f}" for e in err.tolist()) + f" (band {band['error']}), ess " + " ".join(f"{e:.2f}" for e in ess.tolist())
          + f" (band {band['ess']}), mean acceptance {acc:.4f} (band {band['accept']}); steps used {steps_used.flatten().tolist()} "
          f"(band {band['steps']})")
    assert log_px.dtype == torch.float64 and log_px.shape == (N,) and log_w.shape == (N, C) and steps_used.shape == (N, C // P)
    assert resampled.shape == (N, C // P) and 0 < int(resampled.sum()) <= resampled.numel() * (T - 1)
    assert bool(((err >= band["error"][0]) & (err <= band["error"][1])).all())
    assert bool(((ess.cpu() >= band["ess"][0]) & (ess.cpu() <= band["ess"][1])).all())
    assert band["accept"][0] <= acc <= band["accept"][1]
    su = steps_used.cpu().double()
    assert bool(((su >= band["steps"][0]) & (su <= band["steps"][1])).all())
    assert bool((temper.beta == 1.0).all()) and ph.offset == 10 + T + 1

"""TEST INFRASTRUCTURE (GPU): what tests/test_gpu_hmc_resample.py (`lsnf_hmc_step_resample`, the chain on z) and
tests/test_gpu_rhmc_resample.py (`lsnf_reverse_hmc_step_resample`, the chain on eps) check, written once for both on
tests/hmc_rows_gpu.py's `Space`; the cases, teacher-forcing records, plans and `state_for` of the scalar tests and the helpers of
tests/hmc_metric_gpu.py, tests/hmc_tempered_gpu.py and tests/hmc_exchange_gpu.py are reused by import.  Bit identities are against the
tempered call or the device against itself (tests/hmc_resample_restated.py's lines as torch fp32 operations on the device's own stored
values); float64 enters in the forced decisions, and in ess_out and the new log_w, whose bounds the restatement returns.

How a decision is forced (`targets`, `forced`).  The annealing end call WITHOUT the flag is run twice: once from a zero Kahan pair,
which gives every row's increment, and once from the pair  target - increment, so that the rows end at the targets: group k's log
weights are base_k in U(-40, 40) plus, alternately, 0.1 U(-1, 1) (ess about P: the group stays) and HEAVY[P] rungs within 1 of the top
with the others 3 .. 6 below it (ess at most 1.1 / 1.4 / 2.7 / 4.5 for P = 2 / 4 / 8 / 16: the group resamples).  |l| <= 64 is
asserted.  From the second call's stored pairs the float64 decision is taken BEFORE the resampling launch.  Each group's uniform is
the first of the 64 fixed CANDIDATES whose thresholds tau_k are all at least MARGIN * err(P, 64) * S1 from every cumulative sum, with
err = 2^-24 (2 max|l| + 2 EXP_ULP + P + 2) the fp32 error of a sum or a threshold relative to S1 (tests/hmc_resample_restated.py) and
MARGIN = 50; |ess - ess_frac P| / ess must clear MARGIN * 4 err likewise.  No group may be left out: both are asserted and the nearest
group's distance is printed (profiles/hmc_resample_geometries.txt).  Rows other than a group's first are given the decoy uniform
1 - u: the kernel reads the first row's.

ess_threshold is 0.5, except at P = 2: there ess lies in [1, 2] and 0.5 P = 1 is never undercut, so no group of two can resample at
0.5; P = 2 runs at 0.75 (ess < 1.5), which the targets above separate as clearly.

The case lists are tests/hmc_exchange_gpu.py's (SWAP as MOVE, UNIFORM, FORMS): the same lanes, tiles and waves."""
import torch
import numpy as np

from oracle.philox_oracle import philox4x32_10
import hmc_exchange_gpu as XG
import hmc_metric_gpu as MG
import hmc_resample_restated as R
import hmc_rows_gpu as HG
import hmc_tempered_gpu as TG
import mala_restated as MA

bits, fig, FIELDS, METRIC, TEMPER = HG.bits, HG.fig, HG.FIELDS, MG.METRIC, TG.TEMPER
C3, TINY = HG.C3, HG.TINY
IDENTITY = HG.IDENTITY                       # every instantiation of a resampling kernel, by the dispatch rule
MOVE, UNIFORM, FORMS = XG.SWAP, XG.UNIFORM, XG.FORMS
# Added to `targets`' seed for a case of MOVE, keyed by the case, should the default draws leave a group without a candidate or a
# launch without both kinds of group.  To be chosen on the CPU from the float64 records, never from the device's answer: none needed.
DESIGN_SEED = {}
MARGIN = 50.0
LMAX = 64.0
HEAVY = {2: 1, 4: 1, 8: 2, 16: 3}
CANDIDATES = torch.tensor([0.03 + 0.94 * ((c * 0.6180339887498949) % 1.0) for c in range(64)], dtype=torch.float64).float()
ANCESTOR = -2                                # `ancestor` in `whole` of a resampling call's result


def threshold_of(P):
    return 0.75 if P == 2 else 0.5


def run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, rows=slice(None), state=None, adapt=None, window=None, propose=True,
        anneal=None, resample=None, ess_threshold=0.5, resample_uniform=None, e="record", ge="record", point=None, inplace=False,
        reuse_buffers=False):
    """The recorded call r on its rows from its inputs' casts through the resampling wrapper: (state after, [next point, accepted,
    log_alpha, ancestor, ess])."""
    F, dev = lsnf.flow, s.dev
    cut = lambda t: None if t is None else t[rows].float().to(dev).contiguous()
    state = sp.T.state_for(lsnf, s, r, rows) if state is None else state
    kw = dict(phase=r.phase, uniform=uniform, propose=propose, adapt=adapt, window=window, anneal=anneal, resample=resample,
              ess_threshold=ess_threshold, resample_uniform=resample_uniform, inplace=inplace, reuse_buffers=reuse_buffers)
    point = cut(sp.point(r)) if point is None else point
    e = cut(r.e) if isinstance(e, str) else e
    ge = cut(r.ge) if isinstance(ge, str) else ge
    if sp.name == "z":
        out = F.hmc_step_resample(s.plan, point, ge, e, state, noise, steps, metric, temper, **kw)
        out = out[:3] + out[4:]
    else:
        saved, act = sp.T.stash_at(lsnf, s.plan, point)
        out = F.reverse_hmc_step_resample(s.plan, point, saved, act, ge, e, state, noise, steps, metric, temper, **kw)
    return state, list(out)


def whole(res, steps, metric, temper):
    state, out = res
    return TG.flat((state, out[:3]), steps, metric, temper) + [out[3], out[4]]


# ---- 1 ----
def check_no_resample_is_the_tempered_call(lsnf, sp, s):
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
                ref = TG.flat(TG.run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, propose=propose, adapt=adapt, window=window,
                                     anneal=anneal), steps, metric, temper)
                steps, metric, temper = fresh()
                state, out = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, propose=propose, adapt=adapt, window=window,
                                 anneal=anneal)
                assert out[3] is None and out[4] is None     # nothing is written without the move: there is nothing to write to
                got = TG.flat((state, out[:3]), steps, metric, temper)
                name = f"{sp.name} {c.geo} B{B} {r.phase} propose={propose} {how} adapt={adapt} window={window} anneal={anneal is not None}"
                assert len(got) == len(ref)
                for k, (a, b) in enumerate(zip(got, ref)):
                    assert bits(a, b), f"{name}: output {k} differs"


# ---- 2 ----
def targets(B, P, first_resamples, seed=0):
    """(B) fp32: the log weights the rows are to end at (module docstring); group k is meant to resample iff (k even) ==
    first_resamples."""
    g = torch.Generator().manual_seed(8000 + seed)
    G = B // P
    base = (-40.0 + 80.0 * torch.rand(G, generator=g))[:, None]
    flat = 0.1 * (2.0 * torch.rand(G, P, generator=g) - 1.0)
    low = -(3.0 + 3.0 * torch.rand(G, P, generator=g))
    order = torch.rand(G, P, generator=g).argsort(dim=1)     # the ranks of the rungs: the HEAVY[P] first are near the top
    top = -torch.rand(G, P, generator=g)
    top = torch.where(order == 0, torch.zeros(G, P), top)
    steep = torch.where(order < HEAVY[P], top, low)
    want = (torch.arange(G) % 2 == 0) == first_resamples
    return (base + torch.where(want[:, None], steep, flat)).reshape(-1).float(), want


def forced(l32, P, ess_frac):
    """From the rows' fp32 log weights: (u (B) fp32 -- the group's uniform at its first row, the decoy 1 - u on the others --, the
    float64 decision with that u, the least threshold and ess distances in units of err(P, LMAX)).  No group is left out: a group
    without a candidate fails the assertion here."""
    l64 = l32.double().cpu()
    G = l64.shape[0] // P
    d0 = R.decide(l64, torch.zeros_like(l64), P, ess_frac)
    cand = CANDIDATES.double()
    k = torch.arange(P, dtype=torch.float64)
    pick = torch.zeros(G, dtype=torch.long)
    for lo in range(0, G, 256):                              # (in slabs: G * 64 * P * P numbers)
        s1, cum = d0.s1[lo:lo + 256], d0.cum[lo:lo + 256]
        tau = ((k[None, None, :] + cand[None, :, None]) / P) * s1[:, None, None]
        gap = (cum[:, None, None, :] - tau[..., None]).abs().flatten(2).min(dim=2).values / s1[:, None]
        ok = (gap >= MARGIN * R.err(P, LMAX)) | ~d0.group_on[lo:lo + 256, None]
        assert bool(ok.any(dim=1).all()), "a group has no candidate uniform that clears the margin"
        pick[lo:lo + 256] = ok.float().argmax(dim=1)
    ug = CANDIDATES[pick]
    u = torch.stack([ug] + [1.0 - ug] * (P - 1), dim=1).reshape(-1).float()
    d = R.decide(l64, u.double(), P, ess_frac)
    gap, edge = R.margins(d, P, ess_frac, LMAX)
    return u, d, gap, edge


def preload(lsnf, sp, s, r, B, P, beta, bn, sd, noise, uniform, propose, want_first, seed):
    """The Kahan pairs (B, 2) from which the annealing end call ends at `targets`: target - increment, the increment being what the
    same call leaves in a zero pair."""
    dev = s.dev
    steps, metric = MG.same_steps(lsnf, sp, s.c, B, dev, 7), MG.new_metric(lsnf, s, B, sd)
    temper = TG.new_temper(lsnf, s, B, beta, "old")
    temper.log_w.zero_()
    run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, propose=propose, anneal=bn)
    inc = temper.log_w[:, 0] - temper.log_w[:, 1]
    tgt, want = targets(B, P, want_first, seed)
    pair = torch.zeros(B, 2, device=dev)
    pair[:, 0] = tgt.to(dev) - inc
    return pair, want


def check_move_bits(lsnf, sp, s, P):
    """From the device's own stored state after the same annealing call WITHOUT the flag, the header's fp32 lines hold to the bit;
    temperatures, steps, scales and accumulators do not move; rows that keep their state have the plain call's bits."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = sp.end_calls(c)[0]
    frac = threshold_of(P)
    sd = MG.column_scale(B, c.nz, 3, spread=1.0)
    beta = TG.beta_rows(B, 5, lo=0.1, hi=0.9).to(dev)
    bn = TG.next_beta(beta, 5)
    seen_move = seen_on = seen_off = False
    for propose in (True, False):
        for first in (True, False):
            name = f"[{sp.name} resample] {c.geo} B{B} P{P} propose={propose} first_resamples={first}"
            noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, propose)
            pair, want = preload(lsnf, sp, s, r, B, P, beta, bn, sd, noise, uniform, propose, first, P + DESIGN_SEED.get(c.geo + (B, P), 0))

            def call(**kw):
                steps, metric = MG.same_steps(lsnf, sp, c, B, dev, 7), MG.new_metric(lsnf, s, B, sd)
                temper = TG.new_temper(lsnf, s, B, beta, "old")
                temper.log_w.copy_(pair)
                before = (steps.step.clone(), steps.adapt.clone(), MG.clone_metric(lsnf, metric))
                state, out = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, propose=propose, anneal=bn, **kw)
                return state, out, steps, metric, temper, before
            sa, oa, _, _, ta, _ = call()
            torch.cuda.synchronize()
            # the float64 restatement of the decisions, from the plain call's stored Kahan pairs: BEFORE the resampling launch
            l32 = ta.log_w[:, 0] - ta.log_w[:, 1]
            assert float(l32.abs().max()) <= LMAX
            u, d64, gap, edge = forced(l32, P, frac)
            G = B // P
            assert gap >= MARGIN and edge >= MARGIN, f"{name}: a group is near a tie ({gap:.3g} / {edge:.3g} of err)"
            on, rung, anc = d64.on, d64.rung, d64.ancestor
            moved = anc != torch.arange(B)
            print(f"{name}: {int(d64.group_on.sum())} of {G} groups resample, {int(moved.sum())} rows take another row's state; nearest "
                  f"threshold at {gap:.3g} err, nearest ess at {edge:.3g} x 4 err from its edge")
            assert torch.equal(d64.group_on, want), f"{name}: the targets did not give the meant decisions"
            seen_move, seen_on, seen_off = seen_move or bool(moved.any()), seen_on or bool(on.any()), seen_off or bool((~on).any())
            if G > 1:
                assert bool(on.any()) and bool((~on).any()) and bool(moved.any()), f"{name}: the launch needs both kinds of group"
            sb, ob, steps, metric, tb, (step0, adapt0, metric0) = call(resample=P, ess_threshold=frac, resample_uniform=u.to(dev))
            torch.cuda.synchronize()
            on_d, moved_d = on.to(dev), moved.to(dev)
            # the trajectory's own decision and outputs
            assert bits(ob[1], oa[1]) and bits(ob[2], oa[2]) and bits(sb.kin, sa.kin), f"{name}: accepted / log_alpha / kin0"
            # the move's outputs
            assert bits(ob[3], rung.float().to(dev)), f"{name}: ancestor is not the float64 decision"
            rel_ess, abs_lw = R.bounds(d64, P, LMAX)
            e = ((ob[4].cpu().double() - d64.ess).abs() / d64.ess) / rel_ess
            print(f"{name}: worst |ess - fp64| / bound = {fig(e):.3f}")
            assert bool((e <= 1.0).all()), f"{name}: ess_out"
            e = (tb.log_w[:, 0].cpu().double() - d64.lw).abs()[on] / abs_lw[on]
            print(f"{name}: worst |log_w' - fp64| / bound = {fig(e):.3f}")
            assert bool((e <= 1.0).all()) and bool((tb.log_w[:, 1][on_d] == 0.0).all()), f"{name}: the new Kahan pair"
            lw = tb.log_w[:, 0].view(G, P)[d64.group_on.to(dev)]
            assert bits(lw, lw[:, :1].expand(-1, P).contiguous()), f"{name}: the rows of a resampling group differ in their new weight"
            # the moved state: the header's lines in fp32 on the plain call's stored arrays, at the rows' temperatures after the anneal
            z, g, uu, gl, el = R.gather(ta.beta, sa.z, sa.grad, sa.energy, ta.like_grad, ta.like_energy, anc.to(dev))
            for f, got, ref in (("state.z", sb.z, z), ("state.grad", sb.grad, g), ("state.energy", sb.energy, uu),
                                ("like_grad", tb.like_grad, gl), ("like_energy", tb.like_energy, el)):
                assert bits(got, ref), f"{name}: {f} differs from the restated gather"
            if bool(moved.any()):
                assert not bits(sb.z[moved_d], sa.z[moved_d]) and not bits(sb.grad[moved_d], sa.grad[moved_d])
            # what must not move: the temperatures, the steps, the metric and its accumulators
            assert bits(tb.beta, ta.beta) and bits(tb.beta, bn), f"{name}: beta moved"
            assert bits(steps.step, step0) and bits(steps.adapt, adapt0) and MG.untouched(metric, metric0), f"{name}: steps / metric moved"
            # rows that keep their state have the plain call's bits -- but for log_w in a resampling group
            stay = ~moved_d
            for a, b in zip(HG.flat((sb, ob[:3])), HG.flat((sa, oa[:3]))):
                assert bits(a[stay], b[stay]), f"{name}: a row that kept its state differs from the plain call"
            for a, b in zip(TG.flat((sb, ob[:3]), steps, metric, tb), TG.flat((sa, oa[:3]), steps, metric, ta)):
                assert bits(a[~on_d], b[~on_d]), f"{name}: a row of a group that did not resample differs from the plain call"
            assert bits(ob[3][~on_d], (torch.arange(B) % P).float().to(dev)[~on_d])
            if not propose:                                  # nothing begun: the full-step momentum of the plain call, on every row
                assert ob[0] is None and bits(sb.mom, sa.mom)
                continue
            # the next trajectory begins from the RESAMPLED state with the row's own step, scale and xi
            st, sdd = steps.step[:, None], metric.scale
            ph = noise - (0.5 * st) * (sdd * sb.grad)
            assert bits(sb.mom, ph), f"{name}: mom is not xi - (0.5 s) (sd grad_acc')"
            assert bits(ob[0], sb.z + st * (sdd * ph)), f"{name}: the next point is not z_state' + s (sd mom)"
            if bool(moved.any()):
                assert not bits(sb.mom[moved_d], sa.mom[moved_d])
    assert seen_move and seen_on and seen_off, f"[{sp.name} resample] {c.geo} B{B} P{P}: the case needs a moving row and both kinds of group"


# ---- 3 ----
def check_always_and_never(lsnf, sp, s, P):
    """ess_threshold = 2 resamples every group, 0 none (the plain call's bits); with equal weights in a group every ancestor is the row
    itself whatever u is, and a resampling call leaves the plain call's bits."""
    c, dev, B = s.c, s.dev, s.c.B
    r = sp.end_calls(c)[0]
    beta = TG.beta_rows(B, 5, lo=0.1, hi=0.9).to(dev)
    bn = TG.next_beta(beta, 5)
    noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, True)
    own = (torch.arange(B) % P).float().to(dev)
    u = torch.rand(B, generator=torch.Generator().manual_seed(8100)).to(dev)

    def call(anneal, pair, **kw):
        steps, metric = MG.same_steps(lsnf, sp, c, B, dev, 7), MG.new_metric(lsnf, s, B)
        temper = TG.new_temper(lsnf, s, B, beta, "old")
        temper.log_w.copy_(pair)
        return whole(run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, anneal=anneal, **kw), steps, metric, temper)
    pair = TG.weights_at(TG.new_temper(lsnf, s, B, beta, "old")).log_w.clone()
    pair[:, 0] = 0.3 * pair[:, 0]                            # (spread 3 within a group)
    plain = call(bn, pair)
    never = call(bn, pair, resample=P, ess_threshold=0.0, resample_uniform=u)
    for k, (a, b) in enumerate(zip(never[:-2], plain[:-2])):
        assert bits(a, b), f"ess_threshold = 0: output {k} differs from the plain call"
    assert bits(never[ANCESTOR], own) and bool((never[-1] >= 1.0).all()) and bool((never[-1] <= P * (1.0 + 1e-5)).all())
    always = call(bn, pair, resample=P, ess_threshold=2.0, resample_uniform=u)
    lw = always[-3]
    assert bool((lw[:, 1] == 0.0).all()) and bits(lw[:, 0].view(-1, P), lw[:, 0].view(-1, P)[:, :1].expand(-1, P).contiguous())
    anc = always[ANCESTOR].view(-1, P)
    assert bool((anc[:, 1:] >= anc[:, :-1]).all()) and bool((anc >= 0).all()) and bool((anc <= P - 1).all())      # systematic: sorted
    assert bits(always[-1], never[-1])
    # equal weights: d = 0 leaves the preloaded pair {base_k, 0} as it is; e_i = 1, cum_j = j + 1, tau_k = k + u: a_k = k
    base = (-40.0 + 80.0 * torch.rand(B // P, generator=torch.Generator().manual_seed(8101)))[:, None].expand(-1, P).reshape(-1)
    pair = torch.stack([base, torch.zeros(B)], dim=1).to(dev)
    plain = call(beta, pair)
    for ug in (0.0, 0.5, 1.0 - 2.0 ** -12, None):
        uu = u if ug is None else torch.full((B,), ug, device=dev)
        same = call(beta, pair, resample=P, ess_threshold=2.0, resample_uniform=uu)
        for k, (a, b) in enumerate(zip(same[:-2], plain[:-2])):
            assert bits(a, b), f"equal weights, u={ug}: output {k} differs from the plain call"
        assert bits(same[ANCESTOR], own) and bits(same[-1], torch.full((B,), float(P), device=dev))


# ---- 4 ----
def resample_uniform_draws(B, seed, offset=0, row0=0):
    """(B,) np.float32: mala_restated.uniform_draws at field value 4 of the counter instead of 2 -- the number the kernel draws for the
    group whose first row is row0 + sample."""
    mask = np.uint64(0xFFFFFFFF)
    rows = np.arange(B, dtype=np.uint64) + np.uint64(row0)
    c3 = np.uint64((offset >> 32) & 0xFFFFFFFF) ^ (rows >> np.uint64(32))
    x0 = philox4x32_10(np.uint64(4 << 16), rows & mask, np.uint64(offset & 0xFFFFFFFF), c3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return ((x0 >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def check_in_kernel_uniform(lsnf, sp, s, P):
    """With a PhiloxNoise the group's uniform is Philox at field 4 of its first row's counter: the call is the tensor form's with the
    restated draws, bit for bit; a group alone at row0 = k P gives group k of the whole batch; the trajectory's and the swap's
    uniforms in its place give other ancestors.  Every group is made to resample (ess_threshold = 2) from a Kahan pair spread by 3."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = sp.end_calls(c)[0]
    seed, offset = 99, (7 << 32) + 5
    beta = TG.beta_rows(B, 6, lo=0.1, hi=0.9).to(dev)
    bn = TG.next_beta(beta, 6)
    u_traj, u_swap, u_res = MA.uniform_draws(B, seed, offset), XG.swap_uniform_draws(B, seed, offset), resample_uniform_draws(B, seed, offset)
    assert not np.any(u_traj == u_res) and not np.any(u_swap == u_res)
    pair = TG.weights_at(TG.new_temper(lsnf, s, B, beta, "old")).log_w.clone()
    pair[:, 0] = 0.3 * pair[:, 0]

    def go(rows, row0, how, propose=True):
        n = len(range(*rows.indices(B)))
        whole_steps, wt = MG.same_steps(lsnf, sp, c, B, dev, 7), TG.new_temper(lsnf, s, B, beta, "old")
        wt.log_w.copy_(pair)
        steps, metric = F.HmcRowSteps(whole_steps.step[rows].clone(), whole_steps.adapt[rows].clone()), MG.new_metric(lsnf, s, n)
        temper = F.HmcRowTemper(*(getattr(wt, f)[rows].clone() for f in TEMPER))
        if isinstance(how, str):                             # "philox"; else the move's uniforms, with the restated trajectory's
            noise, uniform, ru = F.PhiloxNoise(seed, offset, row0), None, None
        else:
            noise, uniform, ru = None, torch.from_numpy(u_traj)[rows].to(dev), torch.from_numpy(how)[rows].to(dev)
        res = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, rows=rows, propose=propose, anneal=bn[rows].clone(), resample=P,
                  ess_threshold=2.0, resample_uniform=ru)
        return whole(res, steps, metric, temper)
    batch = go(slice(0, B), 0, "philox")
    own = (torch.arange(B) % P).float().to(dev)
    assert not bits(batch[ANCESTOR], own)                    # some row takes another row's state
    for k in range(B // P):                                  # a group alone, sharded at its first row
        alone = go(slice(k * P, (k + 1) * P), k * P, "philox")
        for a, b in zip(batch, alone):
            assert bits(a[k * P:(k + 1) * P], b), f"{sp.name}: group {k} alone differs from group {k} of the batch"
    drawn, given = go(slice(0, B), 0, "philox", propose=False), go(slice(0, B), 0, u_res, propose=False)
    for a, b in zip(drawn, given):
        assert bits(a, b), f"{sp.name}: the in-kernel uniform is not Philox at field 4 of the group's first row"
    for other in (u_traj, u_swap):
        assert not bits(go(slice(0, B), 0, other, propose=False)[ANCESTOR], drawn[ANCESTOR])


# ---- 5 ----
def check_move_forms(lsnf, sp, s, P):
    """The call forms of a resampling end call that proposes, each against the plain form of the same call bit for bit: in place;
    every tensor 4 bytes off a 16-byte boundary, log_w 8 bytes off; grad_g = energy_g = None against zeros with a PhiloxNoise;
    reuse_buffers=True, two consecutive calls against two calls with fresh buffers.  The decisions are forced as `check_move_bits`
    forces them."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = sp.end_calls(c)[0]
    name, frac = f"[{sp.name} resample] {c.geo} B{B} P{P} forms", threshold_of(P)
    sd = MG.column_scale(B, c.nz, 5, spread=1.0)
    beta = TG.beta_rows(B, 7, lo=0.1, hi=0.9).to(dev)
    bn = TG.next_beta(beta, 7)
    noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, True)
    pair, want = preload(lsnf, sp, s, r, B, P, beta, bn, sd, noise, uniform, True, True, 90 + P)

    def fresh(start=None):
        steps, metric = MG.same_steps(lsnf, sp, c, B, dev, 7), MG.new_metric(lsnf, s, B, sd)
        temper = TG.new_temper(lsnf, s, B, beta, "old")
        temper.log_w.copy_(pair if start is None else start)
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
    run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, anneal=bn)
    torch.cuda.synchronize()
    u, d64, gap, edge = forced(temper.log_w[:, 0] - temper.log_w[:, 1], P, frac)
    moved = d64.ancestor != torch.arange(B)
    assert gap >= MARGIN and edge >= MARGIN and bool(moved.any()) and bool((~d64.on).any()), f"{name}: the call needs both kinds of group"
    u = u.to(dev)
    kw = dict(resample=P, ess_threshold=frac)
    steps, metric, temper = fresh()
    ref = whole(run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, anneal=bn, resample_uniform=u, **kw), steps, metric, temper)
    assert bits(ref[ANCESTOR], d64.rung.float().to(dev)), f"{name}: ancestor is not the float64 decision"
    # in place: the next point over the point
    steps, metric, temper = fresh()
    point = sp.point(r).float().to(dev).contiguous()
    res = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, point=point, inplace=True, anneal=bn, resample_uniform=u, **kw)
    assert res[1][0].data_ptr() == point.data_ptr()
    same(whole(res, steps, metric, temper), ref, "in place")
    # every tensor off its 16-byte boundary
    steps, metric, temper = fresh()
    steps = F.HmcRowSteps(off(steps.step), steps.adapt)
    metric = F.HmcRowMetric(off(metric.scale), off(metric.mean), off(metric.m2), off(metric.count))
    temper = F.HmcRowTemper(off(temper.beta), off(temper.like_grad), off(temper.like_energy), off(temper.log_w, 2))
    assert temper.log_w.data_ptr() % 16 == 8
    st = sp.T.state_for(lsnf, s, r)
    state = F.HmcState(*(off(getattr(st, f)) for f in FIELDS))
    res = run(lsnf, sp, s, r, steps, metric, temper, off(noise), off(uniform), state=state, point=off(sp.point(r)), ge=off(r.ge), e=off(r.e),
              inplace=True, anneal=off(bn), resample_uniform=off(u), **kw)
    same(whole(res, steps, metric, temper), ref, "4 bytes off")
    # NULL gradient and energy are zeros
    rng, both = F.PhiloxNoise(8, 9, 0), []
    for gg, e in ((None, None), (torch.zeros(B, c.nz, device=dev), torch.zeros(B, device=dev))):
        steps, metric, temper = fresh()
        both.append(whole(run(lsnf, sp, s, r, steps, metric, temper, rng, None, ge=gg, e=e, anneal=bn, **kw), steps, metric, temper))
    same(both[0], both[1], "NULL grad_g / energy_g")

    # reuse_buffers: two consecutive calls (the second from the first one's state and weights) against the same two with fresh buffers
    def twice(reuse):
        steps, metric, temper = fresh()
        state, outs, ptrs = sp.T.state_for(lsnf, s, r), [], []
        for _ in range(2):
            res = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, state=state, anneal=bn, resample_uniform=u, reuse_buffers=reuse, **kw)
            outs.append([t.clone() for t in whole(res, steps, metric, temper)])
            ptrs.append((res[1][3].data_ptr(), res[1][4].data_ptr()))
        return outs, ptrs
    (a1, a2), kept_ptrs = twice(True)
    (b1, b2), _ = twice(False)
    assert kept_ptrs[0] == kept_ptrs[1]                      # (ancestor and ess live on the plan)
    same(a1, ref, "reuse_buffers, first call"); same(b1, ref, "fresh buffers, first call")
    same(a2, b2, "reuse_buffers, second call")


# ---- 6 ----
def check_a_nan_row(lsnf, sp, s, P):
    """A NaN log weight in one row leaves its group unresampled (the plain call's bits, the NaN included) and the others untouched."""
    c, dev, B = s.c, s.dev, s.c.B
    r = sp.end_calls(c)[0]
    bad = P + 1                                              # (a row of the second group)
    beta = TG.beta_rows(B, 8, lo=0.1, hi=0.9).to(dev)
    bn = TG.next_beta(beta, 8)
    noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, True)
    u = torch.rand(B, generator=torch.Generator().manual_seed(8200)).to(dev)
    pair = TG.weights_at(TG.new_temper(lsnf, s, B, beta, "old")).log_w.clone()
    pair[:, 0] = 0.3 * pair[:, 0]

    def call(pair, **kw):
        steps, metric = MG.same_steps(lsnf, sp, c, B, dev, 7), MG.new_metric(lsnf, s, B)
        temper = TG.new_temper(lsnf, s, B, beta, "old")
        temper.log_w.copy_(pair)
        return whole(run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, anneal=bn, **kw), steps, metric, temper)
    kw = dict(resample=P, ess_threshold=2.0, resample_uniform=u)
    clean = call(pair, **kw)
    spoilt = pair.clone()
    spoilt[bad, 0] = float("nan")
    plain, got = call(spoilt), call(spoilt, **kw)
    grp = torch.zeros(B, dtype=torch.bool, device=dev)
    grp[P:2 * P] = True
    for k, (a, b) in enumerate(zip(got[:-2], plain[:-2])):
        assert bits(a[grp], b[grp]), f"output {k}: the group of the NaN row differs from the plain call"
    assert bits(got[ANCESTOR][grp], (torch.arange(B) % P).float().to(dev)[grp]) and bool(torch.isnan(got[-1][grp]).all())
    for k, (a, b) in enumerate(zip(got, clean)):
        assert bits(a[~grp], b[~grp]), f"output {k}: another group differs from the run without the NaN"
    assert not bits(clean[ANCESTOR][~grp], (torch.arange(B) % P).float().to(dev)[~grp])


# ---- 7 ----
def check_samplers(lsnf, sp, K, dev, monkeypatch):
    """The SMC sampler is the hand-driven sequence of `_netF.*_resample` calls bit for bit; its launches on the flow's side; `resampled`;
    the Philox offset; the empty forms."""
    from counting_lib import install
    F, Lv = lsnf.flow, lsnf.langevin
    net, netG, x, _, _ = TG.ais_problem(lsnf, K, dev)
    fn = Lv.estimate_log_px_smc_z_with_flow if sp.name == "z" else Lv.estimate_log_px_smc_eps_with_flow
    N, C, P, T, L, nz, step, thr = x.shape[0], 8, 4, 6, 2, x.shape[1], 0.28, 0.9
    B, plan = N * C, net._plan()
    betas = Lv.ais_schedule(T)
    kw = dict(betas=betas, chains=C, particles=P, leapfrog_steps=L, g_l_step_size=step, g_llhd_sigma=1.0, ess_threshold=thr)
    ph = F.PhiloxNoise(7, 3, 0)
    stand = install(monkeypatch, lsnf)
    log_px, log_w, ess, rate, z_T, temper, resampled = fn(x, netG, net, philox=ph, **kw)
    torch.cuda.synchronize()
    entered = dict(stand.entered)
    monkeypatch.undo()
    calls = T * L + 1
    mine = "lsnf_hmc_step_resample" if sp.name == "z" else "lsnf_reverse_hmc_step_resample"
    launching = {n: k for n, k in entered.items() if n in stand.launching()}
    if sp.name == "z":
        want = {"lsnf_sample": 1, "lsnf_forward": calls, mine: calls}
    elif F.reverse_keep_supported(plan, B):
        want = {"lsnf_sample": 1, "lsnf_reverse_keep": calls, "lsnf_reverse": 1, mine: calls}
    else:
        want = {"lsnf_sample": 1, "lsnf_reverse": calls + 1, "lsnf_forward": calls, mine: calls}
    assert launching == want, launching
    assert ph.offset == 3 + T + 1 and log_px.shape == (N,) and log_w.shape == (N, C) and resampled.shape == (N, C // P)
    # by hand: the same sequence of flow calls
    ph = F.PhiloxNoise(7, 3, 0)
    xs = x.repeat_interleave(C, dim=0)
    z0, eps0 = net.sample(B, ph.step(0), return_eps=True)
    point = (z0 if sp.name == "z" else eps0).detach().reshape(B, nz).contiguous().clone()
    steps, metric, mine_t = F.new_hmc_row_steps(B, dev, step), F.new_hmc_row_metric(plan, B, dev), F.new_hmc_row_temper(plan, B, dev, 0.0)
    st, act = F.new_hmc_state(plan, B, dev), F.new_act_saved(plan, B, dev)
    rows = lambda t: torch.full((B,), float(betas[t]), dtype=torch.float32, device=dev)
    count, esses = torch.zeros(N, C // P, device=dev), []
    for j in range(calls):
        t, inner = j // L, j % L != 0
        phase = "inner" if inner else "end" if j else "init"
        anneal = rows(t + 1) if not inner and t < T else None
        move = bool(j) and not inner and t < T
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
        rkw = dict(phase=phase, propose=j < calls - 1, inplace=True, anneal=anneal, resample=P if move else None, ess_threshold=thr)
        with torch.no_grad():
            if sp.name == "z":
                out = net.hmc_step_resample(point, gg, e.detach(), st, noise, steps, metric, mine_t, **rkw)
            else:
                out = net.reverse_hmc_step_resample(point, saved, act, gg, e.detach(), st, noise, steps, metric, mine_t, **rkw)
        if move:
            esses.append(out[-1].clone())
            count += (out[-1].view(N, C // P, P)[:, :, 0] < thr * P).float()
        else:
            assert out[-1] is None and out[-2] is None
    for f in TEMPER:
        assert bits(getattr(temper, f), getattr(mine_t, f)), f
    top = st.z if sp.name == "z" else F.reverse(plan, st.z, None)[0]
    assert bits(z_T.reshape(B, nz), top) and bits(log_w, mine_t.log_weight().view(N, C)) and bits(resampled, count)
    assert len(esses) == T - 1 and 0 < int(count.sum()) < (T - 1) * N * (C // P)      # some groups resampled at some steps, not all at all
    print(f"[{sp.name} resample] sampler N={N} chains={C} particles={P} T={T} L={L}: resampled {count.flatten().tolist()} of {T - 1}, "
          f"final ess {[round(v, 2) for v in ess.tolist()]}")
    # nothing to do
    ph = F.PhiloxNoise(7, 3, 0)
    assert fn(x, netG, net, philox=ph, **dict(kw, betas=[0.0])) == (None,) * 7 and ph.offset == 3
    none = fn(x[:0], netG, net, philox=ph, **kw)
    assert none[0].shape == (0,) and none[1].shape == (0, C) and none[3:] == (None,) * 4 and ph.offset == 3


# ---- 9: both samplers on the CPU experiment's problem ----
def check_sampler_band(lsnf, sp, K, dev):
    """One seed of tests/smc_restated.py's experiment at the short schedule (T = 20, 64 chains in groups of 16, L = 3) with the
    in-kernel draws: the errors against the closed form, the final ess and the mean acceptance lie inside the CPU bands
    (profiles/smc_cpu.txt); the resampling counts are plausible."""
    import math
    import ais_restated as A
    import smc_restated as S
    F, Lv = lsnf.flow, lsnf.langevin
    net, netG, x, exact, _ = TG.ais_problem(lsnf, K, dev)
    fn = Lv.estimate_log_px_smc_z_with_flow if sp.name == "z" else Lv.estimate_log_px_smc_eps_with_flow
    N, C, D, T, P = x.shape[0], A.EXP_CHAINS, x[0].numel(), S.SHORT_T, S.EXP_PARTICLES
    ph = F.PhiloxNoise(5, 10, 0)
    log_px, log_w, ess, rate, z_T, temper, resampled = fn(x, netG, net, betas=Lv.ais_schedule(T), chains=C, particles=P, leapfrog_steps=A.EXP_L,
                                                          g_l_step_size=A.EXP_STEP, g_llhd_sigma=1.0, philox=ph, ess_threshold=S.EXP_THRESHOLD)
    torch.cuda.synchronize()
    band = S.BAND["smc"][T][sp.name]
    err = log_px.cpu() + 0.5 * D * math.log(2.0 * math.pi) - exact
    acc = rate.double().mean().item()
    print(f"[{sp.name} resample] SMC sampler, T={T}, L={A.EXP_L}, {C} chains in groups of {P}, step {A.EXP_STEP}: errors log Z_hat - closed form "
          + " ".join(f"{e:+.4f}" for e in err.tolist()) + f" (band {band['error']}), ess " + " ".join(f"{e:.2f}" for e in ess.tolist())
          + f" (band {band['ess']}), mean acceptance {acc:.4f} (band {band['accept']}); resampled {resampled.flatten().tolist()} of {T - 1}")
    assert log_px.dtype == torch.float64 and log_px.shape == (N,) and log_w.shape == (N, C) and resampled.shape == (N, C // P)
    assert bool(((err >= band["error"][0]) & (err <= band["error"][1])).all())
    assert bool(((ess.cpu() >= band["ess"][0]) & (ess.cpu() <= band["ess"][1])).all())
    assert band["accept"][0] <= acc <= band["accept"][1]
    assert bool((temper.beta == 1.0).all()) and ph.offset == 10 + T + 1
    assert 0 < int(resampled.sum()) < resampled.numel() * (T - 1)

"""TEST INFRASTRUCTURE (GPU): what tests/test_gpu_hmc_exchange.py (`lsnf_hmc_step_exchange`, the chain on z) and
tests/test_gpu_rhmc_exchange.py (`lsnf_reverse_hmc_step_exchange`, the chain on eps) check, written once for both on
tests/hmc_rows_gpu.py's `Space`: the scalar tests' cases, teacher-forcing records, plans and `state_for`, tests/hmc_metric_gpu.py's and
tests/hmc_tempered_gpu.py's helpers are reused by import.  Bit identities are against the tempered call or the device against itself
(tests/hmc_exchange_restated.py's lines as torch fp32 operations on the device's own stored values); float64 enters in the forced
swap decisions and in the next trajectory of a swapping call.

How a swap is forced (`design`, `forced`): the call without the swap is run first and its stored like_energy gives the float64 log_r of
every pair; pair k is meant to swap or not alternately and gets u = exp(log_r -+ 1), clipped into (0, 1).  A pair with log_r >= 0 swaps
whatever u is (`forced` lets it), so a pair meant to reject is given temperatures ordered against its energies: the kept like_energy of a row is set to
the record's energy + 2^-9 (1 + row % 3), so that el_s is within 0.006 of the record's energy whether the row accepts or not and the
sign of e = el_s_a - el_s_b is known beforehand wherever the records differ by more.  The float64 decision is taken with the fp32 u the
kernel is given, and no pair may be nearer to a tie than 1e-4 (1 + |log_r|) -- some fifty times what fp32 can move log(u) - log_r.

The case lists (SWAP, NEXT, UNIFORM, FORMS) hold C3 / TINY / C5 and the geometry classes of tests/chain_geometries.py;
tests/test_chain_geometries_cpu.py holds them to that table.  `check_swap_forms` compares call forms of a swapping call with its plain
form.  No check here has a tolerance of its own: bit identities, and hmc_metric_gpu.gates for the next trajectory."""
import copy
import types

import numpy as np
import torch

from oracle.philox_oracle import philox4x32_10
import chain_geometries as G
import hmc_exchange_restated as X
import hmc_metric_gpu as MG
import hmc_rows_gpu as HG
import hmc_tempered_gpu as TG
import mala_restated as MA
import rmala_restated as RM

bits, fig, FIELDS, METRIC, TEMPER = HG.bits, HG.fig, HG.FIELDS, MG.METRIC, TG.TEMPER
C3, TINY = HG.C3, HG.TINY
IDENTITY = HG.IDENTITY                       # every instantiation of an exchanging kernel, by the dispatch rule
# (geometry, B, R).  C3 runs <2, 2> (every wave owns a unit), TINY <1, 1> (waves 2 and 3 own none).  B = R: one ladder; 24 rows of
# R = 8: a ragged tile; 32 and 64 rows of R = 16: whole tiles, rows 15 | 16 are a ladder's border.  4100 / 8200 / 16400 rows launch
# 16 / 32 / 64 rows per workgroup (two and four tiles, hence several ladders, per workgroup in the last two); 4100 and 8200 end in a
# ragged tile whose dead rows pair among themselves.  C5 runs <2, 4> (16 and 32 rows per workgroup only), the kernels at the end of the
# register file.
SWAP = [g + (R, R) for g in (C3, TINY) for R in (2, 4, 8, 16)] + [g + bR for g in (C3, TINY) for bR in ((24, 8), (32, 16), (64, 16))] + \
       [C3 + (4100, 4), C3 + (8200, 8), C3 + (16400, 16), TINY + (4100, 4), TINY + (8200, 8), HG.C5 + (32, 16), HG.C5 + (4100, 4)]
NEXT = [C3 + (24, 8), TINY + (32, 16), C3 + (4100, 4)]
UNIFORM = [C3 + (64, 8), TINY + (32, 16)]                   # the in-kernel uniform (`check_in_kernel_uniform`)
# The geometry classes of tests/chain_geometries.py (a ragged half, a half 2 mod 4, halves 31 / 33 with their scalar row access, whole
# tiles of padding, additive coupling): where nz / 2 and the width end inside the 32-column tiles decides which columns of a quad the
# partner's lane holds, which waves own a half-unit without a real column and what the next trajectory's xi masks.  Every entry at 24
# rows of R = 8 (one whole 16-row tile and one with a live and a dead ladder: dead lanes pair among themselves); every R at a ragged
# half and at an empty second half-tile of <2, 2> and of <2, 4>; B = 4: two ladders in a tile of twelve dead rows; (62, 31) as one
# ladder of 16; additive coupling; the two 4100 / 8200-row entries (32 and 64 rows per workgroup: several ladders per workgroup, 4100
# ends in a ragged tile).
SWAP += [g + (24, 8) for g in G.GEOS] + \
        [(66, 33, 2, 1, 32, 16), (66, 33, 2, 1, 4, 2), (10, 40, 2, 1, 32, 16), (12, 100, 2, 1, 20, 4), (62, 31, 2, 1, 16, 16),
         (66, 33, 3, 0, 32, 16)] + [G.LARGE[0] + (4,), G.LARGE[1] + (8,)]
# half 62: a four-column draw straddles the end of the half under xi, mom and kin0 of the exchanged state; an empty half-tile
NEXT += [(124, 63, 3, 1, 24, 8), (10, 40, 2, 1, 32, 16)]
UNIFORM += [(66, 33, 2, 1, 32, 8), (10, 40, 2, 1, 32, 16)]
FORMS = [c[:4] + (24, 8) for c in G.FORMS]                   # the call forms of a swapping end call (`check_swap_forms`)
# Added to `design`'s seed for a case of SWAP, keyed by the case, should the default draws leave it without a swapping and a
# non-swapping pair in some launch or put a pair within `forced`'s margin of a tie.  To be chosen on the CPU from the float64 records
# (their energies and `kept_energy` on the rows either way, accepted or not), never from the device's answer: none needed -- every
# launch of every case above has both kinds of pair, and the nearest pair of any case is 100 margins from a tie (profiles/hmc_exchange_geometries.txt).
DESIGN_SEED = {}
DELTA = 2.0 ** -9
SWAPPED = -(len(TEMPER) + len(METRIC) + 2) - 2               # `swapped` in hmc_tempered_gpu.flat of a swapping call's result


def run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, rows=slice(None), state=None, adapt=None, window=None, propose=True,
        anneal=None, swap=None, ladder=0, swap_uniform=None, e="record", ge="record", point=None, inplace=False, reuse_buffers=False):
    """The recorded call r on its rows from its inputs' casts through the exchanging wrapper: (state after, [next point, accepted,
    log_alpha, swapped, log_swap]).  e / ge / point: the record's energy_g / grad_g / point, or another (the rows' own, already
    cut; None for e and ge: the NULL form)."""
    F, dev = lsnf.flow, s.dev
    cut = lambda t: None if t is None else t[rows].float().to(dev).contiguous()
    state = sp.T.state_for(lsnf, s, r, rows) if state is None else state
    kw = dict(phase=r.phase, uniform=uniform, propose=propose, adapt=adapt, window=window, anneal=anneal, swap=swap, ladder=ladder,
              swap_uniform=swap_uniform, inplace=inplace, reuse_buffers=reuse_buffers)
    point = cut(sp.point(r)) if point is None else point
    e = cut(r.e) if isinstance(e, str) else e
    ge = cut(r.ge) if isinstance(ge, str) else ge
    if sp.name == "z":
        out = F.hmc_step_exchange(s.plan, point, ge, e, state, noise, steps, metric, temper, **kw)
        out = out[:3] + out[4:]
    else:
        saved, act = sp.T.stash_at(lsnf, s.plan, point)
        out = F.reverse_hmc_step_exchange(s.plan, point, saved, act, ge, e, state, noise, steps, metric, temper, **kw)
    return state, list(out)


# ---- 1 ----
def check_no_swap_is_the_tempered_call(lsnf, sp, s):
    c, dev, B = s.c, s.dev, s.c.B
    beta = TG.beta_rows(B).to(dev)
    bn = TG.next_beta(beta)
    for r, propose in MG.forms_of(sp, c):
        end = r.phase == "end"
        kept = sp.T.state_for(lsnf, s, r).z if end else None
        variants = [(None, None, None)]
        variants += [("update", "close", bn), (None, "fold", None)] if end else [(None, None, bn)] if r.phase == "init" else []
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
                assert out[3] is None and out[4] is None     # nothing is written without the swap: there is nothing to write to
                got = TG.flat((state, out[:3]), steps, metric, temper)
                name = f"{sp.name} {c.geo} B{B} {r.phase} propose={propose} {how} adapt={adapt} window={window} anneal={anneal is not None}"
                assert len(got) == len(ref)
                for k, (a, b) in enumerate(zip(got, ref)):
                    assert bits(a, b), f"{name}: output {k} differs"


# ---- 2 and 4 ----
def kept_energy(e32):
    """The kept like_energy of the swap tests: the record's energy + 2^-9 (1 + row % 3) -- recognisable, and near enough for the sign of
    a pair's e to be known beforehand (module docstring)."""
    rows = torch.arange(e32.shape[0], device=e32.device)
    return e32 + DELTA * (1.0 + (rows % 3).float())


def design(B, R, parity, e32, first_swaps, seed=0):
    """(beta (B) fp32, want (B) bool, prt): U(0.2, 1.5) temperatures per row; pair k is meant to swap iff (k even) == first_swaps; a
    pair meant to reject gets its two temperatures 0.2 .. 1.0 apart and ordered so that log_r < 0 for the records' energies e32."""
    g = torch.Generator().manual_seed(7000 + seed)
    beta = (0.2 + 1.3 * torch.rand(B, generator=g)).float()
    gap = (0.2 + 0.8 * torch.rand(B, generator=g)).float()
    prt = X.partner(B, R, parity)
    want = torch.zeros(B, dtype=torch.bool)
    e = e32.cpu()
    k = 0
    for a in range(B):
        b = int(prt[a])
        if b <= a:
            continue
        w = (k % 2 == 0) == first_swaps
        k += 1
        want[a] = want[b] = w
        if not w:
            lo = beta[a].item()
            hi = float(np.float32(lo + gap[a].item()))
            beta[a], beta[b] = (lo, hi) if e[a] > e[b] else (hi, lo)      # d = beta_a - beta_b against e = e_a - e_b
    return beta, want, prt


def forced(lr64, want, prt):
    """(u (B) fp32 -- exp(log_r -+ 1) clipped into (0, 1), the same on both rows of a pair --, the float64 decision with that u, the
    least distance of a pair from a tie relative to 1e-4 (1 + |log_r|)).  A pair meant to reject whose log_r is so near 0 (or above
    it) that the clipped u would leave it within a hundred times that distance of a tie is made to swap instead: no pair is left out."""
    lr64 = lr64.cpu()
    top = 1.0 - 2.0 ** -24
    reject = torch.exp(lr64 + 1.0).clamp(max=top).float()
    clear = torch.log(reject.double()) - lr64 > 1e-2 * (1.0 + lr64.abs())
    u = torch.where(want | ~clear, torch.exp(lr64 - 1.0).clamp(2.0 ** -126, top).float(), reject)
    rows = torch.arange(prt.shape[0])
    u = u[torch.minimum(rows, prt)]
    sw = X.decide(lr64, u.double(), prt)
    paired = prt != rows
    tie = ((torch.log(u.double()) - lr64).abs() / (1e-4 * (1.0 + lr64.abs())))[paired]
    return u, sw, (tie.min().item() if tie.numel() else float("inf"))


def check_swap_bits(lsnf, sp, s, R):
    """From the device's own stored state after the same call WITHOUT the swap, the header's fp32 lines hold to the bit; the rows'
    temperatures, steps, scales and accumulators do not move; an idle rung has the plain call's bits."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = sp.end_calls(c)[0]
    e32 = r.e.float()
    sd = MG.column_scale(B, c.nz, 3, spread=1.0)
    for parity in ("even", "odd"):
        prt = X.partner(B, R, parity)
        paired = prt != torch.arange(B)
        seen_swap = seen_stay = False
        for propose in (True, False):
            for first in (True, False):
                name = f"[{sp.name} exchange] {c.geo} B{B} R{R} {parity} propose={propose} first_swaps={first}"
                beta, want, _ = design(B, R, parity, e32, first, seed=R + (parity == "odd") + DESIGN_SEED.get(c.geo + (B, R), 0))
                beta = beta.to(dev)
                noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, propose)

                def call(**kw):
                    steps, metric = MG.same_steps(lsnf, sp, c, B, dev, 7), MG.new_metric(lsnf, s, B, sd)
                    temper = TG.new_temper(lsnf, s, B, beta, "old")
                    temper.like_energy.copy_(kept_energy(e32.to(dev)))
                    before = (steps.step.clone(), steps.adapt.clone(), MG.clone_metric(lsnf, metric), TG.clone_temper(lsnf, temper))
                    state, out = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, propose=propose, **kw)
                    return state, out, steps, metric, temper, before
                sa, oa, _, _, ta, _ = call()
                torch.cuda.synchronize()
                # the float64 restatement of the decisions, from the plain call's stored like_energy: BEFORE the swapping launch
                lr64 = X.log_ratio(beta.double().cpu(), ta.like_energy.double().cpu(), prt)
                u, sw64, tie = forced(lr64, want, prt)
                assert tie > 1.0, f"{name}: a pair is near a tie ({tie:.3g} of the margin)"
                print(f"{name}: {int(sw64.sum())} of {int(paired.sum())} paired rows swap, the nearest pair at {tie:.3g} of the margin from a tie")
                seen_swap, seen_stay = seen_swap or bool(sw64.any()), seen_stay or bool((~sw64 & paired).any())
                if paired.sum() > 2:                         # (a launch with one pair cannot hold both kinds: the case does, below)
                    assert bool(sw64.any()) and bool((~sw64 & paired).any()), f"{name}: the launch needs a swapping and a non-swapping pair"
                sb, ob, steps, metric, tb, (step0, adapt0, metric0, temper0) = call(swap=parity, ladder=R, swap_uniform=u.to(dev))
                torch.cuda.synchronize()
                sw = sw64.to(dev)
                # the trajectory's own decision and outputs
                assert bits(ob[1], oa[1]) and bits(ob[2], oa[2]) and bits(sb.kin, sa.kin), f"{name}: accepted / log_alpha / kin0"
                # the move's outputs
                assert bits(ob[3], sw.float()), f"{name}: swapped is not the float64 decision"
                assert bits(ob[4], X.log_ratio(beta, ta.like_energy, prt)), f"{name}: log_swap is not (beta_a - beta_b) * (el_a - el_b)"
                # the exchanged state: the header's lines in fp32 on the plain call's stored arrays
                z, g, uu, gl, el = X.exchange(beta, sa.z, sa.grad, sa.energy, ta.like_grad, ta.like_energy, prt, sw)
                for f, got, ref in (("state.z", sb.z, z), ("state.grad", sb.grad, g), ("state.energy", sb.energy, uu),
                                    ("like_grad", tb.like_grad, gl), ("like_energy", tb.like_energy, el)):
                    assert bits(got, ref), f"{name}: {f} differs from the restated exchange"
                if bool(sw64.any()):
                    assert not bits(sb.z[sw], sa.z[sw]) and not bits(sb.grad[sw], sa.grad[sw])
                # what must not move: the temperatures, the steps, the metric and its accumulators, the weights
                assert bits(tb.beta, temper0.beta) and bits(tb.log_w, temper0.log_w), f"{name}: beta / log_w moved"
                assert bits(steps.step, step0) and bits(steps.adapt, adapt0) and MG.untouched(metric, metric0), f"{name}: steps / metric moved"
                # rows that did not swap -- idle rungs among them -- have the plain call's bits everywhere
                stay = ~sw
                for a, b in zip(HG.flat((sb, ob[:3])), HG.flat((sa, oa[:3]))):
                    assert bits(a[stay], b[stay]), f"{name}: a row that did not swap differs from the plain call"
                assert bool((~sw64[~paired]).all()) and bits(ob[4][(~paired).to(dev)], torch.zeros(int((~paired).sum()), device=dev))
                if not propose:                              # nothing begun: the full-step momentum of the plain call, on every row
                    assert ob[0] is None and bits(sb.mom, sa.mom)
                    continue
                # the next trajectory begins from the EXCHANGED state with the row's own step, scale and xi
                st, sdd = steps.step[:, None], metric.scale
                ph = noise - (0.5 * st) * (sdd * sb.grad)
                assert bits(sb.mom, ph), f"{name}: mom is not xi - (0.5 s) (sd grad_acc')"
                assert bits(ob[0], sb.z + st * (sdd * ph)), f"{name}: the next point is not z_state' + s (sd mom)"
                if bool(sw64.any()):
                    assert not bits(sb.mom[sw], sa.mom[sw])
        if R > 2 or parity == "even":
            assert seen_swap and seen_stay, f"[{sp.name} exchange] {c.geo} B{B} R{R} {parity}: the case needs a swapping and a non-swapping pair"
        else:                                                # R = 2 with odd parity swaps nothing
            assert not paired.any() and not seen_swap


# ---- 3 ----
def check_next_trajectory_follows_float64(lsnf, sp, s, R):
    """z_next / eps_next, state.mom and state.kin after a swapping call against the float64 restatement, under hmc_metric_gpu.gates:
    the exchanged state (float64, and fp32 for the widening) is given to `gates` as the state an init call begins from."""
    c, dev, B, F, T = s.c, s.dev, s.c.B, lsnf.flow, sp.T
    f32, f64 = torch.float32, torch.float64
    r = next(x for x in sp.end_calls(c) if x.noise is not None) if any(x.noise is not None for x in sp.end_calls(c)) else None
    if r is None:                                            # (B > 100: one trajectory, its end call proposes with the init call's noise)
        r = copy.copy(sp.end_calls(c)[0])
        r.noise = c.calls[0].noise
    ones = torch.ones(B, c.nz)
    for parity in ("even", "odd"):
        beta, want, prt = design(B, R, parity, r.e.float(), True, seed=50 + R)
        r2, o = TG.general_gates(sp, c, r, beta)
        o32 = MG.expected(sp, r2, ones, c.s, f32, acc=o.acc)
        steps, metric = F.new_hmc_row_steps(B, dev, c.s), MG.new_metric(lsnf, s, B)
        temper = TG.new_temper(lsnf, s, B, beta, "old")
        kg, ke = temper.like_grad.cpu(), temper.like_energy.cpu()
        point = sp.point(r)
        gl32 = r.ge.to(f32) if sp.name == "z" else RM.pull_back(c.p, point.to(f32), r.ge.to(f32), f32)
        a = o.acc[:, None]
        gls64, els64 = torch.where(a, r2.gl64, kg.double()), torch.where(o.acc, r2.el64, ke.double())
        gls32, els32 = torch.where(a, gl32, kg), torch.where(o.acc, r.e.to(f32), ke)
        us64, us32 = torch.where(o.acc, r2.U_prop, r2.u_acc), torch.where(o.acc, r2.o32.U_prop, r2.u_acc.to(f32))
        lr64 = X.log_ratio(beta.double(), els64, prt)
        u, sw64, tie = forced(lr64, want, prt)
        assert tie > 1.0
        x64, g64 = X.exchange(beta.double(), o.xs, o.gs, us64, gls64, els64, prt, sw64)[:2]
        x32, g32 = X.exchange(beta, o32.xs, o32.gs, us32, gls32, els32, prt, sw64)[:2]
        r3 = copy.copy(r2)
        r3.phase = "init"
        setattr(r3, "z_prop" if sp.name == "z" else "e_prop", x64)
        r3.g = g64
        r3.o32 = types.SimpleNamespace(g=g32, U_prop=torch.zeros(B))
        r3.smooth = r.smooth & r.smooth[prt]
        o3 = MG.gates(sp, T, r3, ones, c.s)
        noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, True)
        state = T.state_for(lsnf, s, r2)                     # (the kept state at beta)
        state, (nxt, acc, la, swapped, log_swap) = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, state=state, propose=True,
                                                       swap=parity, ladder=R, swap_uniform=u.to(dev))
        torch.cuda.synchronize()
        d = o.decided & o.decided[prt] & r3.smooth           # both rows of a pair decided their trajectory as float64 did
        assert torch.equal(acc.cpu()[d] == 1.0, o.acc[d]) and torch.equal(swapped.cpu()[d] == 1.0, sw64[d])
        assert bool((sw64 & d).any()) and bool((~sw64 & d).any())
        name = f"[{sp.name} exchange] {c.geo} B{B} R{R} {parity}"
        e = (state.mom.cpu().double() - o3.mom).norm(dim=1)
        print(f"{name}: {int(sw64.sum())} rows swapped, {int((~d).sum())} set aside; worst |mom - fp64| / bound = {fig((e / o3.mom_bound)[d]):.3f} "
              f"({o3.mom_wide} rows widened by the fp32 restatement)")
        assert bool((e <= o3.mom_bound)[d].all())
        e = T.rel_rows(nxt.cpu(), o3.nxt)
        print(f"{name}: worst next-point rel-L2 / bound = {fig((e / o3.nxt_bound)[d]):.3f} ({o3.nxt_wide} rows widened)")
        assert bool((e <= o3.nxt_bound)[d].all())
        e = (state.kin.cpu().double() - o3.kin).abs()
        print(f"{name}: worst kin0 error / bound = {fig(e / o3.kin_bound):.3f} ({o3.kin_wide} rows widened)")
        assert bool((e <= o3.kin_bound).all())


# ---- 5 ----
def swap_uniform_draws(B, seed, offset=0, row0=0):
    """(B,) np.float32: mala_restated.uniform_draws at field value 3 of the counter instead of 2 -- the number the kernel draws for the
    pair whose lower row is row0 + sample."""
    mask = np.uint64(0xFFFFFFFF)
    rows = np.arange(B, dtype=np.uint64) + np.uint64(row0)
    c3 = np.uint64((offset >> 32) & 0xFFFFFFFF) ^ (rows >> np.uint64(32))
    x0 = philox4x32_10(np.uint64(3 << 16), rows & mask, np.uint64(offset & 0xFFFFFFFF), c3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return ((x0 >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def uniform_problem(B, R):
    """(beta (B), energy_g (B)) of `check_in_kernel_uniform`, fp32: a ladder 0.2 .. 1.4 with a jitter per row; U(0, 60) energies."""
    g = torch.Generator().manual_seed(7100)
    beta = (torch.linspace(0.2, 1.4, R).repeat(B // R) + 0.05 * torch.rand(B, generator=g)).float()
    return beta, (60.0 * torch.rand(B, generator=g)).float()


def check_in_kernel_uniform(lsnf, sp, s, R):
    """With a PhiloxNoise the pair's uniform is Philox at field 3 of the lower row's counter: the call is the tensor form's with the
    restated draws, bit for bit; a ladder alone at row0 = k R gives ladder k of the whole batch; the draw is not the trajectory's.
    The energies are the test's own, U(0, 60) per row with the kept ones beside them (`kept_energy`), so that whatever the
    trajectories decide a ladder's log_r are of order +-3 and the drawn uniforms swap some pairs and not others: `uniform_problem`
    restates that on the CPU."""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = sp.end_calls(c)[0]
    seed, offset = 99, (7 << 32) + 5
    beta, energy = uniform_problem(B, R)
    beta, energy = beta.to(dev), energy.to(dev)
    u_traj, u_swap = MA.uniform_draws(B, seed, offset), swap_uniform_draws(B, seed, offset)
    assert not np.any(u_traj == u_swap)                      # another field of the counter: another stream
    for parity in ("even", "odd"):
        def go(rows, row0, how, propose=True):
            n = len(range(*rows.indices(B)))
            whole, wt = MG.same_steps(lsnf, sp, c, B, dev, 7), TG.new_temper(lsnf, s, B, beta, "old")
            steps, metric = F.HmcRowSteps(whole.step[rows].clone(), whole.adapt[rows].clone()), MG.new_metric(lsnf, s, n)
            temper = F.HmcRowTemper(*(getattr(wt, f)[rows].clone() for f in TEMPER))
            temper.like_energy.copy_(kept_energy(energy)[rows])
            if isinstance(how, str):                         # "philox"; else the swap's uniforms, with the restated trajectory's
                noise, uniform, su = F.PhiloxNoise(seed, offset, row0), None, None
            else:
                noise, uniform, su = None, torch.from_numpy(u_traj)[rows].to(dev), torch.from_numpy(how)[rows].to(dev)
            res = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, rows=rows, propose=propose, swap=parity, ladder=R, swap_uniform=su,
                      e=energy[rows].clone())
            return TG.flat(res, steps, metric, temper)
        whole = go(slice(0, B), 0, "philox")
        swapped = whole[SWAPPED]
        pairs = int((X.partner(B, R, parity) != torch.arange(B)).sum())
        if pairs:
            assert 0 < int(swapped.sum()) < pairs, f"{sp.name} {parity}: the in-kernel draws should swap some pairs and not others"
        for k in range(B // R):                              # a ladder alone, sharded at its first row
            alone = go(slice(k * R, (k + 1) * R), k * R, "philox")
            for a, b in zip(whole, alone):
                assert bits(a[k * R:(k + 1) * R], b), f"{sp.name} {parity}: ladder {k} alone differs from ladder {k} of the batch"
        # nothing proposed: the tensor form needs no noise, and its uniforms are the restated draws of fields 2 and 3
        drawn, given = go(slice(0, B), 0, "philox", propose=False), go(slice(0, B), 0, u_swap, propose=False)
        for a, b in zip(drawn, given):
            assert bits(a, b), f"{sp.name} {parity}: the in-kernel swap uniform is not Philox at field 3 of the lower row"
        if pairs:                                            # (and with the trajectory's uniforms in their place other pairs swap)
            other = go(slice(0, B), 0, u_traj, propose=False)
            assert not bits(other[SWAPPED], drawn[SWAPPED])


# ---- 6 ----
def pt_problem(lsnf, K, dev):
    """(net, netG, x (2, nz)) of tests/hmc_tempered_gpu.py's sampler problem: the affine TINY flow and netG(z) = diag(a) z."""
    net, netG, x, _, _ = TG.ais_problem(lsnf, K, dev)
    return net, netG, x


def check_samplers(lsnf, sp, K, dev, monkeypatch):
    from counting_lib import install
    F, Lv = lsnf.flow, lsnf.langevin
    net, netG, x = pt_problem(lsnf, K, dev)
    fn = Lv.sample_hmc_pt_post_z_with_flow if sp.name == "z" else Lv.sample_hmc_pt_post_eps_with_flow
    N, R, Ks, L, nz, step = x.shape[0], 4, 6, 2, x.shape[1], 0.28
    B, plan = N * R, net._plan()
    betas = Lv.pt_ladder(R, 0.05)
    start = torch.randn(N, nz, generator=torch.Generator().manual_seed(11)).to(dev)
    kw = dict(betas=betas, g_l_steps=Ks, leapfrog_steps=L, g_l_step_size=step, g_llhd_sigma=1.0)
    ph = F.PhiloxNoise(7, 3, 0)
    stand = install(monkeypatch, lsnf)
    first, rate, swap_rate, U, state, temper = fn(start, x, netG, net, philox=ph, **kw)
    torch.cuda.synchronize()
    entered = dict(stand.entered)
    monkeypatch.undo()
    # launches on the flow's side: one exchanging call per leapfrog step, and the step's forward (z) or reverse (eps) in front of it
    calls = Ks * L + 1
    mine = "lsnf_hmc_step_exchange" if sp.name == "z" else "lsnf_reverse_hmc_step_exchange"
    launching = {n: k for n, k in entered.items() if n in stand.launching()}
    if sp.name == "z":
        want = {"lsnf_forward": calls, mine: calls}
    elif F.reverse_keep_supported(plan, B):
        want = {"lsnf_reverse_keep": calls, "lsnf_reverse": 1, mine: calls}      # (the last reverse: z_k of the cold rung)
    else:
        want = {"lsnf_reverse": calls + 1, "lsnf_forward": calls, mine: calls}
    assert launching == want, launching
    assert ph.offset == 3 + Ks + 1 and first.shape == (N, nz, 1, 1) and rate.shape == (B,) and swap_rate.shape == (N, R - 1) and U.shape == (B,)
    assert bits(temper.beta, betas.float().repeat(N).to(dev))
    # by hand: the same sequence of flow calls; every end call swaps, even / odd alternating
    ph = F.PhiloxNoise(7, 3, 0)
    xs = x.repeat_interleave(R, dim=0)
    point = start.repeat_interleave(R, dim=0).contiguous().clone()
    steps, metric = F.new_hmc_row_steps(B, dev, step), F.new_hmc_row_metric(plan, B, dev)
    mine_t = F.new_hmc_row_temper(plan, B, dev, betas.float().repeat(N))
    st, act = F.new_hmc_state(plan, B, dev), F.new_act_saved(plan, B, dev)
    flags, sums, tried = [], {"even": torch.zeros(B, device=dev), "odd": torch.zeros(B, device=dev)}, {"even": 0, "odd": 0}
    for j in range(calls):
        t, inner = j // L, j % L != 0
        phase = "inner" if inner else "end" if j else "init"
        parity = None if inner or not j else ("even", "odd")[(t - 1) % 2]
        noise = None if inner else ph.step(t)
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
                out = net.hmc_step_exchange(point, gg, e.detach(), st, noise, steps, metric, mine_t, phase=phase, propose=j < calls - 1,
                                            inplace=True, swap=parity, ladder=R)
                acc, swapped = out[1], out[4]
            else:
                out = net.reverse_hmc_step_exchange(point, saved, act, gg, e.detach(), st, noise, steps, metric, mine_t, phase=phase,
                                                    propose=j < calls - 1, inplace=True, swap=parity, ladder=R)
                acc, swapped = out[1], out[3]
        if parity:
            flags.append(acc.clone()); sums[parity] += swapped; tried[parity] += 1
    for f in FIELDS:
        assert bits(getattr(state, f), getattr(st, f)), f
    for f in TEMPER:
        assert bits(getattr(temper, f), getattr(mine_t, f)), f
    top = st.z.view(N, R, nz)[:, R - 1].contiguous()
    assert bits(first.view(N, nz), top if sp.name == "z" else F.reverse(plan, top, None)[0])
    assert bits(rate, torch.stack(flags).sum(0) / Ks) and bits(U, st.energy)
    # swap_rate is the mean of `swapped` per adjacent pair over the calls that tried it, read at the pair's lower row
    want = torch.stack([sums[("even", "odd")[p % 2]].view(N, R)[:, p] / tried[("even", "odd")[p % 2]] for p in range(R - 1)], dim=1)
    assert tried == {"even": 3, "odd": 3} and bits(swap_rate, want)
    print(f"[{sp.name} exchange] sampler N={N} R={R} K={Ks} L={L}: mean acceptance {rate.mean().item():.2f}, swap rates "
          + " ".join(f"{v:.2f}" for v in swap_rate.mean(0).tolist()))
    assert swap_rate.max().item() > 0.0 and rate.max().item() > 0.0      # some pair swapped, some trajectory was accepted
    # swap_every = 2: end calls 2, 4, 6 swap, even / odd / even
    ph = F.PhiloxNoise(7, 3, 0)
    sparse = fn(start, x, netG, net, philox=ph, swap_every=2, **kw)
    assert not bits(sparse[4].z, state.z) and sparse[2].shape == (N, R - 1)
    # nothing to do
    ph = F.PhiloxNoise(7, 3, 0)
    none = fn(start, x, netG, net, philox=ph, **dict(kw, g_l_steps=0))
    assert bits(none[0].view(N, nz), start) and none[1:] == (None,) * 5 and ph.offset == 3


# ---- 8 ----
def check_swap_forms(lsnf, sp, s, R):
    """The call forms of an end call with swap="odd" that proposes, each against the plain form of the same swapping call bit for
    bit (hmc_tempered_gpu.flat plus swapped and log_swap): in place; every tensor 4 bytes off a 16-byte boundary -- swap_uniform, the
    state, steps, metric and temper tensors among them, log_w 8 bytes off: it stays 8-byte aligned; the stash stays 16-byte aligned --,
    which is where the scalar row access meets the lane exchange whatever the half; grad_g = energy_g = None against zeros with a
    PhiloxNoise (the kept like_energy zero as well: log_r is +-0 and EVERY pair swaps, asserted); reuse_buffers=True, two consecutive
    calls against two calls with fresh buffers.  The uniforms are forced as `check_swap_bits` forces them, so the plain form has a
    swapping and a non-swapping pair.  (The wrapper always allocates swapped / log_swap: the NULL form of those two arguments of the
    C call is not reachable from here and is not covered.)"""
    c, dev, B, F = s.c, s.dev, s.c.B, lsnf.flow
    r = sp.end_calls(c)[0]
    parity, name = "odd", f"[{sp.name} exchange] {c.geo} B{B} R{R} odd forms"
    e32 = r.e.float()
    sd = MG.column_scale(B, c.nz, 5, spread=1.0)
    prt = X.partner(B, R, parity)
    paired = prt != torch.arange(B)
    beta, want, _ = design(B, R, parity, e32, True, seed=90 + R)
    beta = beta.to(dev)
    noise, uniform = HG.draws(lsnf, sp, c, r, "tensors", dev, True)
    swap = dict(swap=parity, ladder=R)

    def fresh(kept=None):
        steps, metric = MG.same_steps(lsnf, sp, c, B, dev, 7), MG.new_metric(lsnf, s, B, sd)
        temper = TG.new_temper(lsnf, s, B, beta, "old")
        temper.like_energy.copy_(kept_energy(e32.to(dev)) if kept is None else kept)
        return steps, metric, temper

    def whole(res, steps, metric, temper):
        state, out = res
        return TG.flat((state, out[:3]), steps, metric, temper) + [out[3], out[4]]

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
    # the uniforms, from the float64 log_r of the call without the swap
    steps, metric, temper = fresh()
    run(lsnf, sp, s, r, steps, metric, temper, noise, uniform)
    torch.cuda.synchronize()
    u, sw64, tie = forced(X.log_ratio(beta.double().cpu(), temper.like_energy.double().cpu(), prt), want, prt)
    assert tie > 1.0 and bool(sw64.any()) and bool((~sw64 & paired).any()), f"{name}: the call needs a swapping and a non-swapping pair"
    u = u.to(dev)
    steps, metric, temper = fresh()
    ref = whole(run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, swap_uniform=u, **swap), steps, metric, temper)
    assert bits(ref[-2], sw64.float().to(dev)), f"{name}: swapped is not the float64 decision"
    # in place: the next point over the point
    steps, metric, temper = fresh()
    point = sp.point(r).float().to(dev).contiguous()
    res = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, point=point, inplace=True, swap_uniform=u, **swap)
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
              inplace=True, swap_uniform=off(u), **swap)
    same(whole(res, steps, metric, temper), ref, "4 bytes off")
    # NULL gradient and energy are zeros; with the kept like_energy zero too every el_s is 0, log_r = +-0 and every pair swaps
    rng, both = F.PhiloxNoise(8, 9, 0), []
    for gg, e in ((None, None), (torch.zeros(B, c.nz, device=dev), torch.zeros(B, device=dev))):
        steps, metric, temper = fresh(torch.zeros(B, device=dev))
        both.append(whole(run(lsnf, sp, s, r, steps, metric, temper, rng, None, ge=gg, e=e, **swap), steps, metric, temper))
    same(both[0], both[1], "NULL grad_g / energy_g")
    swapped, log_swap = both[0][-2].cpu(), both[0][-1].cpu()
    assert bool((swapped[paired] == 1.0).all()) and bool((swapped[~paired] == 0.0).all()) and bool((log_swap == 0.0).all()), \
        f"{name}: with a null likelihood every pair swaps"
    # reuse_buffers: two consecutive calls (the second from the first one's state) against the same two with fresh buffers
    def twice(reuse):
        steps, metric, temper = fresh()
        state, outs, ptrs = sp.T.state_for(lsnf, s, r), [], []
        for _ in range(2):
            res = run(lsnf, sp, s, r, steps, metric, temper, noise, uniform, state=state, swap_uniform=u, reuse_buffers=reuse, **swap)
            outs.append([t.clone() for t in whole(res, steps, metric, temper)])
            ptrs.append(res[1][3].data_ptr())
        return outs, ptrs
    (a1, a2), kept_ptrs = twice(True)
    (b1, b2), _ = twice(False)
    assert kept_ptrs[0] == kept_ptrs[1]                      # (swapped lives on the plan: the second call wrote over the first one's)
    same(a1, ref, "reuse_buffers, first call"); same(b1, ref, "fresh buffers, first call")
    same(a2, b2, "reuse_buffers, second call")
    assert not all(bits(x, y) for x, y in zip(a2, a1))       # (the second call is another computation: it starts from the first one's state)

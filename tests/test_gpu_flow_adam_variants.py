"""GPU: the variants of the fused optimizer step (lsnf_adam_step_ex, flow.adam_step's options, FlowAdam / FlowAdamW) -- amsgrad,
maximize, decoupled weight decay, the non-finite skip and the on-device weight average -- against the float64 restatement
(tests/adam_variants_restated.py, held to torch.optim.Adam / AdamW on the CPU by tests/test_flow_adam_variants_cpu.py).

Allowance for p / m / v / vmax, per tensor, as in test_gpu_flow_adam.py: max(3 x the deviation of the matching torch optimizer
-- on the GPU, fp32, foreach=False, with clip_grad_norm_ -- from that same float64 result, 2^-23 x max|value|).  The code under
test sets no tolerance.  That rule is applied to that file's own cases (its seeded parameters, gradients and betas): their
gradient scales rise, so every stored value grows and the roundings of earlier steps stay below an ulp of the final value,
which is what the rule's floor assumes.  There amsgrad's maximum IS v, so a second set of cases -- gradient scales that FALL
after the second step (0.02 x (1, 3, 0.1, 0.1, 0.1)) with beta2 = 0.9 -- makes the maximum bite; with falling values a stored
v carries roundings made when it was larger, so those cases hold vmax (frozen when it was largest) to the rule and p to
k x 2^-24 x max|p| after k steps: one fp32 rounding of p per step, the update's own error (a relative 2^-23 of stored m, v,
vmax times an update of about lr) being 1e-4 of that.  The average: k x 2^-24 x max|average| per tensor after k steps against
the float64 average of the parameters the device stored (one fp32 rounding per step, earlier errors shrink by the decay).
Geometries: those of test_gpu_flow_adam.py (one short chunk; many chunks with a ragged last one and tensors off the 16-byte
boundary inside the state arrays; all 192 table entries; additive coupling; the reference geometry once)."""
import ctypes
import functools
import math

import pytest
import torch

from adam_variants_restated import clip_adam_variants, ema_of
from oracle import flow_oracle as O
from test_gpu_flow_adam import BETAS as RISING_BETAS, GEOS, assert_within_allowance, case as rising_case, make_net, oracle_params, shapes_of

pytestmark = pytest.mark.gpu

BETAS, LR, EPS, WD = (0.5, 0.9), 1e-3, 1e-8, 1e-2
SCALES = (1.0, 3.0, 0.1, 0.1, 0.1)
# name -> (options of the step, weight decay, clip)
VARIANTS = {
    "amsgrad": (dict(amsgrad=True), 0.0, None),
    "maximize": (dict(maximize=True), WD, None),
    "decoupled": (dict(decoupled=True), WD, None),
    "ema": (dict(ema_decay=0.9), 0.0, None),
    "decoupled-ema": (dict(decoupled=True, ema_decay=0.9), WD, None),       # lsnf_adam_kernel<false, true, true>: FlowAdamW's average without amsgrad
    "skip": (dict(skip_nonfinite=True), 0.0, None),
    "amsgrad-decoupled-maximize-clip": (dict(amsgrad=True, decoupled=True, maximize=True), WD, "below"),
}
CASES = [(g, v, s) for g in ("tiny", "odd", "max-depth", "additive") for v in VARIANTS for s in (1, 5)] + \
        [("reference", "amsgrad-decoupled-maximize-clip", 5)]


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


@functools.lru_cache(maxsize=None)
def case(geo_name):
    """The falling cases: seeded fp32 parameters and five lists of fp32 gradients (CPU), and the float64 global norm of every
    step.  (The rising ones are test_gpu_flow_adam.py's `case`.)"""
    gen = torch.Generator().manual_seed(sum(map(ord, geo_name)))
    shapes = shapes_of(GEOS[geo_name])
    params = [torch.randn(*s, generator=gen) * 0.1 for s in shapes]
    grads = [[torch.randn(*s, generator=gen) * (0.02 * SCALES[k]) for s in shapes] for k in range(5)]
    norms = [float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs))) for gs in grads]
    return params, grads, norms


def max_norm_of(clip, norms):
    return None if clip is None else 0.5 * min(norms)


@functools.lru_cache(maxsize=None)
def references(geo_name, variant, steps, rising=True):
    """(float64 restatement, the matching torch optimizer on the GPU in fp32 as (p, m, v, vmax | None)), computed once.
    rising: test_gpu_flow_adam.py's cases and betas, else the falling ones of this file."""
    params, grads, norms = (rising_case if rising else case)(geo_name)
    betas = RISING_BETAS if rising else BETAS
    opts, wd, clip = VARIANTS[variant]
    mn = max_norm_of(clip, norms[:steps])
    r64 = clip_adam_variants(params, grads[:steps], lr=LR, betas=betas, eps=EPS, weight_decay=wd, max_norm=mn, **opts)
    dev = torch.device("cuda:0")
    live = [torch.nn.Parameter(p.to(dev)) for p in params]
    cls = torch.optim.AdamW if opts.get("decoupled") else torch.optim.Adam
    amsgrad = bool(opts.get("amsgrad"))
    opt = cls(live, lr=LR, betas=betas, eps=EPS, weight_decay=wd, foreach=False, amsgrad=amsgrad, maximize=bool(opts.get("maximize")))
    for gs in grads[:steps]:
        for p, g in zip(live, gs):
            p.grad = g.to(dev)
        if mn is not None:
            torch.nn.utils.clip_grad_norm_(live, mn, foreach=False)
        opt.step()
    t32 = ([p.detach().cpu() for p in live], [opt.state[p]["exp_avg"].cpu() for p in live],
           [opt.state[p]["exp_avg_sq"].cpu() for p in live],
           [opt.state[p]["max_exp_avg_sq"].cpu() for p in live] if amsgrad else None)
    return r64, t32, mn


def run_fused(lsnf, geo_name, grad_steps, dev, *, wd=0.0, mn=None, offset=0, snapshots=False, amsgrad=False, maximize=False,
              decoupled=False, ema_decay=None, skip_nonfinite=False, rising=False):
    """One flow.adam_step per entry of grad_steps on a fresh state; returns a dict of p, m, v, vmax, ema (device views), norms,
    step, skipped and, with snapshots, the parameters before the first step and after each (CPU copies).  offset: every
    parameter and gradient is a view `offset` floats into a 16-byte aligned buffer.  rising: start from the parameters of
    test_gpu_flow_adam.py's case, with its betas."""
    geo = GEOS[geo_name]
    F = lsnf.flow

    def put(t):
        buf = torch.zeros(t.numel() + 4 + offset, device=dev)
        assert buf.data_ptr() % 16 == 0
        v = buf[offset: offset + t.numel()].view(t.shape)
        v.copy_(t)
        return v

    p = [put(t) for t in (rising_case if rising else case)(geo_name)[0]]
    betas = RISING_BETAS if rising else BETAS
    ema = ema_decay is not None
    state = F.new_adam_state(*geo, dev, amsgrad=amsgrad, ema=ema)
    snaps, norms = [[t.cpu() for t in p]] if snapshots else None, []
    for gs in grad_steps:
        g = [None if t is None else put(t) for t in gs]
        n = F.adam_step(p, g, state, *geo, lr=LR, betas=betas, eps=EPS, weight_decay=wd, max_norm=mn, amsgrad=amsgrad,
                        maximize=maximize, decoupled_weight_decay=decoupled, ema_decay=ema_decay, skip_nonfinite=skip_nonfinite)
        norms.append(None if n is None else n.clone())
        if snapshots:
            snaps.append([t.cpu() for t in p])
    steps_view, _, m, v = F.adam_state_views(state, *geo)
    vmax, avg, skipped = F.adam_state_extra_views(state, *geo, amsgrad, ema)
    return dict(p=p, m=m, v=v, vmax=vmax, ema=avg, norms=norms, step=steps_view[0].item(), skipped=skipped.item(), snaps=snaps,
                state=state)


def same_bits(a, b, keys=("p", "m", "v", "vmax", "ema")):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k


# ---- 1. p / m / v / vmax against float64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo_name,variant,steps", CASES)
def test_matches_float64_within_the_matching_torch_optimizers_error(lsnf, gpu_device, geo_name, variant, steps):
    r64, t32, mn = references(geo_name, variant, steps)
    opts, wd, _ = VARIANTS[variant]
    got = run_fused(lsnf, geo_name, rising_case(geo_name)[1][:steps], gpu_device, wd=wd, mn=mn, rising=True,
                    snapshots="ema_decay" in opts, **opts)
    assert got["step"] == steps and got["skipped"] == 0
    if "ema_decay" in opts:                                   # the average of the parameters as stored: section 3's allowance
        for i, (e, r) in enumerate(zip(got["ema"], ema_of(got["snaps"], opts["ema_decay"]))):
            err, allow = (e.double().cpu() - r).abs().max().item(), steps * 2.0 ** -24 * r.abs().max().item()
            assert err <= allow, f"average[{i}]: error {err:.3e} > allowance {allow:.3e}"
    for key, t in zip(("p", "m", "v", "vmax"), t32):
        assert (got[key] is None) == (t is None)
        if t is not None:
            assert_within_allowance(got[key], r64[key], t, key)
    if mn is not None or opts.get("skip_nonfinite"):          # float64 accumulation, one rounding to fp32
        for n, r in zip(got["norms"], r64["norms"]):
            assert abs(n.item() - r) <= 2.0 ** -22 * r
    else:
        assert all(n is None for n in got["norms"])


# ---- 2. amsgrad must bite --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo_name", ["tiny", "odd", "max-depth", "additive"])
def test_amsgrads_maximum_is_above_v_and_changes_the_parameters(lsnf, gpu_device, geo_name):
    r64, t32, _ = references(geo_name, "amsgrad", 5, rising=False)
    above = sum((a > b).sum().item() for a, b in zip(r64["vmax"], r64["v"]))
    assert above >= 0.5 * sum(a.numel() for a in r64["v"])          # a condition of the test: a missing max cannot hide
    got = run_fused(lsnf, geo_name, case(geo_name)[1], gpu_device, amsgrad=True)
    assert_within_allowance(got["vmax"], r64["vmax"], t32[3], "vmax")
    for i, (a, r) in enumerate(zip(got["p"], r64["p"])):             # one fp32 rounding of p per step
        err, allow = (a.double().cpu() - r).abs().max().item(), 5 * 2.0 ** -24 * r.abs().max().item()
        assert err <= allow, f"p[{i}]: error {err:.3e} > allowance {allow:.3e}"
    plain = run_fused(lsnf, geo_name, case(geo_name)[1], gpu_device)
    assert all(bool((a >= b).all()) for a, b in zip(got["vmax"], got["v"]))
    assert sum((a > b).sum().item() for a, b in zip(got["vmax"], got["v"])) >= 0.5 * sum(a.numel() for a in got["v"])
    assert all(torch.equal(a, b) for a, b in zip(got["m"], plain["m"]))          # m does not see the option ...
    assert not all(torch.equal(a, b) for a, b in zip(got["p"], plain["p"]))      # ... the parameters do


# ---- 3. the weight average --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 5])
@pytest.mark.parametrize("geo_name", ["tiny", "odd", "max-depth", "additive"])
def test_average_is_the_float64_average_of_the_stored_parameters(lsnf, gpu_device, geo_name, steps):
    decay = 0.9
    _, grads, _ = case(geo_name)
    frozen = {1, 5, 11}                                           # tensors without a gradient in every step
    gs = [[None if i in frozen else g for i, g in enumerate(step)] for step in grads[:steps]]
    got = run_fused(lsnf, geo_name, gs, gpu_device, wd=WD, ema_decay=decay, amsgrad=True, snapshots=True)
    avg64 = ema_of(got["snaps"], decay)
    for i, (e, r) in enumerate(zip(got["ema"], avg64)):
        err = (e.double().cpu() - r).abs().max().item()
        allow = steps * 2.0 ** -24 * r.abs().max().item()
        assert err <= allow, f"average[{i}]: error {err:.3e} > allowance {allow:.3e}"
    params = case(geo_name)[0]
    for i in frozen:
        assert torch.equal(got["ema"][i].cpu(), params[i]) and torch.equal(got["p"][i].cpu(), params[i])
        assert not got["m"][i].any() and not got["v"][i].any() and not got["vmax"][i].any()
    # the option leaves p, m, v and vmax alone
    without = run_fused(lsnf, geo_name, gs, gpu_device, wd=WD, amsgrad=True)
    same_bits(got, without, keys=("p", "m", "v", "vmax"))


def test_module_loaded_from_ema_state_dict_evaluates_the_average(lsnf, gpu_device):
    nz, w, d, B, decay = 8, 4, 5, 33, 0.8
    net = make_net(lsnf, nz, w, d, gpu_device)
    opt = lsnf.FlowAdamW(net, lr=3e-3, betas=BETAS, ema_decay=decay, amsgrad=True)
    z = torch.randn(B, nz, generator=torch.Generator().manual_seed(9))
    zd = z.to(gpu_device)
    snaps = [[p.detach().cpu().clone() for p in net._param_list()]]
    for _ in range(4):
        net.mle_step(zd, opt)                                     # every variant goes through mle_step unchanged
        snaps.append([p.detach().cpu().clone() for p in net._param_list()])
    avg64 = ema_of(snaps, decay)
    for e, r in zip(opt.ema_parameters(), avg64):
        assert (e.double().cpu() - r).abs().max().item() <= 4 * 2.0 ** -24 * r.abs().max().item()
    sd = opt.ema_state_dict()
    assert list(sd) == list(net.state_dict())
    from_dict, from_avg, by_copy = (make_net(lsnf, nz, w, d, gpu_device, seed=5) for _ in range(3))
    from_dict.load_state_dict(sd)
    with torch.no_grad():
        for q, r in zip(from_avg._param_list(), avg64):
            q.copy_(r.to(torch.float32))
    by_copy.log_prob(zd)                                          # a plan of the old weights is cached: the copy must refresh it
    opt.copy_ema_to(by_copy)
    ll_avg = from_avg.log_prob(zd)[2].double().cpu()
    ll_ref = O.flow_log_prob({k: v.double() for k, v in oracle_params(from_avg).items()}, z.double())[2]
    assert ((ll_avg - ll_ref).abs() / ll_ref.abs()).max().item() <= 1e-5
    for other in (from_dict, by_copy):
        ll = other.log_prob(zd)[2].double().cpu()
        assert ((ll - ll_avg).abs() / ll_avg.abs()).max().item() <= 1e-5
    assert all(torch.equal(a, b) for a, b in zip(from_dict._param_list(), by_copy._param_list()))
    ll_live = net.log_prob(zd)[2].double().cpu()                  # the average is not the live weights
    assert ((ll_live - ll_avg).abs() / ll_avg.abs()).max().item() > 1e-4


# ---- 4. skip -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, "below"])
@pytest.mark.parametrize("poison", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("geo_name", ["tiny", "odd", "max-depth"])
def test_a_non_finite_step_is_skipped_whole(lsnf, gpu_device, geo_name, poison, clip):
    _, grads, norms = case(geo_name)
    bad = [g.clone() for g in grads[1]]
    bad[len(bad) // 2].view(-1)[-1] = poison                     # one element, in the last chunk of a tensor in the middle
    mn = max_norm_of(clip, [norms[0], norms[2]])
    kw = dict(wd=WD, mn=mn, amsgrad=True, decoupled=True, ema_decay=0.9)
    three = run_fused(lsnf, geo_name, [grads[0], bad, grads[2]], gpu_device, skip_nonfinite=True, **kw)
    two = run_fused(lsnf, geo_name, [grads[0], grads[2]], gpu_device, **kw)
    same_bits(three, two)
    assert three["step"] == 2 and three["skipped"] == 1 and two["step"] == 2 and two["skipped"] == 0
    steps_view = lsnf.flow.adam_state_views(three["state"], *GEOS[geo_name])[0]
    grid = int((steps_view != 0).sum().item())
    assert grid >= 1 and bool((steps_view[:grid] == 2).all())     # every workgroup reached the same verdict
    assert not math.isfinite(three["norms"][1].item())
    assert abs(three["norms"][2].item() - norms[2]) <= 2.0 ** -22 * norms[2]
    for p in three["p"]:
        assert bool(torch.isfinite(p).all())


def test_without_the_flag_the_same_gradients_poison_the_step(lsnf, gpu_device):
    _, grads, _ = case("tiny")
    bad = [g.clone() for g in grads[1]]
    bad[2].view(-1)[0] = float("inf")
    got = run_fused(lsnf, "tiny", [grads[0], bad], gpu_device, amsgrad=True)
    assert got["step"] == 2 and got["skipped"] == 0 and not bool(torch.isfinite(got["p"][2]).all())


# ---- 5. bits ---------------------------------------------------------------------------------------------------------------------
ALL = dict(wd=WD, amsgrad=True, decoupled=True, maximize=True, ema_decay=0.9, skip_nonfinite=True)


@pytest.mark.parametrize("geo_name", ["odd", "max-depth"])
def test_two_fresh_runs_are_bit_identical(lsnf, gpu_device, geo_name):
    _, grads, norms = case(geo_name)
    runs = [run_fused(lsnf, geo_name, grads, gpu_device, mn=0.5 * min(norms), **ALL) for _ in range(2)]
    same_bits(*runs)
    assert all(torch.equal(x, y) for x, y in zip(runs[0]["norms"], runs[1]["norms"]))


@pytest.mark.parametrize("geo_name", ["tiny", "odd", "max-depth"])
def test_views_off_the_16_byte_boundary_give_the_aligned_bits(lsnf, gpu_device, geo_name):
    _, grads, norms = case(geo_name)
    a = run_fused(lsnf, geo_name, grads[:3], gpu_device, mn=0.5 * min(norms), **ALL)
    b = run_fused(lsnf, geo_name, grads[:3], gpu_device, mn=0.5 * min(norms), offset=1, **ALL)
    assert b["p"][0].data_ptr() % 16 == 4
    same_bits(a, b)
    assert all(torch.equal(s, t) for s, t in zip(a["norms"], b["norms"]))


@pytest.mark.parametrize("geo_name", ["tiny", "odd", "additive"])
def test_ex_with_no_flag_is_lsnf_adam_step(lsnf, gpu_device, geo_name):
    geo, lib = GEOS[geo_name], lsnf.load_library()
    params, grads, norms = case(geo_name)
    n = len(params)
    assert lib.lsnf_adam_state_bytes_ex(*geo, 0) == lib.lsnf_adam_state_bytes(*geo)
    Options = lsnf._lib.LsnfAdamOptions
    results = []
    for ex in (False, True):
        p = [t.to(gpu_device) for t in params]
        state = torch.zeros(lib.lsnf_adam_state_bytes(*geo) // 4, device=gpu_device)
        out = torch.zeros(1, device=gpu_device)
        ptab = (ctypes.c_void_p * n)(*[t.data_ptr() for t in p])
        for k in range(3):
            g = [t.to(gpu_device) for t in grads[k]]
            gtab = (ctypes.c_void_p * n)(*[t.data_ptr() for t in g])
            mn = 0.5 * min(norms) if k else 0.0                    # one launch, then two
            stream = torch.cuda.current_stream(gpu_device).cuda_stream
            if ex:
                o = Options(ctypes.sizeof(Options), 0, LR, None, BETAS[0], BETAS[1], EPS, WD, mn, 0.0, out.data_ptr() if k else None)
                rc = lib.lsnf_adam_step_ex(ptab, gtab, *geo, state.data_ptr(), ctypes.byref(o), stream)
            else:
                rc = lib.lsnf_adam_step(ptab, gtab, *geo, state.data_ptr(), LR, None, BETAS[0], BETAS[1], EPS, WD, mn,
                                        out.data_ptr() if k else None, stream)
            assert rc == 0, lib.lsnf_last_error()
            torch.cuda.synchronize()
        results.append((p, state, out))
    (p0, s0, o0), (p1, s1, o1) = results
    assert all(torch.equal(a, b) for a, b in zip(p0, p1)) and torch.equal(s0.view(torch.int32), s1.view(torch.int32)) and torch.equal(o0, o1)
    assert lsnf.flow.adam_state_views(s0, *geo)[0][0].item() == 3


# ---- 6. captured step ----------------------------------------------------------------------------------------------------------
def test_captured_step_of_every_variant_replays_eager_bits_and_follows_lr(lsnf, gpu_device):
    nz, w, d = 8, 4, 5
    geo = (nz, w, d, 1)
    gen = torch.Generator().manual_seed(21)
    grads = [[torch.randn(*s, generator=gen) * (0.02 * SCALES[k]) for s in shapes_of(geo)] for k in range(4)]
    grads[1][7].view(-1)[0] = float("inf")                        # the second replay is a skipped step
    norms = [float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs))) for gs in grads]
    hyper = dict(lr=1e-3, betas=BETAS, weight_decay=0.1, max_norm=0.5 * min(norms), capturable=True, amsgrad=True, ema_decay=0.9,
                 skip_nonfinite=True)
    lrs = [1e-3, 1e-3, 1e-3, 4e-4]

    def fresh():
        net = make_net(lsnf, nz, w, d, gpu_device)
        for p in net._param_list():
            p.grad = torch.zeros_like(p)          # static gradient buffers
        return net, lsnf.FlowAdamW(net, **hyper)

    def feed(net, k):
        with torch.no_grad():
            for p, g in zip(net._param_list(), grads[k]):
                p.grad.copy_(g)

    eager_net, eager = fresh()
    for k in range(4):
        feed(eager_net, k)
        eager.param_groups[0]["lr"] = lrs[k]
        eager.step()
    net, opt = fresh()
    weights, blank = [p.detach().clone() for p in net._param_list()], opt.state_dict()
    feed(net, 0)
    opt.step()                                    # warm-up outside the capture, then back to the start
    net._plan()
    with torch.no_grad():
        for p, t in zip(net._param_list(), weights):
            p.copy_(t)
    opt.load_state_dict(blank)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                 # one stream, no parallel branches
        opt.step()
        net._plan()
    for k in range(4):
        feed(net, k)
        opt.param_groups[0]["lr"] = lrs[k]
        opt.sync_lr()                             # a replay runs no Python: the device copy of lr is refreshed here
        graph.replay()
    torch.cuda.synchronize()
    assert opt._steps[0].item() == 3 == eager._steps[0].item() and opt.skipped_steps.item() == 1 == eager.skipped_steps.item()
    mine = list(net._param_list()) + opt._m + opt._v + opt._vmax + opt.ema_parameters()
    theirs = list(eager_net._param_list()) + eager._m + eager._v + eager._vmax + eager.ema_parameters()
    for x, y in zip(mine, theirs):
        assert torch.equal(x.detach(), y.detach())
    # the lr change took effect (in the decoupled decay as well, which reads the device value): with the first rate
    # throughout the parameters would differ
    cpu_w = [t.cpu() for t in weights]
    kw = dict(betas=BETAS, eps=EPS, weight_decay=0.1, max_norm=hyper["max_norm"], amsgrad=True, decoupled=True, skip_nonfinite=True)
    sched = clip_adam_variants(cpu_w, grads, lr=lrs, **kw)
    const = clip_adam_variants(cpu_w, grads, lr=1e-3, **kw)
    assert sched["step"] == 3 and sched["skipped"] == 1
    q = net._param_list()[2].detach().double().cpu()
    assert (q - sched["p"][2]).abs().max().item() < 0.01 * (const["p"][2] - sched["p"][2]).abs().max().item()
    # the replayed plan refresh holds the final values
    z = torch.randn(33, nz, generator=torch.Generator().manual_seed(2))
    plan_ll = lsnf.flow.forward(net._cached_plan, z.to(gpu_device))[2].double().cpu()
    ll_ref = O.flow_log_prob(oracle_params(net), z.double())[2]
    assert ((plan_ll - ll_ref).abs() / ll_ref.abs()).max().item() <= 1e-5


# ---- 7. state dict ---------------------------------------------------------------------------------------------------------------
def set_grads(net, grads, dev):
    for p, g in zip(net._param_list(), grads):
        p.grad = g.to(dev)


@pytest.mark.parametrize("direction", ["fused-to-torch", "torch-to-fused"])
@pytest.mark.parametrize("kind", ["adam-amsgrad", "adamw"])
def test_state_dict_round_trip_with_torch_amsgrad_and_adamw(lsnf, gpu_device, kind, direction):
    nz, w, d = 8, 4, 5
    gen = torch.Generator().manual_seed(23)
    grads = [[torch.randn(*s, generator=gen) * (0.02 * SCALES[k]) for s in shapes_of((nz, w, d, 1))] for k in range(4)]
    src_net, dst_net = make_net(lsnf, nz, w, d, gpu_device), make_net(lsnf, nz, w, d, gpu_device)
    hyper = dict(lr=1e-3, betas=BETAS, weight_decay=WD)
    amsgrad, decoupled = kind == "adam-amsgrad", kind == "adamw"
    fused_first = direction == "fused-to-torch"
    tcls = torch.optim.AdamW if decoupled else torch.optim.Adam
    mk_f = lambda n: (lsnf.FlowAdamW if decoupled else lsnf.FlowAdam)(n, amsgrad=amsgrad, **hyper)
    mk_t = lambda n: tcls(n.parameters(), foreach=False, amsgrad=amsgrad, **hyper)
    src, dst = (mk_f(src_net), mk_t(dst_net)) if fused_first else (mk_t(src_net), mk_f(dst_net))
    start = [p.detach().cpu() for p in src_net._param_list()]
    for k in range(3):
        set_grads(src_net, grads[k], gpu_device)
        src.step()
    sd = src.state_dict()
    assert len(sd["state"]) == 12 * d and len(sd["param_groups"][0]["params"]) == 14 * d      # the dead fc_*.b carry no state
    assert sd["param_groups"][0]["amsgrad"] == amsgrad and sd["param_groups"][0]["decoupled_weight_decay"] == decoupled
    assert all(("max_exp_avg_sq" in st) == amsgrad for st in sd["state"].values())
    dst.load_state_dict(sd)
    dst_net.load_state_dict(src_net.state_dict())
    for net, opt in ((src_net, src), (dst_net, dst)):
        set_grads(net, grads[3], gpu_device)
        opt.step()
    # both sides against float64, with an all-torch run of the same four steps as the fp32 reference leg
    r64 = clip_adam_variants(start, grads, eps=EPS, amsgrad=amsgrad, decoupled=decoupled, **hyper)
    live = [torch.nn.Parameter(p.to(gpu_device)) for p in start]
    leg = tcls(live, foreach=False, amsgrad=amsgrad, **hyper)
    for gs in grads:
        for p, g in zip(live, gs):
            p.grad = g.to(gpu_device)
        leg.step()
    for net in (src_net, dst_net):
        assert_within_allowance([p.detach() for p in net._param_list()], r64["p"], [p.detach().cpu() for p in live], "param")
    f_opt = src if fused_first else dst
    if amsgrad:
        assert_within_allowance(f_opt._vmax, r64["vmax"], [leg.state[p]["max_exp_avg_sq"].cpu() for p in live], "vmax")
    for name, q in dst_net.named_parameters():
        if name.endswith(("fc_1.b", "fc_2.b")):
            assert not q.any()

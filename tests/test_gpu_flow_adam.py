"""GPU: the fused optimizer step of the flow (lsnf_adam_step, flow.adam_step, FlowAdam, netF.mle_step) against the float64
restatement of clip_grad_norm_ + torch.optim.Adam (tests/adam_restated.py).

Allowance, per tensor: max(3 x the deviation of torch.optim.Adam itself -- on the GPU, fp32, foreach=False, with
clip_grad_norm_ -- from that same float64 result, 2^-23 x max|value|).  The floor is one ulp of the largest entry: any fp32
store is off by up to half of it, and torch's own deviation can be exactly zero on a tiny tensor.  The code under test sets no
tolerance.  Gradients are seeded tensors, so most tests need no flow kernel."""
import functools
import types

import pytest
import torch

from adam_restated import clip_adam
from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu

BETAS, LR, EPS = (0.5, 0.999), 1e-3, 1e-8
GEOS = {"tiny": (2, 1, 1, 1), "odd": (126, 127, 2, 1), "reference": (128, 64, 5, 1), "max-depth": (8, 4, 16, 1),
        "additive": (20, 10, 3, 0)}
CONFIGS = {"plain": (0.0, None), "decay": (1e-2, None), "clip-below": (0.0, "below"), "decay-clip-above": (1e-2, "above")}


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


def shapes_of(geo):
    import lsnf_amd
    nz, w, d, c = geo
    return lsnf_amd.flow._param_shapes(nz, w, c) * d


@functools.lru_cache(maxsize=None)
def case(geo_name, steps=5):
    """Seeded fp32 parameters and `steps` lists of fp32 gradients (CPU), and the float64 global norm of every step."""
    gen = torch.Generator().manual_seed(sum(map(ord, geo_name)))
    shapes = shapes_of(GEOS[geo_name])
    params = [torch.randn(*s, generator=gen) * 0.1 for s in shapes]
    grads = [[torch.randn(*s, generator=gen) * (0.02 * (k + 1)) for s in shapes] for k in range(steps)]
    norms = [float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs))) for gs in grads]
    return params, grads, norms


def max_norm_of(clip, norms):
    return None if clip is None else (0.5 * min(norms) if clip == "below" else 2.0 * max(norms))


@functools.lru_cache(maxsize=None)
def references(geo_name, cfg_name, steps):
    """(float64 restatement, torch.optim.Adam on the GPU in fp32) as (p, m, v) lists on the CPU, computed once."""
    params, grads, norms = case(geo_name)
    wd, clip = CONFIGS[cfg_name]
    mn = max_norm_of(clip, norms[:steps])
    p64, m64, v64, n64 = clip_adam(params, grads[:steps], lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, max_norm=mn)
    dev = torch.device("cuda:0")
    live = [torch.nn.Parameter(p.to(dev)) for p in params]
    opt = torch.optim.Adam(live, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, foreach=False)
    for gs in grads[:steps]:
        for p, g in zip(live, gs):
            p.grad = g.to(dev)
        if mn is not None:
            torch.nn.utils.clip_grad_norm_(live, mn, foreach=False)
        opt.step()
    t32 = ([p.detach().cpu() for p in live], [opt.state[p]["exp_avg"].cpu() for p in live],
           [opt.state[p]["exp_avg_sq"].cpu() for p in live])
    return (p64, m64, v64), t32, n64, mn


def assert_within_allowance(got, ref64, torch32, what, torch_ref64=None):
    """torch_ref64: the float64 result torch's leg is measured against, where it was fed other gradients than `got`'s leg."""
    for i, (a, r, t) in enumerate(zip(got, ref64, torch32)):
        tr = r if torch_ref64 is None else torch_ref64[i]
        allow = max(3.0 * (t.double() - tr).abs().max().item(), 2.0 ** -23 * r.abs().max().item())
        err = (a.double().cpu() - r).abs().max().item()
        assert err <= allow, f"{what}[{i}]: error {err:.3e} > allowance {allow:.3e}"


def run_fused(lsnf, geo_name, steps, wd, mn, dev, offset=0, grads_override=None, want_norm=False):
    """`steps` calls of flow.adam_step on fresh state; returns (p, m, v, norms).  offset: every parameter and gradient is a view
    `offset` floats into a 16-byte aligned buffer."""
    geo = GEOS[geo_name]
    params, grads, _ = case(geo_name)

    def put(t):
        buf = torch.zeros(t.numel() + 4 + offset, device=dev)
        assert buf.data_ptr() % 16 == 0
        v = buf[offset: offset + t.numel()].view(t.shape)
        v.copy_(t)
        return v

    p = [put(t) for t in params]
    state = lsnf.flow.new_adam_state(*geo, dev)
    norms = []
    for k in range(steps):
        gs = grads[k] if grads_override is None else grads_override[k]
        g = [None if t is None else put(t) for t in gs]
        n = lsnf.flow.adam_step(p, g, state, *geo, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, max_norm=mn, want_norm=want_norm)
        norms.append(None if n is None else n.clone())
    steps_view, _, m, v = lsnf.flow.adam_state_views(state, *geo)
    assert steps_view[0].item() == steps
    return p, m, v, norms


@pytest.mark.parametrize("steps", [1, 5])
@pytest.mark.parametrize("cfg_name", list(CONFIGS))
@pytest.mark.parametrize("geo_name", list(GEOS))
def test_matches_float64_within_torch_adams_own_error(lsnf, gpu_device, geo_name, cfg_name, steps):
    ref64, t32, n64, mn = references(geo_name, cfg_name, steps)
    p, m, v, norms = run_fused(lsnf, geo_name, steps, CONFIGS[cfg_name][0], mn, gpu_device, want_norm=True)
    for got, r, t, what in zip((p, m, v), ref64, t32, "pmv"):
        assert_within_allowance(got, r, t, what)
    for n, r in zip(norms, n64):          # float64 accumulation, one rounding to fp32
        assert abs(n.item() - r) <= 2.0 ** -22 * r


@pytest.mark.parametrize("geo_name", ["odd", "reference"])
def test_two_fresh_runs_are_bit_identical(lsnf, gpu_device, geo_name):
    _, _, norms = case(geo_name)
    runs = [run_fused(lsnf, geo_name, 5, 1e-2, 0.5 * min(norms), gpu_device) for _ in range(2)]
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.equal(x, y) for x, y in zip(runs[0][3], runs[1][3]))


@pytest.mark.parametrize("geo_name", ["tiny", "odd", "reference"])
def test_max_norm_above_the_norm_gives_the_unclipped_bits(lsnf, gpu_device, geo_name):
    _, _, norms = case(geo_name)
    clipped = run_fused(lsnf, geo_name, 5, 1e-2, 2.0 * max(norms), gpu_device)
    plain = run_fused(lsnf, geo_name, 5, 1e-2, None, gpu_device)
    assert all(n is None for n in plain[3]) and all(n is not None for n in clipped[3])
    for a, b in zip(clipped[:3], plain[:3]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("geo_name", ["tiny", "odd", "max-depth"])
def test_views_off_the_16_byte_boundary_give_the_aligned_bits(lsnf, gpu_device, geo_name):
    """Parameters and gradients 4 bytes off a 16-byte boundary (the scalar path); the state itself must be 16-byte aligned, its
    m / v slices sit wherever the tensor sizes put them (`odd`: mostly off the boundary)."""
    _, _, norms = case(geo_name)
    a = run_fused(lsnf, geo_name, 3, 1e-2, 0.5 * min(norms), gpu_device)
    b = run_fused(lsnf, geo_name, 3, 1e-2, 0.5 * min(norms), gpu_device, offset=1)
    assert b[0][0].data_ptr() % 16 == 4
    for x, y in zip(a[:3], b[:3]):
        assert all(torch.equal(s, t) for s, t in zip(x, y))
    assert all(torch.equal(s, t) for s, t in zip(a[3], b[3]))


def test_none_gradient_freezes_and_zero_gradient_decays(lsnf, gpu_device):
    geo_name = "odd"
    params, grads, _ = case(geo_name)
    skipped, zeroed = {1, 2, 14, 23}, {0, 6, 18}
    gs = [[None if i in skipped else (torch.zeros_like(g) if i in zeroed else g) for i, g in enumerate(step)] for step in grads[:3]]
    p, m, v, norms = run_fused(lsnf, geo_name, 3, 1e-2, 0.05, gpu_device, grads_override=gs)
    for i in skipped:
        assert torch.equal(p[i].cpu(), params[i]) and not m[i].any() and not v[i].any()
    for i in zeroed:          # an explicit zero gradient is a gradient: weight decay moves the tensor
        assert not torch.equal(p[i].cpu(), params[i]) and m[i].any() and v[i].any()
    p64, m64, v64, n64 = clip_adam(params, gs, lr=LR, betas=BETAS, eps=EPS, weight_decay=1e-2, max_norm=0.05)
    for n, r in zip(norms, n64):          # a skipped tensor contributes nothing to the norm
        assert abs(n.item() - r) <= 2.0 ** -22 * r


def test_argument_errors(lsnf, gpu_device):
    import ctypes
    geo = GEOS["tiny"]
    F, lib = lsnf.flow, lsnf.load_library()
    params = [t.to(gpu_device) for t in case("tiny")[0]]
    grads = [t.to(gpu_device) for t in case("tiny")[1][0]]
    state = F.new_adam_state(*geo, gpu_device)
    before = [p.clone() for p in params]
    tab = (ctypes.c_void_p * 12)(*[p.data_ptr() for p in params])
    gtab = (ctypes.c_void_p * 12)(*[g.data_ptr() for g in grads])

    def raw(st=state.data_ptr(), b1=0.5, b2=0.999, eps=1e-8):
        return lib.lsnf_adam_step(tab, gtab, *geo, st, 1e-3, None, b1, b2, eps, 0.0, 0.0, None, None)

    assert raw(st=None) == -1 and raw(st=state.data_ptr() + 4) == -1 and raw(b1=1.0) == -1 and raw(b2=1.0) == -1 and raw(eps=-1e-8) == -1
    with pytest.raises(lsnf.LsnfError):
        F.adam_step(params, grads, state, *geo, betas=(1.0, 0.999))
    with pytest.raises(lsnf.LsnfError):
        F.adam_step(params, grads, state, *geo, eps=-1e-8)
    with pytest.raises(lsnf.LsnfError):
        F.adam_step(params, grads[:3] + [grads[3].cpu()] + grads[4:], state, *geo)        # a gradient on another device
    with pytest.raises(lsnf.LsnfError):
        F.adam_step(params, grads, state[: state.numel() - 4], *geo)                      # an undersized state
    with pytest.raises(lsnf.LsnfError):
        F.adam_step(params, grads, state[1:], *GEOS["tiny"])                              # ... and a misaligned one
    with pytest.raises(lsnf.LsnfError):
        F.adam_step(params, grads, None, *geo)
    with pytest.raises(lsnf.LsnfError):
        F.adam_step(params, grads[:-1], state, *geo)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(params, before)) and not state.any()     # nothing was launched


# ---- module level ------------------------------------------------------------------------------------------------------
def make_net(lsnf, nz, w, d, dev, seed=3):
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=d, f_flow_permutation=2, f_width=w, f_flow_coupling=1)
    net = lsnf._netF(hps, nz=nz)
    net.load_state_dict(O.init_params(nz, w, d, seed=seed), strict=True)
    return net.to(dev)


def oracle_params(net):
    return {k: v.detach().double().cpu() for k, v in net.state_dict().items()}


HYPER = dict(lr=1e-3, betas=BETAS, weight_decay=1e-2)


@pytest.mark.parametrize("nz,w", [(8, 4), (128, 64)])
def test_mle_step_refreshes_the_plan_and_tracks_torch_adam(lsnf, gpu_device, nz, w):
    B, d = 33, 5
    z = torch.randn(B, nz, generator=torch.Generator().manual_seed(9))
    zd = z.to(gpu_device)
    net, twin = make_net(lsnf, nz, w, d, gpu_device), make_net(lsnf, nz, w, d, gpu_device)
    opt = lsnf.FlowAdam(net, max_norm=0.5, **HYPER)
    topt = torch.optim.Adam(twin.parameters(), foreach=False, **HYPER)
    losses, twin_losses, start = [], [], [p.detach().cpu() for p in net._param_list()]
    gnet, gtwin = [], []
    for _ in range(3):
        losses.append(net.mle_step(zd, opt))
        assert net._plan_key == net._current_key()                 # the plan was left current
        gnet.append([p.grad.detach().cpu().clone() for p in net._param_list()])       # unclipped: the optimizer clips in registers
        ll = net.log_prob(zd)[2].double().cpu()
        ll_ref = O.flow_log_prob(oracle_params(net), z.double())[2]
        assert ((ll - ll_ref).abs() / ll_ref.abs()).max().item() <= 1e-5      # ... and it holds the written values
        topt.zero_grad(set_to_none=True)
        twin_losses.append(twin.mle_grads(zd, max_norm=0.5, reuse_buffers=True))
        gtwin.append([p.grad.detach().cpu().clone() for p in twin._param_list()])     # clipped in place by mle_grads
        topt.step()
    assert opt.last_grad_norm is not None and opt.last_grad_norm.item() > 0.5      # the clip was active
    assert losses[2].item() < losses[0].item()
    for a, b in zip(losses, twin_losses):          # the two modules walk the same path (the forward's gate on ll)
        assert abs(a.item() - b.item()) <= 1e-5 * abs(b.item())
    # Each fp32 leg against the float64 restatement fed ITS OWN fp32 gradients -- from the second step on the two modules'
    # gradients differ in their last bits, and Adam's normalised update amplifies that on elements whose gradient is small --
    # with torch's deviation from its float64 leg setting the allowance for the fused step's deviation from its own.
    kw = dict(lr=HYPER["lr"], betas=BETAS, eps=EPS, weight_decay=HYPER["weight_decay"])
    p64, _, _, n64 = clip_adam(start, gnet, max_norm=0.5, **kw)
    t64, _, _, _ = clip_adam(start, gtwin, **kw)
    tw = [p.detach().cpu() for p in twin._param_list()]
    assert_within_allowance([p.detach() for p in net._param_list()], p64, tw, "param", torch_ref64=t64)
    assert abs(opt.last_grad_norm.item() - n64[2]) <= 2.0 ** -22 * n64[2]
    for name, q in net.named_parameters():         # the reference's dead fc_*.b: no gradient, no state, same bits under weight decay
        if name.endswith(("fc_1.b", "fc_2.b")):
            assert q.grad is None and not q.any()
    assert len(opt.state_dict()["state"]) == 12 * d


def test_stale_weights_guard_sees_the_step(lsnf, gpu_device):
    net = make_net(lsnf, 8, 4, 2, gpu_device)
    opt = lsnf.FlowAdam(net, lr=1e-3)
    z = torch.randn(5, 8, device=gpu_device)
    z1, logdet, _ = net(z, torch.zeros(5, device=gpu_device))
    for p in net._param_list():
        p.grad = torch.ones_like(p)
    opt.step()
    with pytest.raises(lsnf.LsnfError, match="modified between forward and backward"):
        (z1.sum() + logdet.sum()).backward()
    with pytest.raises(lsnf.LsnfError, match="flow_mle_step"):
        net.mle_step(z, torch.optim.Adam(net.parameters()))


def test_exponential_lr_drives_the_next_update(lsnf, gpu_device):
    geo_name = "additive"
    nz, w, d, c = GEOS[geo_name]
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=d, f_flow_permutation=2, f_width=w, f_flow_coupling=c)
    net = lsnf._netF(hps, nz=nz).to(gpu_device)
    params, grads, _ = case(geo_name)
    with torch.no_grad():
        for p, t in zip(net._param_list(), params):
            p.copy_(t)
    opt = lsnf.FlowAdam(net, lr=1e-3, betas=BETAS)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, 0.5)
    lrs = []
    for k in range(3):
        for p, g in zip(net._param_list(), grads[k]):
            p.grad = g.to(gpu_device)
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
        opt.zero_grad()
    assert lrs == [1e-3, 5e-4, 2.5e-4]
    p64, _, _, _ = clip_adam(params, grads[:3], lr=lrs, betas=BETAS, eps=EPS)
    pfix, _, _, _ = clip_adam(params, grads[:3], lr=1e-3, betas=BETAS, eps=EPS)
    # three steps, each a handful of fp32 roundings on p: within 8 ulp of the largest entry, and 100 times closer to the scheduled
    # rates than the fixed rate is (the two differ by lr-sized steps)
    for q, r, f in zip(net._param_list(), p64, pfix):
        err = (q.detach().double().cpu() - r).abs().max().item()
        assert err <= 2.0 ** -20 * r.abs().max().item() and err < 0.01 * (f - r).abs().max().item()


# ---- state dict ----------------------------------------------------------------------------------------------------------
def set_grads(net, grads, dev):
    for p, g in zip(net._param_list(), grads):
        p.grad = g.to(dev)


@pytest.mark.parametrize("direction", ["fused-to-torch", "torch-to-fused"])
def test_state_dict_round_trip_with_torch_adam(lsnf, gpu_device, direction):
    geo_name = "reference"
    nz, w, d, _ = GEOS[geo_name]
    _, grads, _ = case(geo_name)
    src_net, dst_net = make_net(lsnf, nz, w, d, gpu_device), make_net(lsnf, nz, w, d, gpu_device)
    hyper = dict(lr=1e-3, betas=BETAS, weight_decay=1e-2)
    fused_first = direction == "fused-to-torch"
    mk_f = lambda n: lsnf.FlowAdam(n, **hyper)
    mk_t = lambda n: torch.optim.Adam(n.parameters(), foreach=False, **hyper)
    src, dst = (mk_f(src_net), mk_t(dst_net)) if fused_first else (mk_t(src_net), mk_f(dst_net))
    start = [p.detach().cpu() for p in src_net._param_list()]
    for k in range(3):
        set_grads(src_net, grads[k], gpu_device)
        src.step()
    sd = src.state_dict()
    assert len(sd["state"]) == 12 * d and len(sd["param_groups"][0]["params"]) == 14 * d      # the dead fc_*.b carry no state
    dst.load_state_dict(sd)
    dst_net.load_state_dict(src_net.state_dict())
    for net, opt in ((src_net, src), (dst_net, dst)):
        set_grads(net, grads[3], gpu_device)
        opt.step()
    # both sides against float64, with an all-torch run of the same four steps as the fp32 reference leg
    p64, _, _, _ = clip_adam(start, grads[:4], eps=EPS, **hyper)
    leg = references_torch_only(start, grads[:4], hyper)
    for net in (src_net, dst_net):
        assert_within_allowance([p.detach() for p in net._param_list()], p64, leg, "param")
    for name, q in dst_net.named_parameters():
        if name.endswith(("fc_1.b", "fc_2.b")):
            assert not q.any()
    # exp_avg / exp_avg_sq are copies, not aliases of the flat state
    f_opt = src if fused_first else dst
    sd2 = f_opt.state_dict()
    sd2["state"][0]["exp_avg"].add_(1.0)
    assert not torch.equal(sd2["state"][0]["exp_avg"], f_opt.state_dict()["state"][0]["exp_avg"])


def references_torch_only(start, grad_steps, hyper):
    dev = torch.device("cuda:0")
    live = [torch.nn.Parameter(p.to(dev)) for p in start]
    opt = torch.optim.Adam(live, foreach=False, **hyper)
    for gs in grad_steps:
        for p, g in zip(live, gs):
            p.grad = g.to(dev)
        opt.step()
    return [p.detach().cpu() for p in live]


# ---- graph ---------------------------------------------------------------------------------------------------------------
def test_captured_step_replays_eager_bits_and_follows_lr(lsnf, gpu_device):
    geo_name = "reference"
    nz, w, d, _ = GEOS[geo_name]
    _, grads, norms = case(geo_name)
    hyper = dict(lr=1e-3, betas=BETAS, weight_decay=1e-2, max_norm=0.5 * min(norms), capturable=True)
    lrs = [1e-3, 1e-3, 4e-4]

    def fresh():
        net = make_net(lsnf, nz, w, d, gpu_device)
        for p in net._param_list():
            p.grad = torch.zeros_like(p)          # static gradient buffers
        return net, lsnf.FlowAdam(net, **hyper)

    def feed(net, k):
        with torch.no_grad():
            for p, g in zip(net._param_list(), grads[k]):
                p.grad.copy_(g)

    eager_net, eager = fresh()
    for k in range(3):
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
    for k in range(3):
        feed(net, k)
        opt.param_groups[0]["lr"] = lrs[k]
        opt.sync_lr()                             # a replay runs no Python: the device copy of lr is refreshed here
        graph.replay()
    torch.cuda.synchronize()
    a, b = lsnf.flow.adam_state_views(opt._flat, *GEOS[geo_name]), lsnf.flow.adam_state_views(eager._flat, *GEOS[geo_name])
    assert a[0][0].item() == 3 and b[0][0].item() == 3
    assert torch.equal(a[1], b[1])
    for x, y in zip(list(net._param_list()) + a[2] + a[3], list(eager_net._param_list()) + b[2] + b[3]):
        assert torch.equal(x.detach(), y.detach())
    # the lr change took effect: with the first rate throughout the parameters would differ
    cpu_w = [t.cpu() for t in weights]
    p_const, _, _, _ = clip_adam(cpu_w, grads[:3], lr=1e-3, betas=BETAS, eps=EPS, weight_decay=1e-2, max_norm=hyper["max_norm"])
    p_sched, _, _, _ = clip_adam(cpu_w, grads[:3], lr=lrs, betas=BETAS, eps=EPS, weight_decay=1e-2, max_norm=hyper["max_norm"])
    q = net._param_list()[2].detach().double().cpu()
    assert (q - p_sched[2].cpu()).abs().max().item() < 0.01 * (p_const[2] - p_sched[2]).abs().max().item()
    # the replayed plan refresh holds the final values
    z = torch.randn(33, nz, generator=torch.Generator().manual_seed(2))
    plan_ll = lsnf.flow.forward(net._cached_plan, z.to(gpu_device))[2].double().cpu()
    ll_ref = O.flow_log_prob(oracle_params(net), z.double())[2]
    assert ((plan_ll - ll_ref).abs() / ll_ref.abs()).max().item() <= 1e-5

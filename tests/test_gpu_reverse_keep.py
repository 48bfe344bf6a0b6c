"""GPU: the stash-keeping reverse (lsnf_reverse_keep / lsnf_sample_keep, the KEEP form of lsnf_small3_rev_kernel), the module's
`reverse_keeps_stash` bridge and the eps-space Langevin sampler, against float64 autograd of oracle/flow_oracle.py.

Inputs are kink-free inputs of the REVERSE (eps = f_fp64(oracle.smooth_batch(...)), as tests/test_gpu_reverse_autograd.py builds them),
so no row is ever set aside.  Tolerances: max(floor, 3 x the oracle's OWN fp32-vs-fp64 error for that quantity on that input,
computed here on the CPU) -- floors 1e-5 (d eps, block outputs; rel-L2), 2e-5 (rel-L2 per parameter tensor), 2e-5 (trajectory).
Every comparison prints `measured / allowed / oracle-fp32` (run with -s to collect the table)."""
import ctypes
import functools
import math
import types

import pytest
import torch

from oracle import flow_oracle as O
from oracle.philox_oracle import langevin_noise
import reverse_restated as R
import trained_weights as T

pytestmark = pytest.mark.gpu

C3, C5, TINY, C1 = (128, 64, 5, 1), (100, 128, 5, 1), (8, 4, 5, 1), (100, 64, 5, 1)
# (nz, width, depth, coupling, B).  C3: B = 1; 17 (a second 16-row tile inside one 32-sample stash tile); 33; 100; 4 100 (32 rows per
# workgroup, ragged); 8 200 (64 rows, ragged).  C5 (WT = 4: 16 / 32 rows only), nz 126 / w 127, nz 2 / w 1, depth 1 and 16, additive.
CASES = [C3 + (1,), C3 + (17,), C3 + (33,), C3 + (100,), C3 + (4100,), C3 + (8200,),
         TINY + (33,), TINY + (100,), C5 + (33,), C5 + (100,), (126, 127, 2, 1, 33), (126, 127, 2, 1, 100), (2, 1, 3, 1, 33), (2, 1, 3, 1, 100),
         (64, 32, 1, 1, 33), (64, 32, 1, 1, 100), (20, 12, 16, 1, 33), (20, 12, 16, 1, 100), (20, 12, 5, 0, 33), (20, 12, 5, 0, 100), (100, 64, 5, 0, 33), (100, 64, 5, 0, 100)]
PARAM_CASES = [C3 + (100,), C3 + (4100,), C5 + (33,), (64, 32, 1, 1, 100), (20, 12, 16, 1, 33)]
MODES = ["bf16x3", "fp16x2"]


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


@pytest.fixture(params=MODES)
def mode(request, lsnf):
    F = lsnf.flow
    prev = F.set_math_mode(F.MATH_BF16X3 if request.param == "bf16x3" else F.MATH_FP16X2)
    prev_max = F.set_small_batch_max(F.SMALL_BATCH_AUTO)
    yield request.param
    F.set_small_batch_max(prev_max)
    F.set_math_mode(prev)


def report(what, got, allowed, own):
    print(f"[reverse-keep] {what}: measured {got:.3e} allowed {allowed:.3e} oracle-fp32 {own:.3e}")


def additive(p):
    q = dict(p)
    for k in p:
        if ".f.fc_zeros." in k:
            q[k] = p[k][:, : p[k].shape[1] // 2].contiguous()
    return q


def seeded(B, nz, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, nz, generator=gen), torch.randn(B, generator=gen), torch.randn(B, generator=gen)


def block_outputs(p, x):
    """Outputs of forward blocks 0 .. depth-2 at x, in x's dtype: (depth-1, B, nz)."""
    q = O.to_dtype(p, x.dtype)
    z, ld, outs = x, torch.zeros(x.shape[0], dtype=x.dtype), []
    for i in range(O.depth_of(q)):
        z, ld = O.block_fwd(q, i, z, ld, O.coupling_of(q))
        outs.append(z)
    return torch.stack(outs[:-1]) if len(outs) > 1 else x.new_zeros((0,) + tuple(x.shape))


def forward_vjp(p, x, g_z1, g_ld, dtype):
    """J_f(x)^T g_z1 + g_ld * grad_x logdet_f(x) by autograd of the oracle's forward in `dtype`."""
    q = O.to_dtype(p, dtype)
    xx = x.to(dtype).clone().requires_grad_(True)
    z1, ld = O.flow_forward(q, xx, torch.zeros(xx.shape[0], dtype=dtype))
    return torch.autograd.grad((z1 * g_z1.to(dtype)).sum() + (ld * g_ld.to(dtype)).sum(), xx)[0]


class Case:
    """One geometry and batch: the inputs and every float64 / float32 oracle figure the tests share, each computed once on the CPU."""

    def __init__(self, nz, w, depth, coupling, B, weights=T.INIT):
        self.geo, self.B, self.nz, self.depth, self.weights = (nz, w, depth, coupling), B, nz, depth, weights
        p = T.params_for(O, self.geo, weights)
        self.p = additive(p) if coupling == 0 else p
        x, _ = O.smooth_batch(self.p, B, nz, seed=B)
        self.eps = R.forward64(self.p, x)[0].float()
        self.gx, self.go, self.obj = seeded(B, nz, 100 + B)
        assert (O.relu_margin(self.p, R.reverse64(self.p, self.eps)) > 1e-5).all()      # kink-free: no row is set aside

    @functools.cached_property
    def grads(self):
        """float64 and float32 autograd of the oracle's reverse: (x64, g_eps64, params64, x32, g_eps32, params32)."""
        x64, _, g64, p64 = R.reverse_loss_grads(self.p, self.eps, self.obj, self.gx, self.go, torch.float64, want_params=True)
        x32, _, g32, p32 = R.reverse_loss_grads(self.p, self.eps, self.obj, self.gx, self.go, torch.float32, want_params=True)
        return x64, g64, p64, x32, g32, p32

    @functools.cached_property
    def blocks(self):
        x64, _, _, x32, _, _ = self.grads
        return block_outputs(self.p, x64), block_outputs(self.p, x32)

    @functools.cached_property
    def fwd_vjp(self):
        x64, _, _, x32, _, _ = self.grads
        return forward_vjp(self.p, x64, self.gx, self.go, torch.float64), forward_vjp(self.p, x32, self.gx, self.go, torch.float32)

    @functools.cached_property
    def route32(self):
        """The parameter gradients in float32 BY THE ROUTE THE LIBRARY TAKES: x = f^-1(eps), then the forward's backward at x with the
        upstream (-g_eps, -go) -- in exact arithmetic J_f^T J_f^-T gx, the gradients of Case.grads (float64 by this route meets them
        to 1e-13).  Autograd of the reverse itself, Case.grads' float32, does not see this route's conditioning: block 0's actnorm.b
        is the reverse's last operation there, d L / d b = -sum gx whatever the weights (own error 1e-7), while by this route it is
        that sum carried through J_f^-T and back, 9e-5 in float32 on the trained C3 weights against 3e-6 on the init ones."""
        _, _, _, x32, g32, _ = self.grads
        q = {k: v.float().clone().requires_grad_(True) for k, v in self.p.items()}
        z1, ld = O.flow_forward(q, x32, torch.zeros(self.B))
        grads = torch.autograd.grad(-(z1 * g32).sum() - (ld * self.go).sum(), list(q.values()), allow_unused=True)
        return {k: g for k, g in zip(q, grads) if g is not None}


@functools.lru_cache(maxsize=None)
def case(nz, w, depth, coupling, B, weights=T.INIT):
    return Case(nz, w, depth, coupling, B, weights)


def make_plan(lsnf, c, dev):
    nz, w, d, cp = c.geo
    return lsnf.prepare(lsnf.params_from_state_dict(c.p, d, dev), nz, w, d, cp)


def keep_call(lsnf, plan, c, dev, with_ws=False):
    """(x, obj_out, saved, act, ws, eps) of flow.reverse with the stash kept; the stash is NaN-filled first: every word a backward
    reads of a live row must have been written by the reverse."""
    F = lsnf.flow
    act = F.new_act_saved(plan, c.B, dev)
    act.fill_(float("nan"))
    ws = F.new_params_workspace(plan, c.B, dev) if with_ws else None
    if ws is not None:
        ws.fill_(float("nan"))
    eps, obj = c.eps.to(dev), c.obj.to(dev)
    x, o, saved = F.reverse(plan, eps, obj, save_for_backward=True, act_saved=act, params_ws=ws)
    return x, o, saved, act, ws, eps


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------
# 1 - 3. kernel level: bits, block outputs, the stash does its job
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz,w,depth,coupling,B", CASES)
def test_keep_form_bits_block_outputs_and_stash(lsnf, mode, gpu_device, nz, w, depth, coupling, B, weights=T.INIT):
    c = case(nz, w, depth, coupling, B, weights)
    mode = mode if weights == T.INIT else f"{mode} {weights}"
    dev, F, lib = gpu_device, lsnf.flow, lsnf.load_library()
    plan = make_plan(lsnf, c, dev)
    assert F.reverse_keep_supported(plan, B)
    x, o, saved, act, _, eps = keep_call(lsnf, plan, c, dev)
    # 1. bit identity with the plain call, also with all three optional pointers NULL
    x0, o0 = F.reverse(plan, eps, c.obj.to(dev))
    assert torch.equal(x, x0) and torch.equal(o, o0)
    xn, on = torch.empty_like(x), torch.empty_like(o)
    sp = torch.cuda.current_stream(dev).cuda_stream
    objd = c.obj.to(dev)
    assert lib.lsnf_reverse_keep(ptr(plan.buf), *c.geo, B, ptr(eps), ptr(objd), ptr(xn), ptr(on), None, None, None, sp) == 0
    assert torch.equal(xn, x0) and torch.equal(on, o0)
    # 2. block outputs against float64
    x64, g64, _, _, g32, _ = c.grads
    if depth > 1:
        b64, b32 = c.blocks
        assert saved.shape == (depth - 1, B, nz) and bool(torch.isfinite(saved).all())
        for b in range(depth - 1):
            own = R.rel_l2(b32[b], b64[b])
            err = R.rel_l2(saved[b].cpu(), b64[b])
            report(f"{mode} {c.geo} B{B} block {b} output", err, max(1e-5, 3.0 * own), own)
            assert err <= max(1e-5, 3.0 * own)
    else:
        assert saved is None
    # 3. the stash does its job: the backward of the reverse from it, from the rebuilt one, and the forward's backward
    gx, go = c.gx.to(dev), c.go.to(dev)
    own = R.rel_l2(g32, g64)
    tol = max(1e-5, 3.0 * own)
    got = F.reverse_backward_z(plan, eps, saved, act, gx, go)
    err = R.rel_l2(got.cpu(), g64)
    report(f"{mode} {c.geo} B{B} d eps from the reverse's stash", err, tol, own)
    assert bool(torch.isfinite(got).all()) and err <= tol
    act2 = F.new_act_saved(plan, B, dev)
    act2.fill_(float("nan"))
    assert lib.lsnf_restash(ptr(plan.buf), *c.geo, B, ptr(eps), ptr(saved), ptr(act2), sp) == 0
    again = F.reverse_backward_z(plan, eps, saved, act2, gx, go)
    diff = R.rel_l2(got, again)
    report(f"{mode} {c.geo} B{B} d eps: reverse's stash vs lsnf_restash", diff, tol, own)
    assert diff <= tol
    v64, v32 = c.fwd_vjp
    own_v = R.rel_l2(v32, v64)
    back = F.backward_z(plan, eps, saved, gx, go, act_saved=act)
    err_v = R.rel_l2(back.cpu(), v64)
    report(f"{mode} {c.geo} B{B} backward_z from the reverse's stash", err_v, max(1e-5, 3.0 * own_v), own_v)
    assert err_v <= max(1e-5, 3.0 * own_v)


@pytest.mark.parametrize("nz,w,depth,coupling,B", T.CASES)
def test_keep_form_bits_block_outputs_and_stash_at_trained_weights(lsnf, mode, gpu_device, nz, w, depth, coupling, B):
    """The same checks and tolerances on the golden trained weights (tests/trained_weights.py)."""
    test_keep_form_bits_block_outputs_and_stash(lsnf, mode, gpu_device, nz, w, depth, coupling, B, weights=T.TRAINED)


@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (100,), C3 + (4100,), C3 + (8200,), C5 + (33,), TINY + (33,), (2, 1, 3, 1, 33)])
def test_sample_keep_is_sample_and_keeps_what_reverse_keep_keeps(lsnf, mode, gpu_device, nz, w, depth, coupling, B):
    c = case(nz, w, depth, coupling, B)
    dev, F = gpu_device, lsnf.flow
    plan = make_plan(lsnf, c, dev)
    rng = F.PhiloxNoise(2 ** 63 + 5, (1 << 40) + 3, 2 ** 32 - 5)
    x0, o0, e0, l0 = F.sample(plan, B, rng, temperature=0.9, want_eps=True, want_ll=True)
    act, ws = F.new_act_saved(plan, B, dev), F.new_params_workspace(plan, B, dev)
    act.fill_(float("nan")); ws.fill_(float("nan"))
    x, o, e, ll, saved = F.sample(plan, B, rng, temperature=0.9, want_ll=True, save_for_backward=True, act_saved=act, params_ws=ws)
    assert torch.equal(x, x0) and torch.equal(o, o0) and torch.equal(e, e0) and torch.equal(ll, l0)
    # the same rows through lsnf_reverse_keep: the same arithmetic after the row load, so the same bits everywhere
    act_r, ws_r = F.new_act_saved(plan, B, dev), F.new_params_workspace(plan, B, dev)
    act_r.fill_(float("nan")); ws_r.fill_(float("nan"))
    xr, _, saved_r = F.reverse(plan, e, None, save_for_backward=True, act_saved=act_r, params_ws=ws_r)
    assert torch.equal(xr, x)
    assert (saved is None and saved_r is None) or torch.equal(saved, saved_r)
    # (the stash words of the rows past B inside the last 16-row tile differ: the sampling form draws them, the reverse repeats row B-1;
    #  what a backward reads of the live rows is the same -- and h1 / h2 are written for live rows only)
    gx, go = c.gx.to(dev), c.go.to(dev)
    g = F.reverse_backward_z(plan, e, saved, act, gx, go)
    assert bool(torch.isfinite(g).all()) and torch.equal(g, F.reverse_backward_z(plan, e, saved_r, act_r, gx, go))
    live = ~torch.isnan(ws_r)
    assert int(live.sum()) == 2 * depth * B * w and torch.equal(ws[live], ws_r[live]) and torch.equal(torch.isnan(ws), ~live)
    with pytest.raises(lsnf.LsnfError):
        F.sample(plan, B, rng, out=(x, o, None, None), save_for_backward=True, act_saved=act)       # a stash needs eps


def test_every_tensor_four_bytes_off_a_16_byte_boundary(lsnf, mode, gpu_device):
    c = case(*C3, 33)
    dev, F, lib = gpu_device, lsnf.flow, lsnf.load_library()
    plan = make_plan(lsnf, c, dev)
    x, o, saved, act, ws, eps = keep_call(lsnf, plan, c, dev, with_ws=True)

    def off4(t):
        b = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
        assert b.data_ptr() % 16 == 0
        v = b[1: 1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    e4, obj4 = off4(eps), off4(c.obj.to(dev))
    x4, o4, s4 = off4(torch.zeros_like(x)), off4(torch.zeros_like(o)), off4(torch.zeros_like(saved))
    act4, ws4 = torch.full_like(act, float("nan")), torch.full_like(ws, float("nan"))
    sp = torch.cuda.current_stream(dev).cuda_stream
    assert lib.lsnf_reverse_keep(ptr(plan.buf), *c.geo, c.B, ptr(e4), ptr(obj4), ptr(x4), ptr(o4), ptr(s4), ptr(act4), ptr(ws4), sp) == 0
    assert torch.equal(x4, x) and torch.equal(o4, o) and torch.equal(s4, saved)
    for a, b in ((act4, act), (ws4, ws)):
        live = ~torch.isnan(b)
        assert torch.equal(a[live], b[live]) and torch.equal(torch.isnan(a), ~live)
    assert lib.lsnf_reverse_keep(ptr(plan.buf), *c.geo, c.B, ptr(e4), ptr(obj4), ptr(x4), ptr(o4), ptr(s4),
                                 ctypes.c_void_p(act4.data_ptr() + 4), None, sp) == -1


# ---------------------------------------------------------------------------------------------
# 4. parameter gradients from the reverse's workspace (the h1 / h2 dump and the tag)
# ---------------------------------------------------------------------------------------------
TRAINED_PARAM_GATE = 1e-4                   # the plain kernels' gate per parameter tensor on the trained goldens (tests/test_gpu_module.py)


def check_param_grads(lsnf, label, keys, grads, p64, p32, floor=2e-5, route32=None):
    """A tensor's bound is max(floor, 3 x its float32 own error).  route32 (the trained cases alone): a second float32 restatement,
    Case.route32; where 3 x ITS error is the larger the bound is that, but never above TRAINED_PARAM_GATE."""
    worst = (0.0, 0.0, 0.0, "", 0.0)
    for k, g in zip(keys, grads):
        own_k = R.rel_l2(p32[k], p64[k])
        tol_k = max(floor, 3.0 * own_k)
        if route32 is not None:
            route_k = R.rel_l2(route32[k].reshape(p64[k].shape), p64[k])
            tol_k, own_k = max(tol_k, min(3.0 * route_k, TRAINED_PARAM_GATE)), max(own_k, route_k)
        err_k = R.rel_l2(g.cpu().reshape(p64[k].shape), p64[k])
        if err_k / tol_k >= worst[0]:
            worst = (err_k / tol_k, err_k, own_k, k, tol_k)
    report(f"{label} d theta worst {worst[3]}", worst[1], worst[4] if worst[3] else floor, worst[2])
    assert worst[0] <= 1.0, worst


def param_keys(lsnf, depth):
    return [O.block_prefix(i) + k for i in range(depth) for k in lsnf.flow.BLOCK_PARAM_KEYS]


@pytest.mark.parametrize("nz,w,depth,coupling,B", PARAM_CASES)
def test_parameter_gradients_from_the_reverse_workspace(lsnf, mode, gpu_device, nz, w, depth, coupling, B, weights=T.INIT):
    c = case(nz, w, depth, coupling, B, weights)
    mode = mode if weights == T.INIT else f"{mode} {weights}"
    dev, F = gpu_device, lsnf.flow
    params = lsnf.params_from_state_dict(c.p, depth, dev)
    plan = lsnf.prepare(params, nz, w, depth, coupling)
    assert F.params_fast_path()
    x, _, saved, act, ws, eps = keep_call(lsnf, plan, c, dev, with_ws=True)
    go = c.go.to(dev)
    g_eps = F.reverse_backward_z(plan, eps, saved, act, c.gx.to(dev), go)
    grads = F.backward_params(plan, params, x, eps, saved, g_eps.neg(), go.neg(), act_saved=act, workspace=ws)
    _, _, p64, _, _, p32 = c.grads
    assert len(grads) == depth * 12
    # (trained weights: the float32 restatement whose error widens a bound is the one of the route taken -- Case.route32)
    check_param_grads(lsnf, f"{mode} {c.geo} B{B}", param_keys(lsnf, depth), grads, p64, p32, route32=None if weights == T.INIT else c.route32)


TRAINED_PARAM_CASES = [c for c in PARAM_CASES if c in T.CASES]                 # C3 at 100 and 4100 rows, C5 at 33


@pytest.mark.parametrize("nz,w,depth,coupling,B", TRAINED_PARAM_CASES)
def test_parameter_gradients_from_the_reverse_workspace_at_trained_weights(lsnf, mode, gpu_device, nz, w, depth, coupling, B):
    """The init-weight bound per tensor, max(2e-5, 3 x the error of float32 autograd of the reverse), fails here on one tensor: block
    0's actnorm.b at C3 / 4100 rows, 3.9e-5 on the device with an own error of 1.2e-7.  That is the arithmetic's error on
    ill-conditioned weights, not a defect: under autograd of the reverse that tensor is the last operation (-sum gx whatever the
    weights), while the library's route is J_f^T J_f^-T gx -- exact to 1e-13 in float64, 9.2e-5 in a plain float32 restatement of
    the same route on these weights (Case.route32; 3.4e-6 on the init ones).  So for the trained cases alone a tensor's bound may
    grow to 3 x that restatement's error, capped at the plain kernels' documented gate for the parameter gradients on the trained
    goldens, 1e-4 per tensor (TRAINED_PARAM_GATE).  No init-weight bound moves (profiles/chain_trained.txt, section 4)."""
    test_parameter_gradients_from_the_reverse_workspace(lsnf, mode, gpu_device, nz, w, depth, coupling, B, weights=T.TRAINED)


def test_workspace_tag_is_written_from_the_contraction_s_first_row_count(lsnf, mode, gpu_device):
    """From LSNF_X3_MIN_ROWS = 12 288 rows lsnf_backward_params asks the workspace's tag which form h1 / h2 have: the reverse leaves 0
    (row-major) there, as lsnf_forward does, and the contraction on the bf16 matrix pipe reads the reverse's dump."""
    nz, w, depth, coupling, B = 128, 64, 2, 1, 12288                           # (fp16x2's threshold is 12 288 rows: still covered)
    c = case(nz, w, depth, coupling, B)
    dev, F = gpu_device, lsnf.flow
    params = lsnf.params_from_state_dict(c.p, depth, dev)
    plan = lsnf.prepare(params, nz, w, depth, coupling)
    assert F.reverse_keep_supported(plan, B)
    x, _, saved, act, ws, eps = keep_call(lsnf, plan, c, dev, with_ws=True)       # (NaN-filled: a tag left as it was would not read as 0)
    tag = lsnf.load_library().lsnf_backward_params_workspace_floats(nz, w, depth, B) - 4
    assert ws[tag:tag + 1].view(torch.int32).item() == 0
    go = c.go.to(dev)
    g_eps = F.reverse_backward_z(plan, eps, saved, act, c.gx.to(dev), go)
    grads = F.backward_params(plan, params, x, eps, saved, g_eps.neg(), go.neg(), act_saved=act, workspace=ws)
    _, _, p64, _, _, p32 = c.grads
    check_param_grads(lsnf, f"tag {mode} {c.geo} B{B}", param_keys(lsnf, depth), grads, p64, p32)


# ---------------------------------------------------------------------------------------------
# 5. the coverage rule
# ---------------------------------------------------------------------------------------------
def test_coverage_rule_is_one_rule(lsnf, gpu_device):
    c = case(*C3, 100)
    dev, F, lib = gpu_device, lsnf.flow, lsnf.load_library()
    plan = make_plan(lsnf, c, dev)
    sp = torch.cuda.current_stream(dev).cuda_stream
    Rng = lsnf._lib.LsnfRng(1, 0, None, 0)

    def refused(B):
        eps = torch.zeros(B, c.nz, device=dev)
        x, e2 = torch.empty_like(eps), torch.empty_like(eps)
        saved, act = torch.empty(c.depth - 1, B, c.nz, device=dev), F.new_act_saved(plan, B, dev)
        for keep in ((ptr(saved), ptr(act)), (None, None)):
            assert lib.lsnf_reverse_keep(ptr(plan.buf), *c.geo, B, ptr(eps), None, ptr(x), None, *keep, None, sp) == -1
            assert b"lsnf_reverse_keep" in lib.lsnf_last_error()
            assert lib.lsnf_sample_keep(ptr(plan.buf), *c.geo, B, ctypes.byref(Rng), 1.0, ptr(x), None, ptr(e2), None, *keep, None, sp) == -1
            assert b"lsnf_sample_keep" in lib.lsnf_last_error()
        assert lib.lsnf_reverse_keep_covers(*c.geo, B) == 0 and not F.reverse_keep_supported(plan, B)
        with pytest.raises(lsnf.LsnfError):
            F.reverse(plan, eps, None, save_for_backward=True)
        with pytest.raises(lsnf.LsnfError):
            F.reverse(plan, eps, None, act_saved=act[: act.numel() // 2])          # (the size check comes first)

    prev_math = F.set_math_mode(F.MATH_BF16X3)
    prev_max = F.set_small_batch_max(F.SMALL_BATCH_AUTO)
    try:
        top = F.set_small_batch_max(-1)
        assert lib.lsnf_reverse_keep_covers(*c.geo, top) == 1 and F.reverse_keep_supported(plan, 100)
        refused(top + 1)
        F.set_small_batch_max(64)
        assert F.reverse_keep_supported(plan, 64)
        refused(65)
        F.set_small_batch_max(F.SMALL_BATCH_AUTO)
        F.set_math_mode(F.MATH_FP32)
        refused(100)
    finally:
        F.set_small_batch_max(prev_max)
        F.set_math_mode(prev_math)
    with pytest.raises(lsnf.LsnfError):
        F.reverse(plan, c.eps.to(dev), None, act_saved=torch.empty(8, device=dev))


# ---------------------------------------------------------------------------------------------
# 6. module level
# ---------------------------------------------------------------------------------------------
def module_of(lsnf, p, dev, keeps):
    nz, w = p[O.block_prefix(0) + "actnorm.logs"].shape[1], p[O.block_prefix(0) + "f.fc_1.w"].shape[1]
    h = types.SimpleNamespace(f_n_levels=1, f_depth=O.depth_of(p), f_flow_permutation=2, f_width=w, f_flow_coupling=O.coupling_of(p))
    net = lsnf._netF(h, nz)
    net.load_state_dict(p, strict=True)
    net = net.to(dev)
    assert net.reverse_keeps_stash is False
    net.reverse_keeps_stash = keeps
    return net


def count_forward(lsnf, monkeypatch):
    calls = []
    real = lsnf.flow.forward
    monkeypatch.setattr(lsnf.flow, "forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def reverse_module_grads(lsnf, c, dev, keeps):
    net = module_of(lsnf, c.p, dev, keeps)
    e, o = c.eps.to(dev).requires_grad_(), c.obj.to(dev).requires_grad_()
    x, negobj = net(e, o, reverse=True, return_obj=True)
    # L = (x * gx).sum() + (o_out * go).sum(), o_out = -negobj: the loss of Case.grads
    ((x * c.gx.to(dev)).sum() - (negobj * c.go.to(dev)).sum()).backward()
    return net, x.detach(), e.grad, o.grad, [q.grad for q in net._param_list()]


@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (100,), C3 + (4100,), C5 + (33,), (20, 12, 5, 0, 33)])
def test_module_reverse_with_the_stash_kept(lsnf, mode, gpu_device, monkeypatch, nz, w, depth, coupling, B):
    c = case(nz, w, depth, coupling, B)
    dev = gpu_device
    calls = count_forward(lsnf, monkeypatch)
    net, x, ge, gobj, gp = reverse_module_grads(lsnf, c, dev, True)
    assert not calls                                                          # no second pass over x: the reverse kept everything
    with torch.no_grad():
        assert torch.equal(x, net(c.eps.to(dev), c.obj.to(dev), reverse=True))
    _, g64, p64, _, g32, p32 = c.grads
    own = R.rel_l2(g32, g64)
    err = R.rel_l2(ge.cpu(), g64)
    report(f"module {mode} {c.geo} B{B} d eps", err, max(1e-5, 3.0 * own), own)
    assert err <= max(1e-5, 3.0 * own)
    assert torch.equal(gobj, c.go.to(dev))
    check_param_grads(lsnf, f"module {mode} {c.geo} B{B}", param_keys(lsnf, depth), gp, p64, p32)
    # only d eps: no parameter-gradient kernels, no workspace
    bp = []
    real = lsnf.flow.backward_params
    monkeypatch.setattr(lsnf.flow, "backward_params", lambda *a, **k: (bp.append(1), real(*a, **k))[1])
    e = c.eps.to(dev).requires_grad_()
    (g_only,) = torch.autograd.grad((net(e, c.obj.to(dev), reverse=True) * c.gx.to(dev)).sum(), e)
    assert not bp and not calls and bool(torch.isfinite(g_only).all())


def test_module_default_bridge_is_untouched_and_large_batches_fall_back(lsnf, gpu_device, monkeypatch):
    dev, F = gpu_device, lsnf.flow
    c = case(*C3, 100)
    calls = count_forward(lsnf, monkeypatch)
    _, x_off, ge_off, _, gp_off = reverse_module_grads(lsnf, c, dev, False)
    assert len(calls) == 1                                                    # the default bridge: one forward at x per backward
    # the same calls by hand, as _FlowReverseFn makes them today: the same bits
    plan = make_plan(lsnf, c, dev)
    eps, obj, gx, go = (t.to(dev) for t in (c.eps, c.obj, c.gx, c.go))
    x, _ = F.reverse(plan, eps, obj)
    act, ws = F.new_act_saved(plan, c.B, dev), F.new_params_workspace(plan, c.B, dev)
    z1, _, _, saved = F.forward(plan, x, None, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
    g_eps = F.reverse_backward_z(plan, z1, saved, act, gx, go)
    assert torch.equal(x, x_off) and torch.equal(g_eps, ge_off)
    params = lsnf.params_from_state_dict(c.p, c.depth, dev)
    by_hand = F.backward_params(plan, params, x, z1, saved, g_eps.neg(), go.neg(), act_saved=act, workspace=ws)
    for a, b in zip(gp_off, by_hand):
        assert torch.equal(a.reshape(b.shape), b)
    # above the threshold the attribute falls back to that bridge, silently, and still matches float64
    prev = F.set_small_batch_max(64)
    try:
        del calls[:]
        assert not F.reverse_keep_supported(plan, c.B)
        _, _, ge, _, gp = reverse_module_grads(lsnf, c, dev, True)
        assert len(calls) == 1
    finally:
        F.set_small_batch_max(prev)
    _, g64, p64, _, g32, p32 = c.grads
    own = R.rel_l2(g32, g64)
    err = R.rel_l2(ge.cpu(), g64)
    report("module fallback above the threshold d eps", err, max(1e-5, 3.0 * own), own)
    assert err <= max(1e-5, 3.0 * own)
    check_param_grads(lsnf, "module fallback above the threshold", param_keys(lsnf, c.depth), gp, p64, p32)


@pytest.mark.parametrize("nz,w,depth,coupling,B", [C3 + (100,), TINY + (33,)])
def test_module_sample_with_the_stash_kept(lsnf, mode, gpu_device, monkeypatch, nz, w, depth, coupling, B):
    c = case(nz, w, depth, coupling, B)
    dev, F = gpu_device, lsnf.flow
    net = module_of(lsnf, c.p, dev, True)
    for offset in range(64):                          # a draw whose rows are all kink-free inputs of the reverse
        rng = F.PhiloxNoise(77, offset, 0)
        with torch.no_grad():
            _, eps = net.sample(B, rng, return_eps=True)
        if (O.relu_margin(c.p, R.reverse64(c.p, eps.cpu())) > 1e-5).all():
            break
    else:
        pytest.fail("no kink-free draw among 64 offsets")
    calls = count_forward(lsnf, monkeypatch)
    x, e2, lp = net.sample(B, rng, return_eps=True, return_log_prob=True)
    assert torch.equal(e2, eps) and x.requires_grad and lp.requires_grad and not e2.requires_grad
    with torch.no_grad():
        x0, lp0 = net.sample(B, rng, return_log_prob=True)
    assert torch.equal(x, x0) and torch.equal(lp, lp0)
    ((x * c.gx.to(dev)).sum() + (lp * c.go.to(dev)).sum()).backward()
    assert not calls
    # ll = const(eps) - objective_out: L = (x * gx).sum() + (o_out * (-go)).sum()
    zero = torch.zeros(B)
    _, _, _, p64 = R.reverse_loss_grads(c.p, eps.cpu(), zero, c.gx, -c.go, torch.float64, want_params=True)
    _, _, _, p32 = R.reverse_loss_grads(c.p, eps.cpu(), zero, c.gx, -c.go, torch.float32, want_params=True)
    check_param_grads(lsnf, f"module sample {mode} {c.geo} B{B}", param_keys(lsnf, depth), [q.grad for q in net._param_list()], p64, p32)


# ---------------------------------------------------------------------------------------------
# 7. the eps-space sampler
# ---------------------------------------------------------------------------------------------
class TanhGenerator(torch.nn.Module):
    """A fixed-seed two-layer tanh generator (B, nz, 1, 1) -> (B, 16), in the dtype it is built in."""

    def __init__(self, nz, dtype, hidden=24, out=16):
        super().__init__()
        gen = torch.Generator().manual_seed(5)
        self.w1 = (torch.randn(nz, hidden, generator=gen, dtype=torch.float64) / math.sqrt(nz)).to(dtype)
        self.b1 = (0.1 * torch.randn(hidden, generator=gen, dtype=torch.float64)).to(dtype)
        self.w2 = (torch.randn(hidden, out, generator=gen, dtype=torch.float64) / math.sqrt(hidden)).to(dtype)

    def to_device(self, dev):
        self.w1, self.b1, self.w2 = self.w1.to(dev), self.b1.to(dev), self.w2.to(dev)
        return self

    def forward(self, z):
        return torch.tanh(torch.tanh(z.flatten(1) @ self.w1 + self.b1) @ self.w2)


STEPS, STEP_SIZE, SIGMA = 3, 0.1, 0.3


def oracle_trajectory(p, eps, target, dtype):
    """STEPS noise-free steps of eps <- eps - 0.5 s^2 (eps + d/d eps 1/(2 sigma^2) |g(f^-1(eps)) - x|^2) with oracle.flow_reverse and
    autograd in `dtype`; also, per row, the smallest ReLU margin met on the way.  Returns (eps_K, f^-1(eps_K), margin)."""
    q, g = O.to_dtype(p, dtype), TanhGenerator(eps.shape[1], dtype)
    e, tgt, margin = eps.to(dtype), target.to(dtype), torch.full((eps.shape[0],), float("inf"), dtype=torch.float64)
    for _ in range(STEPS):
        e = e.clone().requires_grad_(True)
        z, _ = O.flow_reverse(q, e, torch.zeros(e.shape[0], dtype=dtype))
        margin = torch.minimum(margin, O.relu_margin(p, z.detach()))
        loss = 1.0 / (2.0 * SIGMA * SIGMA) * ((g(z) - tgt) ** 2).sum()
        (ge,) = torch.autograd.grad(loss, e)
        e = (e - 0.5 * STEP_SIZE * STEP_SIZE * (e + ge)).detach()
    return e, O.flow_reverse(q, e, torch.zeros(e.shape[0], dtype=dtype))[0], margin


@functools.lru_cache(maxsize=None)
def trajectory_case(nz, w, depth, coupling, B):
    """B rows whose float64 trajectory stays clear of every ReLU kink at every step (the rows are independent: the first B such rows
    of 2 B kink-free candidates), their targets, and the float64 / float32 oracle trajectories from them."""
    c = case(nz, w, depth, coupling, 2 * B)
    target = torch.tanh(torch.randn(2 * B, 16, generator=torch.Generator().manual_seed(9)))
    e64, z64, margin = oracle_trajectory(c.p, c.eps, target, torch.float64)
    keep = torch.nonzero(margin > 1e-5).flatten()[:B]
    assert keep.numel() == B
    e32, z32, _ = oracle_trajectory(c.p, c.eps[keep], target[keep], torch.float32)
    return c.p, c.eps[keep].contiguous(), target[keep].contiguous(), e64[keep], z64[keep], e32, z32


@pytest.mark.parametrize("nz,w,depth,coupling,B", [TINY + (33,), C1 + (100,)])
def test_eps_space_sampler_follows_the_float64_trajectory(lsnf, mode, gpu_device, monkeypatch, nz, w, depth, coupling, B):
    p, start, target, e64, z64, e32, z32 = trajectory_case(nz, w, depth, coupling, B)
    c = types.SimpleNamespace(p=p, eps=start, geo=(nz, w, depth, coupling))
    dev, F = gpu_device, lsnf.flow
    net = module_of(lsnf, c.p, dev, False)
    netG = TanhGenerator(nz, torch.float32).to_device(dev)
    calls = count_forward(lsnf, monkeypatch)
    kw = dict(g_l_steps=STEPS, g_l_step_size=STEP_SIZE, g_llhd_sigma=SIGMA)
    eps0 = c.eps.to(dev)
    e, z, gg, gf = lsnf.langevin.sample_langevin_post_eps_with_flow(eps0.view(B, nz, 1, 1), target.to(dev), netG, net, noise=False, **kw)
    assert not calls and torch.equal(eps0, c.eps.to(dev))                     # two flow launches per step; the input is not written
    assert e.shape == (B, nz) and z.shape == (B, nz, 1, 1) and gg.dim() == 0 and gf.dim() == 0
    assert torch.equal(z.view(B, nz), F.reverse(net._plan(), e, None)[0])
    for what, got, r64, r32 in (("eps", e, e64, e32), ("z", z.view(B, nz), z64, z32)):
        own = R.rel_l2(r32, r64)
        err = R.rel_l2(got.cpu(), r64)
        report(f"eps-space sampler {mode} {c.geo} B{B} {what} after {STEPS} steps", err, max(2e-5, 3.0 * own), own)
        assert err <= max(2e-5, 3.0 * own)
    # where the keep form is not supported the three-launch form runs: the same trajectory
    prev = F.set_small_batch_max(16)
    try:
        e3, _, _, _ = lsnf.langevin.sample_langevin_post_eps_with_flow(eps0, target.to(dev), netG, net, noise=False, **kw)
    finally:
        F.set_small_batch_max(prev)
    assert len(calls) == STEPS
    own = R.rel_l2(e32, e64)
    assert R.rel_l2(e3.cpu(), e64) <= max(2e-5, 3.0 * own)
    # an empty batch comes back as it is, without a launch; no step: no norms
    e0, z0, gg0, gf0 = lsnf.langevin.sample_langevin_post_eps_with_flow(eps0[:0], target.to(dev)[:0], netG, net, **kw)
    assert e0.shape == (0, nz) and z0.shape == (0, nz, 1, 1) and gg0 is None and gf0 is None
    en, _, ggn, gfn = lsnf.langevin.sample_langevin_post_eps_with_flow(eps0, target.to(dev), netG, net, **dict(kw, g_l_steps=0))
    assert torch.equal(en, eps0) and ggn is None and gfn is None
    # philox noise: step k draws the in-kernel stream at offset + k; one step with and without it gives the draw itself
    ph = F.PhiloxNoise(1234, 40, 0)
    one = dict(kw, g_l_steps=1)
    e_noise, _, _, _ = lsnf.langevin.sample_langevin_post_eps_with_flow(eps0, target.to(dev), netG, net, philox=ph, **one)
    e_plain, _, _, _ = lsnf.langevin.sample_langevin_post_eps_with_flow(eps0, target.to(dev), netG, net, noise=False, **one)
    assert ph.offset == 41
    draw = (e_noise - e_plain) / STEP_SIZE
    ref = torch.from_numpy(langevin_noise(B, nz, 1234, 40, 0)).to(dev)
    # (v_log_f32 / v_sin_f32 / v_cos_f32 against float64 libm and the subtraction above: the bound tests/test_gpu_langevin.py holds)
    assert (draw.double() - ref).abs().max().item() <= 1e-4


# ---------------------------------------------------------------------------------------------
# 8. graph capture
# ---------------------------------------------------------------------------------------------
def test_reverse_keep_and_its_backward_are_graph_capturable(lsnf, gpu_device):
    c = case(*C1, 100)
    dev, F = gpu_device, lsnf.flow
    plan = make_plan(lsnf, c, dev)
    B, nz = c.B, c.nz
    eps, gx, go = torch.empty(B, nz, device=dev), torch.empty(B, nz, device=dev), torch.empty(B, device=dev)
    out = (torch.empty_like(eps), torch.empty(B, device=dev))
    act = F.new_act_saved(plan, B, dev)
    res = torch.empty_like(eps)
    held = []

    def run():
        _, _, saved = F.reverse(plan, eps, None, out=out, save_for_backward=True, act_saved=act)
        held.append(saved)
        F.reverse_backward_z(plan, eps, saved, act, gx, go, out=res)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up on a side stream (lazy module load etc.)
        eps.copy_(c.eps.to(dev)); gx.normal_(); go.normal_()
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # one linear capture on one stream
        run()
    for seed in (2, 3):                                # two replays with new inputs
        a, b, _ = seeded(B, nz, seed)
        gx.copy_(a.to(dev)); go.copy_(b.to(dev)); eps.mul_(0.5)
        graph.replay()
        torch.cuda.synchronize()
        got, x_got = res.clone(), out[0].clone()
        act_e = F.new_act_saved(plan, B, dev)
        x_e, _, saved_e = F.reverse(plan, eps, None, save_for_backward=True, act_saved=act_e)
        assert torch.equal(x_got, x_e) and torch.equal(got, F.reverse_backward_z(plan, eps, saved_e, act_e, gx, go))

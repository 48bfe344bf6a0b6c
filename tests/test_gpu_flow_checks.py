"""GPU: the argument checks of flow.py.  The C ABI takes bare pointers, so a tensor of the wrong size, dtype, stride or device
must be refused in Python, before an entry point that launches is entered.

Geometry nz 8, width 4, depth 2, affine coupling, B = 5: the smallest stack in which z_saved exists, a half-row (4 floats) is
shorter than a vector load and B is no multiple of any tile.  Every malformed argument is malformed by METADATA only (a slice, a
dtype, a CPU tensor) and never reaches a kernel; everything that is launched here is well formed."""
import math
import types

import pytest
import torch

from oracle import flow_oracle as O
from counting_lib import install

pytestmark = pytest.mark.gpu

NZ, W, D, C, B = 8, 4, 2, 1, 5
NAN = float("nan")


@pytest.fixture(scope="module")
def ctx(gpu_device):
    """One well-formed evaluation, computed once and left unchanged: parameters, plan, a batch, the forward's outputs and stash,
    upstream gradients -- and a plan of the same geometry whose buffers live on the CPU."""
    import lsnf_amd
    lsnf_amd.load_library()
    F, dev = lsnf_amd.flow, gpu_device
    c = types.SimpleNamespace(lsnf=lsnf_amd, F=F, dev=dev)
    c.params = F.params_from_state_dict(O.init_params(NZ, W, D, seed=4), D, dev)
    c.plan = F.prepare(c.params, NZ, W, D, C)
    gen = torch.Generator().manual_seed(9)
    c.z, c.gz1, c.gld, c.noise = (torch.randn(*s, generator=gen).to(dev) for s in ((B, NZ), (B, NZ), (B,), (B, NZ)))
    c.gz1_t = torch.randn(NZ, B, generator=gen).to(dev).t()               # (B, nz), not contiguous
    c.act, c.ws = F.new_act_saved(c.plan, B, dev), F.new_params_workspace(c.plan, B, dev)
    c.fast = F.params_fast_path()
    c.z1, c.ld, c.ll, c.saved = F.forward(c.plan, c.z, save_for_backward=True, act_saved=c.act, params_ws=c.ws if c.fast else None)
    c.ws_need = lsnf_amd.load_library().lsnf_backward_params_workspace_floats(NZ, W, D, B)
    assert c.saved.shape == (D - 1, B, NZ) and c.ws_need > 8 and c.act.numel() >= 2
    c.cpu_plan = F.FlowPlan(NZ, W, D, C, c.plan.buf.cpu(), c.plan.scratch.cpu())
    torch.cuda.synchronize()
    return c


def nan(*shape, dev):
    return torch.full(shape, NAN, device=dev)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
# Each case: (wrapper, the argument the message must name, build(c) -> (call, caller-owned outputs pre-filled with NaN)).
def _z_side(c, kw):
    """Arguments of backward_z / backward_params, well formed, with `kw` laid over them."""
    a = dict(plan=c.plan, z_in=c.z, z_out=c.z1, z_saved=c.saved, g_z1=c.gz1, g_logdet=c.gld, act_saved=c.act)
    a.update(kw(c))
    return a


def _backward_z(kw):
    def build(c):
        a = _z_side(c, kw)
        return (lambda: c.F.backward_z(a["plan"], a["z_out"], a["z_saved"], a["g_z1"], a["g_logdet"], act_saved=a["act_saved"])), []
    return build


def _backward_params(kw):
    def build(c):
        a = dict(_z_side(c, lambda c: {}), params=c.params, workspace=torch.full_like(c.ws, NAN))
        a.update(kw(c))
        return (lambda: c.F.backward_params(a["plan"], a["params"], a["z_in"], a["z_out"], a["z_saved"], a["g_z1"], a["g_logdet"],
                                            act_saved=a["act_saved"], workspace=a["workspace"])), [a["workspace"]]
    return build


Z_SIDE = [      # the holes the z-side arguments of backward_z and backward_params shared
    ("z_out-of-nz+2-columns", "z_out", lambda c: dict(z_out=torch.empty(B, NZ + 2, device=c.dev))),
    ("z_saved-one-row-short", "z_saved", lambda c: dict(z_saved=c.saved.view(-1)[: (B - 1) * NZ])),
    ("z_saved-None-at-depth-2", "z_saved", lambda c: dict(z_saved=None)),
    ("g_z1-of-B-1-rows", "g_z1", lambda c: dict(g_z1=c.gz1[: B - 1])),
    ("g_logdet-of-B-1-elements", "g_logdet", lambda c: dict(g_logdet=c.gld[: B - 1])),
    ("act_saved-sliced-to-half", "act_saved", lambda c: dict(act_saved=c.act[: c.act.numel() // 2])),
    ("g_z1-float64", "g_z1", lambda c: dict(g_z1=c.gz1.double())),
    ("g_z1-transposed", "g_z1", lambda c: dict(g_z1=c.gz1_t)),
    ("plan-on-the-cpu", "plan", lambda c: dict(plan=c.cpu_plan)),
]


def _params_with(i, change):
    return lambda c: dict(params=[change(p) if j == i else p for j, p in enumerate(c.params)])


def _langevin_offset_dev_on_cpu(c):
    rng = c.F.PhiloxNoise(5, offset_dev=torch.zeros(1, dtype=torch.int64))
    z = c.z.clone()
    return (lambda: c.F.langevin_step(c.plan, z, None, rng, 0.1)), []


def _prepare_into(make_plan, depth=D):
    def build(c):
        plan = make_plan(c)
        plan.buf.fill_(NAN)
        plan.scratch.fill_(NAN)
        return (lambda: c.F.prepare(c.params, NZ, W, depth, C, plan=plan)), [plan.buf, plan.scratch]
    return build


def _short_plan(c):
    p = c.F.alloc_plan(NZ, W, D, C, c.dev)
    return c.F.FlowPlan(NZ, W, D, C, p.buf[: p.buf.numel() - 4], p.scratch)


def _forward(plan_of, **kw):
    def build(c):
        out = (nan(B, NZ, dev=c.dev), nan(B, dev=c.dev), nan(B, dev=c.dev))
        more = {k: v(c) for k, v in kw.items()}
        return (lambda: c.F.forward(plan_of(c), c.z, out=out, **more)), list(out)
    return build


def _reverse(plan_of, rows=B):
    def build(c):
        out = (nan(rows, NZ, dev=c.dev), nan(B, dev=c.dev))
        return (lambda: c.F.reverse(plan_of(c), c.z, out=out)), list(out)
    return build


def _reverse_backward_z(plan_of, with_act=True):
    def build(c):
        out = nan(B, NZ, dev=c.dev)
        return (lambda: c.F.reverse_backward_z(plan_of(c), c.z1, c.saved, c.act if with_act else None, c.gz1, c.gld, out=out)), [out]
    return build


def _reverse_langevin(plan_of, grad_rows=B):
    def build(c):
        out = (nan(B, NZ, dev=c.dev), nan(B, NZ, dev=c.dev), nan(B, dev=c.dev), nan(B, dev=c.dev))
        return (lambda: c.F.reverse_langevin_step(plan_of(c), c.z1, c.saved, c.act, c.gz1[:grad_rows], c.noise, 0.1, out=out)), list(out)
    return build


def _gpu(c):
    return c.plan


def _cpu(c):
    return c.cpu_plan


REFUSALS = (
    [("backward_z", arg, _backward_z(kw), i) for i, arg, kw in Z_SIDE]
    + [("backward_params", arg, _backward_params(kw), i) for i, arg, kw in Z_SIDE]
    + [("backward_params", "z_in", _backward_params(lambda c: dict(z_in=c.z[: B - 1])), "z_in-of-another-B"),
       ("backward_params", r"param\[3\] \(f\.fc_1\.w\)", _backward_params(_params_with(3, lambda p: p[:-1])), "fc_1.w-one-row-fewer"),
       ("backward_params", r"param\[5\]", _backward_params(_params_with(5, lambda p: p.cpu())), "one-parameter-on-the-cpu"),
       ("backward_params", "workspace", _backward_params(lambda c: dict(workspace=torch.full_like(c.ws, NAN)[: c.ws_need - 8])),
        "workspace-eight-floats-short"),
       ("langevin_step", "offset_dev", _langevin_offset_dev_on_cpu, "offset_dev-on-the-cpu"),
       ("prepare", "plan", _prepare_into(lambda c: c.F.alloc_plan(NZ, W, D + 1, C, c.dev)), "plan-of-another-depth"),
       ("prepare", "plan.buf", _prepare_into(_short_plan), "plan-buf-sliced-short"),
       ("forward", "plan", _forward(_cpu), "plan-on-the-cpu"),
       ("forward", "stats", _forward(_gpu, stats=lambda c: torch.zeros(8, dtype=torch.float64, device=c.dev)), "stats-of-8-doubles"),
       ("reverse", "plan", _reverse(_cpu), "plan-on-the-cpu"),
       ("reverse", "z_out", _reverse(_gpu, rows=B - 1), "z_out-of-B-1-rows"),
       ("reverse_backward_z", "plan", _reverse_backward_z(_cpu), "plan-on-the-cpu"),
       ("reverse_backward_z", "act_saved", _reverse_backward_z(_gpu, with_act=False), "act_saved-None"),
       ("reverse_langevin_step", "plan", _reverse_langevin(_cpu), "plan-on-the-cpu"),
       ("reverse_langevin_step", "grad_g", _reverse_langevin(_gpu, grad_rows=B - 1), "grad_g-of-B-1-rows")])


@pytest.mark.parametrize("wrapper,arg,build,case", REFUSALS, ids=[f"{r[0]}-{r[3]}" for r in REFUSALS])
def test_malformed_argument_is_refused_before_any_launch(ctx, monkeypatch, wrapper, arg, build, case):
    call, outputs = build(ctx)
    torch.cuda.synchronize()
    stand = install(monkeypatch, ctx.lsnf)
    with pytest.raises(ctx.lsnf.LsnfError, match=arg):
        call()
    assert stand.launching() == [], dict(stand.entered)
    torch.cuda.synchronize()
    for t in outputs:
        assert bool(torch.isnan(t).all())


# ---- non-refusals ------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _larger(t, extra=24):
    """The same leading contents in a flat buffer `extra` floats longer than needed."""
    return torch.cat([t.reshape(-1), torch.full((extra,), 3.0, device=t.device)])


def test_larger_stash_buffers_give_the_bits_of_the_exact_size_call(ctx):
    c, F = ctx, ctx.F
    saved, act, ws = _larger(c.saved), _larger(c.act), _larger(c.ws)
    assert saved.numel() > (D - 1) * B * NZ and act.numel() > c.act.numel() and ws.numel() > c.ws.numel()
    assert _same(F.backward_z(c.plan, c.z1, saved, c.gz1, c.gld, act_saved=act), F.backward_z(c.plan, c.z1, c.saved, c.gz1, c.gld, act_saved=c.act))
    assert _same(F.backward_z(c.plan, c.z1, saved, ll_scale=-1.0), F.backward_z(c.plan, c.z1, c.saved, ll_scale=-1.0))
    assert _same(F.reverse_backward_z(c.plan, c.z1, saved, act, c.gz1, c.gld), F.reverse_backward_z(c.plan, c.z1, c.saved, c.act, c.gz1, c.gld))
    big = F.reverse_langevin_step(c.plan, c.z1, saved, act, c.gz1, c.noise, 0.1, want_g=True)
    exact = F.reverse_langevin_step(c.plan, c.z1, c.saved, c.act, c.gz1, c.noise, 0.1, want_g=True)
    assert all(_same(a, b) for a, b in zip(big, exact))
    stash = dict(act_saved=act, workspace=ws) if c.fast else {}
    exact_stash = dict(act_saved=c.act, workspace=c.ws) if c.fast else {}
    g_big = [g.clone() for g in F.backward_params(c.plan, c.params, c.z, c.z1, saved, ll_scale=-1.0 / B, **stash)]
    g_exact = F.backward_params(c.plan, c.params, c.z, c.z1, c.saved, ll_scale=-1.0 / B, **exact_stash)
    assert all(_same(a, b) for a, b in zip(g_big, g_exact)) and all(bool(torch.isfinite(g).all()) for g in g_exact)
    # a stash larger than needed is filled like the exact one (the buffers a kernel writes are held to "at least" as well)
    act2, saved2 = torch.zeros_like(act), torch.zeros_like(saved)
    z1, ld, ll, _ = F.forward(c.plan, c.z, act_saved=act2, z_saved_out=saved2)
    assert _same(z1, c.z1) and _same(saved2[: c.saved.numel()], c.saved.view(-1))
    assert _same(F.backward_z(c.plan, z1, saved2, ll_scale=-1.0, act_saved=act2), F.backward_z(c.plan, c.z1, c.saved, ll_scale=-1.0, act_saved=c.act))


def test_an_empty_batch_passes_every_wrapper(ctx, monkeypatch):
    """B == 0 is not an error: empty results, nothing launched (the library returns before its first launch).  The two wrappers
    whose entry point has always refused an empty batch still refuse it, by that entry point's message."""
    c, F, dev = ctx, ctx.F, ctx.dev
    z0, v0 = torch.empty(0, NZ, device=dev), torch.empty(0, device=dev)
    act0 = F.new_act_saved(c.plan, 0, dev)
    rng = F.PhiloxNoise(1)
    z1, ld, ll, saved = F.forward(c.plan, z0, v0, save_for_backward=True, act_saved=act0)
    assert z1.shape == (0, NZ) and ld.shape == ll.shape == (0,) and saved.shape == (D - 1, 0, NZ)
    F.BoundForward(c.plan, z0, (z1, ld, ll))(None)
    x, obj = F.reverse(c.plan, z0, v0)
    assert x.shape == (0, NZ) and obj.shape == (0,)
    for z_saved in (saved, None):
        assert F.backward_z(c.plan, z0, z_saved, ll_scale=-1.0).shape == (0, NZ)
        assert F.backward_z(c.plan, z0, z_saved, z0, v0, act_saved=act0).shape == (0, NZ)
        assert F.reverse_backward_z(c.plan, z0, z_saved, act0, z0, v0).shape == (0, NZ)
        assert F.reverse_langevin_step(c.plan, z0, z_saved, act0, z0, rng, 0.1)[0].shape == (0, NZ)
    assert [None if t is None else tuple(t.shape) for t in F.sample(c.plan, 0, rng, want_eps=True, want_ll=True)] == [(0, NZ), (0,), (0, NZ), (0,)]
    for reuse in (False, True):
        z_new, ll, gf, gg = F.langevin_step(c.plan, z0, z0, rng, 0.1, reuse_buffers=reuse)
        assert z_new.shape == (0, NZ) and ll.shape == gf.shape == gg.shape == (0,)
    with pytest.raises(c.lsnf.LsnfError, match="B=0 out of range"):
        F.backward_params(c.plan, c.params, z0, z0, saved, ll_scale=-1.0)
    with pytest.raises(c.lsnf.LsnfError, match="non-empty batch"):
        F.actnorm_init([p.clone() for p in c.params], z0, NZ, W, D, C)
    torch.cuda.synchronize()


def test_two_batch_sizes_interleaved_on_one_stream_give_the_bits_of_fresh_plans(ctx):
    """backward_z(act_saved=None) keeps its rebuilt stash, and langevin_step(reuse_buffers=True) its intermediates, on the plan --
    one set per stream, one batch size at a time: switching sizes back and forth must evict and rebuild, never reuse a buffer of
    the other size."""
    c, F, dev = ctx, ctx.F, ctx.dev
    batches = {n: torch.randn(n, NZ, generator=torch.Generator().manual_seed(n)).to(dev) for n in (B, 3)}
    rng = F.PhiloxNoise(11, offset=2)

    def evaluate(plan, z):
        z1, _, _, saved = F.forward(plan, z, save_for_backward=True)
        g = F.backward_z(plan, z1, saved, ll_scale=-1.0)
        z_new, ll, gf, _ = F.langevin_step(plan, z, None, rng, 0.1, reuse_buffers=True)
        return g, z_new, ll.clone(), gf.clone()

    fresh = {n: evaluate(F.prepare(c.params, NZ, W, D, C), z) for n, z in batches.items()}
    shared = F.prepare(c.params, NZ, W, D, C)
    for n in (B, 3, B, B, 3):
        got = evaluate(shared, batches[n])
        assert all(_same(a, b) for a, b in zip(got, fresh[n])), n
        assert all(bool(torch.isfinite(t).all()) for t in got)
        for attr in ("_restash_buffers", "_langevin_buffers"):
            keys = list(shared.__dict__.get(attr, {}))
            assert len(keys) <= 1 and all(k[0] == n for k in keys), (attr, keys)
    assert not math.isnan(float(fresh[B][2].sum()))

"""GPU: `lsnf_backward_params_det` -- the parameter gradients with every sum over the batch in a fixed order.  At the smallest
shapes that reach each contraction kernel and each form of the dump, on the fast path and on the recomputing path: repeated
calls give the same bits in all depth*12 tensors and in dL/dz_in; the values are held to the float64 oracle and to the default
path by the project's TOL / TOL_GZ; the bits do not depend on the stream or on being replayed from a captured graph; two modules
with `deterministic_grads` train to the same bits; a default-size workspace is refused.  Last: the kept buffers of
`reuse_buffers` are keyed by who owns the workspace.

Helpers, batches (`oracle.smooth_batch`) and tolerances are those of tests/test_gpu_param_grads_oracle.py."""
import types

import pytest
import torch

from oracle import flow_oracle as O
from test_gpu_param_grads_oracle import KEYS_PER_BLOCK, TOL, TOL_GZ, _rel, _setup

pytestmark = pytest.mark.gpu

RUNS = 5
MODES = {"BF16X3": "MATH_BF16X3", "FP16X2": "MATH_FP16X2", "FP32": "MATH_FP32"}
# (nz, width, depth, coupling, B, math mode, small-batch setting: None = automatic, else rows)
CASES = [(128, 64, 5, 1, 100, "BF16X3", None),        # one chunk; G from several workgroups
         (128, 64, 5, 1, 1500, "BF16X3", None),       # plain kernel, several chunks
         (128, 64, 5, 1, 5000, "BF16X3", None),       # LDS x4
         (100, 64, 5, 1, 4500, "BF16X3", None),       # LDS x2
         (50, 33, 5, 1, 4100, "BF16X3", None),        # LDS x1
         (128, 64, 5, 1, 14000, "BF16X3", None),      # x3, row-major dumps
         (128, 64, 5, 1, 12289, "BF16X3", 0),         # x3, tiled dumps, ragged tile
         (128, 64, 1, 1, 12289, "BF16X3", 0),         # no z_saved
         (128, 64, 5, 0, 5000, "BF16X3", None),       # additive coupling
         (128, 64, 5, 1, 5000, "FP16X2", None),       # fp16x2
         (128, 64, 5, 1, 5000, "FP32", None)]         # the recomputing path is the only one


def _case_id(c):
    nz, width, depth, coupling, B, mode, small = c
    return (f"nz{nz}-w{width}-d{depth}-{'affine' if coupling else 'additive'}-B{B}-{mode}"
            + ("" if small is None else f"-small{small}"))


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    assert tuple(lsnf_amd.flow.BLOCK_PARAM_KEYS) == KEYS_PER_BLOCK
    return lsnf_amd


def _nan_buffers(F, plan, B, dev, deterministic):
    act = F.new_act_saved(plan, B, dev)
    act.fill_(float("nan"))
    ws = F.new_params_workspace(plan, B, dev, deterministic=deterministic)
    ws.fill_(float("nan"))
    return act, ws


def _one_call(F, plan, params, z, B, dev, fast, deterministic, bufs=None):
    """One evaluation: the forward (with the stash and the h dump on the fast path, into NaN-filled buffers) and the parameter
    gradients; returns clones of (the depth*12 gradients, dL/dz_in)."""
    if fast:
        act, ws = bufs if bufs is not None else _nan_buffers(F, plan, B, dev, deterministic)
        act.fill_(float("nan"))
        ws.fill_(float("nan"))
        z1, _, _, saved = F.forward(plan, z, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
        grads, gz = F.backward_params(plan, params, z, z1, saved, ll_scale=-1.0 / B, want_grad_z=True, act_saved=act, workspace=ws,
                                      deterministic=deterministic)
    else:
        z1, _, _, saved = F.forward(plan, z, want_ll=False, save_for_backward=True)
        if deterministic:
            # A caller-owned workspace is a fast-path argument; on this path the wrapper owns it.  With reuse_buffers it is kept on
            # the plan: the first call allocates it, and it is filled with NaN before every call that counts, so that a slot element
            # no workgroup wrote cannot find an earlier run's value.
            kw = dict(ll_scale=-1.0 / B, want_grad_z=True, reuse_buffers=True, deterministic=True)
            st = plan.__dict__.get("_bp_state")
            if st is None or st["ws"].numel() < F._det_floats(plan, B):
                F.backward_params(plan, params, z, z1, saved, **kw)
                st = plan.__dict__["_bp_state"]
            assert st["ws"].numel() >= F._det_floats(plan, B) > 0
            st["ws"].fill_(float("nan"))
            grads, gz = F.backward_params(plan, params, z, z1, saved, **kw)
            assert plan.__dict__["_bp_state"] is st                  # the call used the poisoned workspace
        else:
            grads, gz = F.backward_params(plan, params, z, z1, saved, ll_scale=-1.0 / B, want_grad_z=True)
    return [g.clone() for g in grads], gz.clone()


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("nz,width,depth,coupling,B,mode,small", CASES, ids=[_case_id(c) for c in CASES])
def test_deterministic_gradients_repeat_bit_for_bit_and_match_float64(lsnf, gpu_device, nz, width, depth, coupling, B, mode, small):
    """Five deterministic calls on the same inputs are `torch.equal` in all depth*12 tensors and in g_z_in (workspace refilled
    with NaN, on the fast path the forward rerun, between calls); every tensor is within TOL of the float64 oracle and of the
    default path, g_z_in within TOL_GZ of the oracle.  Reported, not asserted: whether five default-path runs differed."""
    F, params, plan, z, n_replaced, refs, gz_ref, keys = _setup(lsnf, gpu_device, nz, width, depth, coupling, B)
    prev_small = F.set_small_batch_max(F.SMALL_BATCH_AUTO if small is None else small)
    prev_mode = F.set_math_mode(getattr(F, MODES[mode]))
    try:
        paths = ("fast", "recompute") if F.params_fast_path() else ("recompute",)
        assert ("fast" in paths) == (mode != "FP32")
        det, default = {}, {}
        for path in paths:
            bufs = _nan_buffers(F, plan, B, gpu_device, True) if path == "fast" else None
            det[path] = [_one_call(F, plan, params, z, B, gpu_device, path == "fast", True, bufs) for _ in range(RUNS)]
            # (the default call takes the deterministic workspace too: the header says it is valid for both)
            default[path] = [_one_call(F, plan, params, z, B, gpu_device, path == "fast", False, bufs) for _ in range(RUNS)]
        torch.cuda.synchronize()
    finally:
        F.set_small_batch_max(prev_small)
        F.set_math_mode(prev_mode)
    report, bad = [], []
    for path in paths:
        runs = det[path]
        differing = [i for i in range(1, RUNS) if not _same_bits(runs[0], runs[i])]
        default_moved = any(not _same_bits(default[path][0], default[path][i]) for i in range(1, RUNS))
        grads, gz = runs[0]
        assert len(grads) == len(refs) == depth * 12
        worst = {"det_vs_f64": 0.0, "det_vs_default": 0.0}
        for k, a, d, r in zip(keys, grads, default[path][0][0], refs):
            assert torch.isfinite(a).all(), (path, k)
            errs = {"det_vs_f64": _rel(a, r.reshape(a.shape)), "det_vs_default": _rel(a, d)}
            for what, e in errs.items():
                worst[what] = max(worst[what], e)
                if not e <= TOL:
                    bad.append((path, what, k, e))
        e_gz = _rel(gz, gz_ref)
        report.append(f"{path}: det_runs_differing={differing} default_runs_differed={default_moved} "
                      + " ".join(f"{w}={e:.2e}" for w, e in worst.items()) + f" gz={e_gz:.2e}")
        if differing:
            bad.append((path, "bits", differing))
        if not e_gz <= TOL_GZ:
            bad.append((path, "gz", e_gz))
    print(f"\n[param-grads-det] {_case_id((nz, width, depth, coupling, B, mode, small))} rows_replaced={n_replaced} " + " | ".join(report))
    assert not bad, bad[:8]


def _synthetic(lsnf, dev, nz, width, depth, B):
    """Oracle-free inputs: seeded weights and a seeded N(0,1) batch."""
    F = lsnf.flow
    p = O.init_params(nz, width, depth, seed=3)
    params = F.params_from_state_dict(p, depth, dev)
    plan = F.prepare(params, nz, width, depth, 1)
    z = torch.randn(B, nz, generator=torch.Generator().manual_seed(B)).to(dev)
    return F, p, params, plan, z


def test_full_size_repeats_bit_for_bit_and_stays_on_the_default_path(lsnf, gpu_device):
    """(128, 64, 5, affine, 65 536 rows, bf16x3): three deterministic runs per path are bit-equal and each tensor is within TOL of
    the default path, which tests/test_gpu_param_grads_oracle.py holds to float64 at this size."""
    nz, width, depth, B = 128, 64, 5, 65536
    F, _, params, plan, z = _synthetic(lsnf, gpu_device, nz, width, depth, B)
    prev_small = F.set_small_batch_max(F.SMALL_BATCH_AUTO)
    prev_mode = F.set_math_mode(F.MATH_BF16X3)
    try:
        res = {}
        for path in ("fast", "recompute"):
            bufs = _nan_buffers(F, plan, B, gpu_device, True) if path == "fast" else None
            runs = [_one_call(F, plan, params, z, B, gpu_device, path == "fast", True, bufs) for _ in range(3)]
            res[path] = (runs, _one_call(F, plan, params, z, B, gpu_device, path == "fast", False, bufs))
        torch.cuda.synchronize()
    finally:
        F.set_small_batch_max(prev_small)
        F.set_math_mode(prev_mode)
    for path, (runs, default) in res.items():
        assert _same_bits(runs[0], runs[1]) and _same_bits(runs[0], runs[2]), path
        worst = max(_rel(a, d) for a, d in zip(runs[0][0], default[0]))
        print(f"\n[param-grads-det] B={B} {path}: three runs bit-equal, worst rel-L2 to the default path {worst:.2e}")
        assert all(torch.isfinite(a).all() for a in runs[0][0])
        assert worst <= TOL, (path, worst)
        assert torch.equal(runs[0][1], default[1])          # g_z_in comes from the same backward kernel: the same rows


def test_bits_do_not_depend_on_the_stream_or_on_graph_replay(lsnf, gpu_device):
    """(128, 64, 5, affine, 5 000 rows, bf16x3), fast path: the call on a side stream, and two replays of a `torch.cuda.graph`
    holding the call, give the eager bits of the default stream."""
    nz, width, depth, B = 128, 64, 5, 5000
    F, _, params, plan, z = _synthetic(lsnf, gpu_device, nz, width, depth, B)
    prev_small = F.set_small_batch_max(F.SMALL_BATCH_AUTO)
    prev_mode = F.set_math_mode(F.MATH_BF16X3)
    try:
        act, ws = _nan_buffers(F, plan, B, gpu_device, True)
        z1, _, _, saved = F.forward(plan, z, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
        kw = dict(ll_scale=-1.0 / B, want_grad_z=True, act_saved=act, workspace=ws, deterministic=True)
        grads, gz = F.backward_params(plan, params, z, z1, saved, **kw)
        eager = ([g.clone() for g in grads], gz.clone())
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=gpu_device)
        with torch.cuda.stream(side):
            grads, gz = F.backward_params(plan, params, z, z1, saved, **kw)
            on_side = ([g.clone() for g in grads], gz.clone())
        side.synchronize()
        # the graph: buffers kept on the plan (reuse_buffers), so that replays write the tensors the capture returned
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            F.backward_params(plan, params, z, z1, saved, reuse_buffers=True, **kw)           # warm-up: allocates the kept buffers
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                grads, gz = F.backward_params(plan, params, z, z1, saved, reuse_buffers=True, **kw)
        replays = []
        for _ in range(2):
            for g in grads:
                g.fill_(float("nan"))
            gz.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            replays.append(([g.clone() for g in grads], gz.clone()))
    finally:
        plan.__dict__.pop("_bp_state", None)
        F.set_small_batch_max(prev_small)
        F.set_math_mode(prev_mode)
    assert all(torch.isfinite(g).all() for g in eager[0])
    assert _same_bits(eager, on_side), "side stream"
    assert _same_bits(eager, replays[0]) and _same_bits(eager, replays[1]), "graph replay"


HYPER = dict(lr=1e-3, betas=(0.5, 0.999), weight_decay=1e-2, max_norm=0.5)      # tests/test_gpu_flow_adam.py's module-level setup


def _train(lsnf, dev, p, z, deterministic, steps=3):
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=5, f_flow_permutation=2, f_width=64, f_flow_coupling=1)
    net = lsnf._netF(hps, nz=128)
    net.load_state_dict(p, strict=True)
    net = net.to(dev)
    assert net.deterministic_grads is False
    net.deterministic_grads = deterministic
    opt = lsnf.FlowAdam(net, **HYPER)
    losses, first_grads = [], None
    for _ in range(steps):
        losses.append(net.mle_step(z, opt))
        if first_grads is None:
            first_grads = [q.grad.detach().clone() for q in net._param_list()]
    torch.cuda.synchronize()
    return net, opt, [l.item() for l in losses], first_grads


def test_two_modules_with_deterministic_grads_train_to_the_same_bits(lsnf, gpu_device):
    """B = 5 000: two fresh `_netF` with `deterministic_grads = True`, one seed, 3 `mle_step`s with a clipping `FlowAdam`: equal
    `state_dict`s and optimizer states, bit for bit.  The same run with the attribute off walks the same path: every step's
    loss within 1e-5 relative (the bound tests/test_gpu_flow_adam.py puts on two modules' losses) and the first step's gradients
    -- same weights, same batch -- within TOL per tensor.  (Later parameters are not compared across the two summation orders:
    Adam's normalised update turns a last-bit difference of a near-zero gradient into a difference of order lr.)"""
    B = 5000
    p = O.init_params(128, 64, 5, seed=3)
    z = torch.randn(B, 128, generator=torch.Generator().manual_seed(9)).to(gpu_device)
    prev_mode = lsnf.flow.set_math_mode(lsnf.flow.MATH_BF16X3)
    prev_small = lsnf.flow.set_small_batch_max(lsnf.flow.SMALL_BATCH_AUTO)
    try:
        a_net, a_opt, a_loss, a_g = _train(lsnf, gpu_device, p, z, True)
        b_net, b_opt, b_loss, b_g = _train(lsnf, gpu_device, p, z, True)
        c_net, c_opt, c_loss, c_g = _train(lsnf, gpu_device, p, z, False)
    finally:
        lsnf.flow.set_small_batch_max(prev_small)
        lsnf.flow.set_math_mode(prev_mode)
    sa, sb = a_net.state_dict(), b_net.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert any(not torch.equal(sa[k].cpu(), p[k]) for k in sa)                  # (the steps did move the weights)
    oa, ob = a_opt.state_dict()["state"], b_opt.state_dict()["state"]
    assert sorted(oa) == sorted(ob) and len(oa) == 60
    for i in oa:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(oa[i][k], ob[i][k]), (i, k)
    # the whole device state, header (int64 counters, float64 norm partials) included: compared as bits, not as floats
    assert torch.equal(a_opt._flat.view(torch.int32), b_opt._flat.view(torch.int32))
    assert a_loss == b_loss
    assert a_loss[2] < a_loss[0]
    for x, y in zip(a_loss, c_loss):
        assert abs(x - y) <= 1e-5 * abs(y), (a_loss, c_loss)
    worst = max(_rel(g, h) for g, h in zip(a_g, c_g))
    print(f"\n[param-grads-det] mle_step x3 at B={B}: losses {a_loss} (default path {c_loss}), first-step gradients vs default {worst:.2e}")
    assert worst <= TOL


def test_default_size_workspace_is_refused_before_any_launch(lsnf, gpu_device, monkeypatch):
    from counting_lib import QUERIES, install
    nz, width, depth, B = 128, 64, 5, 100
    F, _, params, plan, z = _synthetic(lsnf, gpu_device, nz, width, depth, B)
    act = F.new_act_saved(plan, B, gpu_device)
    ws = F.new_params_workspace(plan, B, gpu_device)
    z1, _, _, saved = F.forward(plan, z, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
    torch.cuda.synchronize()
    stand = install(monkeypatch, lsnf)
    with pytest.raises(lsnf.LsnfError, match="workspace"):
        F.backward_params(plan, params, z, z1, saved, ll_scale=-1.0 / B, act_saved=act, workspace=ws, deterministic=True)
    assert set(stand.entered) <= set(QUERIES) | {"lsnf_backward_params_det_workspace_floats"}, dict(stand.entered)
    big = F.new_params_workspace(plan, B, gpu_device, deterministic=True)
    assert big.numel() > ws.numel()
    F.backward_params(plan, params, z, z1, saved, ll_scale=-1.0 / B, act_saved=act, workspace=ws)       # the default call takes it as before
    torch.cuda.synchronize()


def test_kept_buffers_do_not_hand_an_empty_workspace_to_a_call_without_one(lsnf, gpu_device):
    """`reuse_buffers=True` keeps one set of buffers per plan.  A call with a caller-owned workspace keeps none of its own; the next
    call WITHOUT one (same parameters, batch and stream) used to find that empty one and fail with "NULL argument".  Default
    path, then the deterministic one; each recomputing result equals the call that keeps nothing."""
    nz, width, depth, B = 128, 64, 5, 100
    F, _, params, plan, z = _synthetic(lsnf, gpu_device, nz, width, depth, B)
    prev_mode = F.set_math_mode(F.MATH_BF16X3)
    try:
        for det in (False, True):
            act, ws = _nan_buffers(F, plan, B, gpu_device, det)
            z1, _, _, saved = F.forward(plan, z, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
            kw = dict(ll_scale=-1.0 / B, deterministic=det)
            F.backward_params(plan, params, z, z1, saved, reuse_buffers=True, act_saved=act, workspace=ws, **kw)
            kept = [g.clone() for g in F.backward_params(plan, params, z, z1, saved, reuse_buffers=True, **kw)]
            fresh = F.backward_params(plan, params, z, z1, saved, **kw)
            torch.cuda.synchronize()
            assert all(torch.isfinite(g).all() for g in kept)
            if det:
                assert all(torch.equal(a, b) for a, b in zip(kept, fresh))
            else:       # (one workgroup per task at 100 rows, but G is summed with atomics: values, not bits)
                assert max(_rel(a, b) for a, b in zip(kept, fresh)) <= TOL
    finally:
        plan.__dict__.pop("_bp_state", None)
        F.set_math_mode(prev_mode)

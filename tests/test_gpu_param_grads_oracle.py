"""GPU: `lsnf_backward_params` -- the fast path (forward with the activation stash and the h dump, backward from the stash,
batch contraction) and the recomputing path -- against the float64 oracle on WHOLE batches, at every batch size, geometry
and arithmetic mode where the kernels of that chain change: the plain, LDS-staged (row vectors of 4 / 2 / 1) and bf16-pipe
contractions; the row-major and the tiled h / g dumps (f_width 64, 48 and 128, a ragged last tile, just above
LSNF_X3_MIN_ROWS); depth 1 (no z_saved) and 16; additive coupling; the phase-separated and fp16x2 forwards.

Batches come from `oracle.smooth_batch`: seeded N(0,1) rows with every row that sits within 2e-5 of a ReLU kink redrawn,
so the batch keeps its size (hence its kernels) and the fp32 gradient of every row is well defined.  On such batches an fp32
restatement of the flow agrees with the fp64 one to ~1e-6 per tensor, so 2e-5 arbitrates: a dropped or duplicated 32-row
stage of the contraction moves a tensor by ~32 / B of its norm (5e-4 at 65 536 rows), 25x the bound."""
import functools
import os
import subprocess
import sys
import types

import pytest
import torch

from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu

TOL = 2e-5          # relative L2 per tensor: fast path vs fp64, recomputing path vs fp64, fast vs recomputing
TOL_GZ = 1e-5       # relative L2 over the batch: dL/dz_in (want_grad_z) vs the oracle
TOL_RUN = 2e-6      # relative L2 per tensor: two runs of the fast path (fp32 atomics in the batch contraction)
KEYS_PER_BLOCK = ("actnorm.b", "actnorm.logs", "invertible_1x1_conv.w", "f.fc_1.w", "f.fc_1.actnorm.b", "f.fc_1.actnorm.logs",
                  "f.fc_2.w", "f.fc_2.actnorm.b", "f.fc_2.actnorm.logs", "f.fc_zeros.w", "f.fc_zeros.b", "f.fc_zeros.logs")


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    assert tuple(lsnf_amd.flow.BLOCK_PARAM_KEYS) == KEYS_PER_BLOCK
    return lsnf_amd


def _params(nz, width, depth, coupling):
    p = O.init_params(nz, width, depth, seed=3)
    if coupling == 0:                    # additive: fc_zeros maps to the nz/2 shifts only (model.py:385)
        for i in range(depth):
            for k in ("f.fc_zeros.w", "f.fc_zeros.b", "f.fc_zeros.logs"):
                p[O.block_prefix(i) + k] = p[O.block_prefix(i) + k][:, : nz // 2].contiguous()
    return p


@functools.lru_cache(maxsize=2)
def _reference(nz, width, depth, coupling, B):
    """(params, smooth batch, rows replaced, {key: d(-mean ll)/dtheta}, d(-mean ll)/dz): the oracle in float64, one autograd
    pass for both (the same restated ops as O.grad_neg_mean_ll_wrt_params and O.grad_neg_sum_ll_wrt_z / B)."""
    p = _params(nz, width, depth, coupling)
    z, n_replaced = O.smooth_batch(p, B, nz, seed=B)
    p64 = O.to_dtype(p, torch.float64)
    live = {k: v.clone().requires_grad_(True) for k, v in p64.items() if O.is_live_param(k)}
    q = dict(p64)
    q.update(live)
    zz = z.double().requires_grad_(True)
    _, _, ll = O.flow_log_prob(q, zz, coupling)
    keys = sorted(live)
    grads = torch.autograd.grad(-ll.mean(), [zz] + [live[k] for k in keys])
    return p, z, n_replaced, dict(zip(keys, grads[1:])), grads[0]


def _rel(a, ref):
    return (a.double().cpu() - ref.double().cpu()).norm().item() / max(ref.double().norm().item(), 1e-30)


def _nan_buffers(F, plan, B, dev):
    act = F.new_act_saved(plan, B, dev)
    act.fill_(float("nan"))
    ws = F.new_params_workspace(plan, B, dev)
    ws.fill_(float("nan"))
    return act, ws


def _misaligned_copy(z):
    """The same values at a 4-byte-but-not-16-byte offset (a contiguous (B, nz) view into a larger allocation)."""
    buf = torch.empty(z.numel() + 1, dtype=z.dtype, device=z.device)
    zm = buf[1:].view(z.shape).copy_(z)
    assert zm.data_ptr() % 16 == 4 and zm.is_contiguous()
    return zm


def _setup(lsnf, dev, nz, width, depth, coupling, B):
    F = lsnf.flow
    p, z, n_replaced, ref, gz_ref = _reference(nz, width, depth, coupling, B)
    params = F.params_from_state_dict(p, depth, dev)
    plan = F.prepare(params, nz, width, depth, coupling)
    keys = [O.block_prefix(i) + k for i in range(depth) for k in KEYS_PER_BLOCK]
    return F, params, plan, z.to(dev), n_replaced, [ref[k] for k in keys], gz_ref, keys


MODES = {"BF16X3": "MATH_BF16X3", "BF16X3_PHASED": "MATH_BF16X3_PHASED", "FP16X2": "MATH_FP16X2"}
# (nz, width, depth, coupling, B, math mode, small-batch setting: None = automatic, else rows).  Together the cases launch every
# instantiation of the kernels that write or read the dumps (profiles/r05_param_grads_oracle_kernel_calls.csv): latency kernels
# (B <= 16 384) with 16 / 32 / 64 rows per workgroup (B <= 4 096 / 8 192 / above), throughput kernels with 4 / 8 waves
# (B <= 32 768 / above), geometries <HT, WT> = <1,1> (nz <= 64, width <= 32), <2,2>, <2,4>, dumps tiled where nz % 64 == 0 and
# width % 16 == 0, row-major elsewhere.  Cases that share a batch (the oracle is cached for the last two) run next to each other;
# the one the two tests below reuse runs last.
CASES = [(128, 64, 5, 1, 100, "BF16X3", None), (128, 64, 5, 1, 5000, "BF16X3", None),      # plain / LDS-staged contraction
         (100, 64, 5, 1, 4500, "BF16X3", None), (50, 33, 5, 1, 4100, "BF16X3", None),     # row vectors of 2 and 1
         (100, 128, 5, 1, 4200, "BF16X3", None), (128, 128, 5, 1, 3000, "BF16X3", None),
         (64, 32, 5, 1, 4000, "BF16X3", None), (64, 32, 5, 1, 8000, "BF16X3", None), (64, 32, 5, 1, 16000, "BF16X3", None),
         (128, 64, 5, 1, 14000, "BF16X3", None),                                           # latency kernels, row-major dumps, x3
         (128, 64, 5, 1, 65536, "BF16X3", None), (128, 64, 5, 1, 65536, "BF16X3_PHASED", None),
         (128, 64, 5, 1, 65536, "FP16X2", None),                                           # tiled dumps; fp16x2: row-major h
         (128, 64, 5, 1, 40001, "BF16X3", None), (128, 48, 5, 1, 20000, "BF16X3", None),  # ragged last tile; f_width 48
         (104, 64, 5, 1, 20000, "BF16X3", None), (104, 64, 5, 1, 40000, "BF16X3", None),  # row-major above the threshold
         (100, 64, 5, 1, 20000, "BF16X3", None),                                           # fp32 LDS contraction
         (100, 128, 5, 1, 20000, "BF16X3", None), (100, 128, 5, 1, 40000, "BF16X3", None),
         (48, 32, 5, 1, 20000, "BF16X3", None), (48, 32, 5, 1, 40000, "BF16X3", None),
         (64, 32, 5, 1, 17000, "BF16X3", None), (64, 32, 5, 1, 17000, "FP16X2", None),
         (64, 32, 5, 1, 40000, "BF16X3", None), (64, 32, 5, 1, 40000, "FP16X2", None),
         (128, 64, 5, 1, 20000, "BF16X3", None), (128, 64, 5, 1, 20000, "BF16X3_PHASED", None),
         (128, 64, 5, 1, 20000, "FP16X2", None),
         (128, 128, 5, 1, 20000, "BF16X3", None), (128, 128, 5, 1, 20000, "FP16X2", None),  # f_width 128: its tiled dumps
         (128, 128, 5, 1, 40001, "BF16X3", None), (128, 128, 5, 1, 40001, "FP16X2", None),
         (128, 64, 5, 1, 12289, "BF16X3", 0),                   # throughput kernels + x3 one row above LSNF_X3_MIN_ROWS, ragged tile
         (128, 64, 1, 1, 40000, "BF16X3", None), (128, 64, 16, 1, 20000, "BF16X3", None),  # no z_saved; LSNF_MAX_DEPTH
         (128, 64, 5, 0, 40000, "BF16X3", None), (128, 64, 5, 0, 5000, "BF16X3", None),    # additive coupling
         (128, 64, 5, 1, 40000, "BF16X3", None)]


def _case_id(c):
    nz, width, depth, coupling, B, mode, small = c
    return (f"nz{nz}-w{width}-d{depth}-{'affine' if coupling else 'additive'}-B{B}-{mode}"
            + ("" if small is None else f"-small{small}"))


@pytest.mark.parametrize("nz,width,depth,coupling,B,mode,small", CASES, ids=[_case_id(c) for c in CASES])
def test_parameter_gradients_match_float64_oracle(lsnf, gpu_device, nz, width, depth, coupling, B, mode, small):
    """All depth*12 tensors and dL/dz of the fast path and of the recomputing path against the fp64 oracle (2e-5 / 1e-5),
    against each other (2e-5, no allowance for kinked blocks: there are none), and the fast path against itself (2e-6)."""
    F, params, plan, z, n_replaced, refs, gz_ref, keys = _setup(lsnf, gpu_device, nz, width, depth, coupling, B)
    prev_small = F.set_small_batch_max(F.SMALL_BATCH_AUTO if small is None else small)
    prev_mode = F.set_math_mode(getattr(F, MODES[mode]))
    try:
        assert F.params_fast_path()
        act, ws = _nan_buffers(F, plan, B, gpu_device)
        z1, _, _, saved = F.forward(plan, z, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
        fast, gz_fast = F.backward_params(plan, params, z, z1, saved, ll_scale=-1.0 / B, want_grad_z=True, act_saved=act, workspace=ws)
        fast, gz_fast = [g.clone() for g in fast], gz_fast.clone()
        again = [g.clone() for g in F.backward_params(plan, params, z, z1, saved, ll_scale=-1.0 / B, act_saved=act, workspace=ws)]
        z1b, _, _, savedb = F.forward(plan, z, want_ll=False, save_for_backward=True)
        slow, gz_slow = F.backward_params(plan, params, z, z1b, savedb, ll_scale=-1.0 / B, want_grad_z=True)
        torch.cuda.synchronize()
    finally:
        F.set_small_batch_max(prev_small)
        F.set_math_mode(prev_mode)
    assert len(fast) == len(refs) == depth * 12
    worst = {"fast_vs_f64": (0.0, None), "slow_vs_f64": (0.0, None), "fast_vs_slow": (0.0, None), "run_to_run": (0.0, None)}
    bad = []
    for k, a, b, c, r in zip(keys, fast, slow, again, refs):
        r = r.reshape(a.shape)
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), k
        errs = {"fast_vs_f64": _rel(a, r), "slow_vs_f64": _rel(b, r), "fast_vs_slow": _rel(a, b), "run_to_run": _rel(c, a)}
        for what, e in errs.items():
            if e > worst[what][0]:
                worst[what] = (e, k)
            if not e <= (TOL_RUN if what == "run_to_run" else TOL):
                bad.append((what, k, e))
    e_gz_fast, e_gz_slow = _rel(gz_fast, gz_ref), _rel(gz_slow, gz_ref)
    print(f"\n[param-grads-oracle] {_case_id((nz, width, depth, coupling, B, mode, small))} rows_replaced={n_replaced} "
          + " ".join(f"{w}={e:.2e}({k})" for w, (e, k) in worst.items()) + f" gz_fast={e_gz_fast:.2e} gz_slow={e_gz_slow:.2e}")
    assert not bad, bad[:8]
    assert e_gz_fast <= TOL_GZ and e_gz_slow <= TOL_GZ, (e_gz_fast, e_gz_slow)


def _check_against_oracle(grads, refs, keys):
    errs = [(k, _rel(g, r.reshape(g.shape))) for k, g, r in zip(keys, grads, refs)]
    bad = [(k, e) for k, e in errs if not e <= TOL]
    assert not bad, bad[:8]


def test_fast_path_with_z_of_another_alignment_than_the_forwards(lsnf, gpu_device):
    """The forward decides the form of the h dump (tiled or row-major) from ITS z pointers; the backward used to re-decide
    from its own.  The same z values at a 4-byte-but-not-16-byte offset in one of the two calls must either be refused
    (LsnfError) or give the oracle's gradients -- never other numbers with a success code."""
    nz, width, depth, B = 128, 64, 5, 40000
    F, params, plan, z, _, refs, _, keys = _setup(lsnf, gpu_device, nz, width, depth, 1, B)
    zm = _misaligned_copy(z)
    prev_small = F.set_small_batch_max(F.SMALL_BATCH_AUTO)
    prev_mode = F.set_math_mode(F.MATH_BF16X3)
    outcome = []
    try:
        # forward on 16-byte aligned z (tiled dump), backward handed the misaligned copy
        act, ws = _nan_buffers(F, plan, B, gpu_device)
        z1, _, _, saved = F.forward(plan, z, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
        try:
            grads = F.backward_params(plan, params, zm, z1, saved, ll_scale=-1.0 / B, act_saved=act, workspace=ws)
        except lsnf.LsnfError as e:
            assert "aligned" in str(e)
            outcome.append("backward refused")
        else:
            _check_against_oracle(grads, refs, keys)
            outcome.append("backward matched the oracle")
        # forward on the misaligned copy, backward handed the aligned z
        act, ws = _nan_buffers(F, plan, B, gpu_device)
        try:
            z1, _, _, saved = F.forward(plan, zm, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
        except lsnf.LsnfError as e:
            assert "aligned" in str(e)
            outcome.append("forward refused")
        else:
            grads = F.backward_params(plan, params, z, z1, saved, ll_scale=-1.0 / B, act_saved=act, workspace=ws)
            _check_against_oracle(grads, refs, keys)
            outcome.append("forward + backward matched the oracle")
        torch.cuda.synchronize()
    finally:
        F.set_small_batch_max(prev_small)
        F.set_math_mode(prev_mode)
    print("\n[param-grads-oracle] misaligned z:", "; ".join(outcome))


def test_module_fast_path_takes_a_misaligned_z(lsnf, gpu_device):
    """`_netF` realigns a contiguous but not 16-byte aligned z before it takes the fast path: the flow-MLE step through
    autograd (train.py:404-411) and through `mle_grads` both give the oracle's gradients on it."""
    nz, width, depth, B = 128, 64, 5, 40000
    p, z, _, ref, _ = _reference(nz, width, depth, 1, B)
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=depth, f_flow_permutation=2, f_width=width, f_flow_coupling=1)
    net = lsnf._netF(hps, nz=nz)
    net.load_state_dict(p, strict=True)
    net = net.to(gpu_device)
    zm = _misaligned_copy(z.to(gpu_device))
    prev_mode = lsnf.flow.set_math_mode(lsnf.flow.MATH_BF16X3)
    try:
        for how in ("autograd", "mle_grads"):
            net.zero_grad()
            if how == "autograd":
                z1, logdet, _ = net(zm, objective=torch.zeros(B, device=gpu_device))
                (-(-0.5 * (z1 ** 2).sum(1) + O.LOG_2PI + logdet).mean()).backward()
            else:
                net.mle_grads(zm)
            named = dict(net.named_parameters())
            keys = sorted(ref)
            _check_against_oracle([named[k].grad for k in keys], [ref[k] for k in keys], keys)
    finally:
        lsnf.flow.set_math_mode(prev_mode)


def test_library_ignores_LSNF_TN_ABL(gpu_device, tmp_path):
    """LSNF_TN_ABL used to switch parts of the LDS-staged fp32 contraction off (only chunk 0 written, no MFMAs, no loads) in any
    process that had it set: wrong gradients with a success code (relative L2 of 1 to 4.8 on this test's 4 224 rows).  One fresh
    child with LSNF_TN_ABL=7 (the knob was read once per process) runs the recomputing path at 300 rows (plain contraction, three
    128-row chunks, the last one ragged) and at 4 224 (LDS-staged contraction, 33 chunks) -- the smallest sizes at which "only
    chunk 0" would show; its 12 tensors meet the oracle."""
    nz, width, depth, batches = 8, 4, 1, (300, 4224)
    out = tmp_path / "grads.pt"
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "param_grads_env_worker.py")
    proc = subprocess.Popen([sys.executable, worker, str(out), str(nz), str(width), str(depth)] + [str(B) for B in batches],
                            env=dict(os.environ, LSNF_TN_ABL="7"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        log = proc.communicate(timeout=300)[0]
    except subprocess.TimeoutExpired:
        proc.kill()
        raise
    assert proc.returncode == 0, log
    got = torch.load(str(out))
    keys = [O.block_prefix(i) + k for i in range(depth) for k in KEYS_PER_BLOCK]
    for B in batches:
        _, _, n_replaced, ref, _ = _reference(nz, width, depth, 1, B)
        assert len(got[B]) == len(keys) == 12
        errs = [(k, _rel(g, ref[k].reshape(g.shape))) for k, g in zip(keys, got[B])]
        print(f"\n[param-grads-oracle] LSNF_TN_ABL=7 nz{nz}-w{width}-d{depth}-B{B} rows_replaced={n_replaced} "
              + "worst=%.2e(%s)" % max((e, k) for k, e in errs))
        assert all(torch.isfinite(g).all() for g in got[B])
        _check_against_oracle(got[B], [ref[k] for k in keys], keys)

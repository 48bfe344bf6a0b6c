"""GPU: the library on both sides of its three 2 GiB dispatch guards, at the four-million-row batches where they lie
(tests/large_batch.py has the table, tests/test_large_batch_cpu.py holds it to its classes and shows on the CPU where a padded-group
access would land without a guard).  Default math mode, default small-batch threshold.

A 2 GiB tensor is the smallest shape at which these switches can go wrong, so the cases are few and each does little:
  * inputs are drawn on the device from a seeded device generator; nothing of full size crosses to the host -- WINDOWS of rows do
    (rows 0-63, the 128 rows around B / 2, the last 160 rows with their ragged tile, the rows around the sentinel row:
    large_batch.windows), at most 4 096 rows per case;
  * float64 is oracle.flow_oracle on the window rows, under the gates of DESIGN.md section 2, unchanged: log-prob 1e-5 relative, z1
    1e-4 absolute, dL/dz 1e-5 relative L2, parameter gradients 2e-5 relative L2 per tensor on kink-free rows, reverse 5e-5 of max|x|;
  * the SMALL RUN is the same rows as a batch of their own on the throughput kernels (lsnf_set_small_batch_max(0)); bit identity
    is asserted only where section 2 claims it across kernel families and batch sizes: z1 and the block outputs across the bf16x3
    forwards, the in-kernel draws, rows of backward_z, the reverse across batch sizes;
  * a float64 parameter gradient over four million rows cannot be computed, so a parameter-gradient batch is 2 048 kink-free LIVE
    rows (oracle.smooth_batch; three runs: from row 0, straddling B / 2, the last 700 rows) with a seeded upstream gradient in a sea
    of device-noise rows whose upstream gradient is zero: the exact gradient is that of the live rows alone, and a wrapped or
    mis-formed read of the dump drops or replaces live rows at full size.

Device memory (large_batch.forward_gb / params_gb, from the restated layouts): a (128, 64) depth-2 forward case holds about 9 GB
(z, z1, the block outputs, the 2.4 GB stash), a parameter-gradient case about 30 GB (those, g_z1, dL/dz and the 17 GB workspace).
A case skips only when torch.cuda.mem_get_info() shows less free memory than it needs, and prints both figures.  Every test frees
its tensors and empties the cache before it returns.

Each check prints `[large-batch] <check> <case>: worst error as a fraction of its gate`, each case its peak memory, its wall time
and its span on three clocks, by which the launches of a kernel trace of the module are assigned to its cases: the kernel names
in the docstrings below are what such a trace showed (profiles/large_batch.txt, profiles/large_batch_kernel_calls.csv)."""
import functools
import time

import pytest
import torch

import large_batch as L
import sample_restated as S
from oracle import flow_oracle as O
from oracle.philox_oracle import langevin_noise

pytestmark = pytest.mark.gpu

LL_REL, Z_ABS, GZ_REL, TOL, TOL_RUN, REV_X, PHILOX = 1e-5, 1e-4, 1e-5, 2e-5, 2e-6, 5e-5, 1e-4
KINK, KINK_REL = 2e-6, 2e-2                 # rows this near a ReLU kink are compared loosely (tests/test_gpu_reverse_backward.py et al.)
SUMS_REL = 1e-9                              # tests/test_gpu_forward.py test_in_kernel_batch_sums: |sum - float64 sum| <= 1e-9 |sum| + 1e-9
SEED, OFFSET = 2 ** 63 + 12345, (2 ** 32 - 1) + (5 << 32)        # tests/test_gpu_sample.py: every word of the Philox counter and key is live
KEYS_PER_BLOCK = ("actnorm.b", "actnorm.logs", "invertible_1x1_conv.w", "f.fc_1.w", "f.fc_1.actnorm.b", "f.fc_1.actnorm.logs",
                  "f.fc_2.w", "f.fc_2.actnorm.b", "f.fc_2.actnorm.logs", "f.fc_zeros.w", "f.fc_zeros.b", "f.fc_zeros.logs")


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    F = lsnf_amd.flow
    assert F.set_math_mode(-1) == F.MATH_BF16X3 and F.set_small_batch_max(-1) == L.SMALL_MAX_AUTO      # the default dispatch
    return lsnf_amd


@functools.lru_cache(maxsize=None)
def _weights(geo):
    nz, width, depth, coupling = geo
    p = O.init_params(nz, width, depth, seed=3)
    return p, O.to_dtype(p, torch.float64)


_PLANS = {}


def _plan(lsnf, dev, geo):
    if geo not in _PLANS:
        params = lsnf.flow.params_from_state_dict(_weights(geo)[0], geo[2], dev)
        _PLANS[geo] = (lsnf.flow.prepare(params, *geo), params)
    return _PLANS[geo]


def _id(case):
    return "nz%d-w%d-B%d" % (case[0], case[1], case[4])


class Span:
    """One case: the memory check in front, the frees behind, peak memory, wall time and the clocks of its first and last launch."""

    def __init__(self, what, case, need):
        self.what, self.case, self.need = what, case, need

    def __enter__(self):
        free, total = torch.cuda.mem_get_info()
        print("\n[large-batch] %s %s: needs %.1f GB, %.1f of %.1f GB free" % (self.what, _id(self.case), self.need / 1e9, free / 1e9, total / 1e9))
        if free < self.need:
            pytest.skip("%.1f GB free, the case needs %.1f GB" % (free / 1e9, self.need / 1e9))
        torch.cuda.reset_peak_memory_stats()
        torch.cuda.synchronize()
        self.t0 = (time.perf_counter(), time.clock_gettime_ns(time.CLOCK_MONOTONIC), time.clock_gettime_ns(time.CLOCK_BOOTTIME), time.time_ns())
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        t1 = (time.perf_counter(), time.clock_gettime_ns(time.CLOCK_MONOTONIC), time.clock_gettime_ns(time.CLOCK_BOOTTIME), time.time_ns())
        print("[large-batch] %s %s: peak %.1f GB, %.2f s; span monotonic %d %d boottime %d %d realtime %d %d"
              % (self.what, _id(self.case), torch.cuda.max_memory_allocated() / 1e9, t1[0] - self.t0[0], self.t0[1], t1[1], self.t0[2], t1[2],
                 self.t0[3], t1[3]))
        torch.cuda.empty_cache()
        return False


def _report(check, case, err, gate):
    print("[large-batch] %s %s: %.3e = %.3f of its gate %.1e" % (check, _id(case), err, err / gate, gate))
    assert err <= gate, (check, case, err, gate)


def _same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def _rel_rows(a, ref):
    """log-prob / log-det, per row: |a - ref| / max(|ref|, 1) (tests/test_gpu_forward.py)."""
    return ((a.double().cpu() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()


def _rel_l2(a, ref):
    return (a.double().cpu() - ref.double()).norm().item() / max(ref.double().norm().item(), 1e-30)


def _rows(case, dev):
    return torch.cat([torch.arange(a, b, device=dev) for a, b in L.windows(case)])


def _randn(dev, seed, *shape):
    return torch.randn(*shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _guard(dev):
    return torch.full((4096,), 7.0, device=dev)       # allocated behind the outputs: a store past the batch would land here


def _untouched(*guards):
    return all(g.min().item() == 7.0 == g.max().item() for g in guards)


def _sums(check, case, stats, ll, logdet):
    """The in-kernel batch sums against the float64 sum of the call's own per-row outputs (the sums are taken on the device)."""
    s = stats.cpu()
    for name, got, rows in (("ll", s[4].item(), ll), ("logdet", s[5].item(), logdet)):
        ref = rows.double().sum().item()
        _report("%s sum-%s" % (check, name), case, abs(got - ref), SUMS_REL * abs(ref) + 1e-9)
    assert s[6].item() == case[4] and s[:4].abs().max().item() == 0.0 and s[8:].view(torch.int64).abs().max().item() == 0


# ------------------------------------------------------------------------------------------------ F1 (+ F2): the forward and backward_z
@pytest.mark.parametrize("case", L.STASH_CASES, ids=_id)
def test_forward_and_backward_z(lsnf, gpu_device, case):
    """Plain, then with z_saved + act_saved (NaN-filled first, a sentinel buffer behind them), then backward_z from that stash, each with
    its in-kernel batch sums: z1 and the block outputs on the windows are the small run's bits, ll / logdet / dz are held to float64,
    dz also to the small run's bits.  Below the stash guard the stash forward is lsnf_fwd3q_kernel<2, 8, 2, 1>, from the guard on
    lsnf_fwd3b_kernel (profiles/large_batch.txt: per case, from a kernel trace of this module)."""
    F, dev = lsnf.flow, gpu_device
    geo, B = case[:4], case[4]
    nz, depth = geo[0], geo[2]
    plan, _ = _plan(lsnf, dev, geo)
    with Span("forward", case, L.forward_gb(geo, B) + 4 * B * nz + (1 << 28)) as span:
        idx = _rows(case, dev)
        z = _randn(dev, B, B, nz)
        out, g0, stats = (_nan(dev, B, nz), _nan(dev, B), _nan(dev, B)), _guard(dev), F.new_stats(dev)
        F.forward(plan, z, out=out, stats=stats)
        assert not bool(torch.isnan(out[0]).any() | torch.isnan(out[1]).any() | torch.isnan(out[2]).any())
        _sums("plain-forward", case, stats, out[2], out[1])
        plain = [t[idx].clone() for t in out]
        del out
        out = (_nan(dev, B, nz), _nan(dev, B), _nan(dev, B))
        act, saved, g1 = F.new_act_saved(plan, B, dev).fill_(float("nan")), _nan(dev, depth - 1, B, nz), _guard(dev)
        F.forward(plan, z, out=out, stats=stats, act_saved=act, z_saved_out=saved)
        assert not bool(torch.isnan(out[0]).any() | torch.isnan(out[1]).any() | torch.isnan(out[2]).any() | torch.isnan(saved).any())
        # (the stash, csrc/lsnf_layout.h lsnf_act_layout: the first 2 048 floats of every whole 32-row tile of every block are sigmas)
        assert not bool(torch.isnan(act.view(depth, -1, L.act_layout(B, 2, 2)[0])[:, : B // 32, :2048]).any())
        _sums("stash-forward", case, stats, out[2], out[1])
        dz = F.backward_z(plan, out[0], saved, ll_scale=-1.0, act_saved=act)
        assert _untouched(g0, g1)
        full = [t[idx].clone() for t in out] + [saved[:, idx].clone(), dz[idx].clone()]
        zs = z[idx].clone()
        del z, out, act, saved, dz, g0, g1
    # the small run: the window rows as a batch of their own on the throughput kernels
    prev = F.set_small_batch_max(0)
    try:
        n = zs.shape[0]
        acts = F.new_act_saved(plan, n, dev)
        z1s, lds, lls, saveds = F.forward(plan, zs, save_for_backward=True, act_saved=acts)
        dzs = F.backward_z(plan, z1s, saveds, ll_scale=-1.0, act_saved=acts)
        torch.cuda.synchronize()
    finally:
        F.set_small_batch_max(prev)
    assert _same_bits(full[0], z1s) and _same_bits(plain[0], z1s), "z1 on the windows is not the small run's bits"
    assert _same_bits(full[3], saveds), "the block outputs on the windows are not the small run's bits"
    assert _same_bits(full[4], dzs), "backward_z on the windows is not the small run's bits"
    p64 = _weights(geo)[1]
    z64 = zs.double().cpu()
    z1r, ldr, llr = O.flow_log_prob(p64, z64)
    gzr = O.grad_neg_sum_ll_wrt_z(p64, z64)
    for name, got in (("plain", plain), ("stash", full)):
        _report("%s z1-abs" % name, case, (got[0].double().cpu() - z1r).abs().max().item(), Z_ABS)
        _report("%s logdet-rel" % name, case, _rel_rows(got[1], ldr), LL_REL)
        _report("%s ll-rel" % name, case, _rel_rows(got[2], llr), LL_REL)
    # rows within 2e-6 of a ReLU kink (oracle.relu_margin; DESIGN.md section 2, "ReLU kinks") may take either side in fp32: they are
    # compared loosely (2 %), every other row strictly
    ok = O.relu_margin(_weights(geo)[0], zs.cpu()) >= KINK
    print("[large-batch] backward_z %s: %d of %d window rows within %.0e of a kink" % (_id(case), int((~ok).sum()), ok.numel(), KINK))
    _report("backward_z rel-L2", case, _rel_l2(full[4].cpu()[ok], gzr[ok]), GZ_REL)
    _report("backward_z worst-row rel-L2", case, ((full[4].double().cpu() - gzr).norm(dim=1) / gzr.norm(dim=1))[ok].max().item(), 10 * GZ_REL)
    if not bool(ok.all()):
        _report("backward_z kink-rows rel-L2", case, _rel_l2(full[4].cpu()[~ok], gzr[~ok]), KINK_REL)
    del full, plain, zs
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ F3: reverse, sample, the Langevin step
def test_reverse_sample_and_langevin_step(lsnf, gpu_device):
    """4 194 369 rows of (128, 64): the reverse (lsnf_rev3_kernel<2, 2, 8, ...> by the trace), `sample` with Philox noise and the Langevin step (the stash forward
    past its guard, then lsnf_bwd3_kernel with the update).  Windows are held to float64 and to the small run; two shards with
    their row0 draw what one call draws on the windows."""
    F, dev, case = lsnf.flow, gpu_device, L.CHAIN_CASE
    geo, B = case[:4], case[4]
    nz = geo[0]
    plan, _ = _plan(lsnf, dev, geo)
    p, p64 = _weights(geo)
    wins, step = L.windows(case), 0.1
    ph = F.PhiloxNoise(SEED, OFFSET)
    with Span("reverse", case, 4 * (3 * B * nz + 2 * B) + (1 << 28)):
        idx = _rows(case, dev)
        eps = _randn(dev, B + 1, B, nz)
        out, g0 = (_nan(dev, B, nz), _nan(dev, B)), _guard(dev)
        F.reverse(plan, eps, out=out)
        assert not bool(torch.isnan(out[0]).any() | torch.isnan(out[1]).any()) and _untouched(g0)
        rev = [eps[idx].clone(), out[0][idx].clone(), out[1][idx].clone()]
        del eps, out, g0
    with Span("sample", case, 4 * (2 * B * nz + 2 * B) + (1 << 28)):
        out, g0 = (_nan(dev, B, nz), _nan(dev, B), _nan(dev, B, nz), _nan(dev, B)), _guard(dev)
        F.sample(plan, B, ph, out=out)
        assert not any(bool(torch.isnan(t).any()) for t in out) and _untouched(g0)
        smp = [t[idx].clone() for t in out]
        del out, g0
    with Span("sample-shards", case, 4 * (2 * B * nz + 2 * B) + (1 << 28)):
        cut = B // 2 + 19                     # inside the middle window, no multiple of 16: both shards own rows of it
        lo = F.sample(plan, cut, ph, want_eps=True, want_ll=True)
        hi = F.sample(plan, B - cut, F.PhiloxNoise(SEED, OFFSET, row0=cut), want_eps=True, want_ll=True)
        assert wins[1][0] < cut < wins[1][1]
        shards = [torch.cat([a[idx[idx < cut]], b[idx[idx >= cut] - cut]]) for a, b in zip(lo, hi)]
        del lo, hi
    with Span("langevin-step", case, L.forward_gb(geo, B) + 4 * (B * nz + 2 * B) + (1 << 28)):
        z = _randn(dev, B + 2, B, nz)
        z_new, ll, gf, _ = F.langevin_step(plan, z, None, ph.step(), step)
        assert not bool(torch.isnan(z_new).any() | torch.isnan(ll).any() | torch.isnan(gf).any())
        lv = [z[idx].clone(), z_new[idx].clone(), ll[idx].clone(), gf[idx].clone()]
        del z, z_new, ll, gf
    # the small runs: all windows as one batch where the rows carry no index (the reverse), one batch per window, with its row0,
    # where they do (the draws)
    prev = F.set_small_batch_max(0)
    try:
        xs, objs = F.reverse(plan, rev[0])
        small_smp, small_lv, o = [], [], 0
        for a, b in wins:
            small_smp.append(F.sample(plan, b - a, F.PhiloxNoise(SEED, OFFSET, row0=a), want_eps=True, want_ll=True))
            small_lv.append(F.langevin_step(plan, lv[0][o:o + b - a].contiguous(), None, F.PhiloxNoise(SEED, OFFSET + 1, row0=a), step)[:3])
            o += b - a
        small_smp = [torch.cat(t) for t in zip(*small_smp)]
        small_lv = [torch.cat(t) for t in zip(*small_lv)]
        xe, obje = F.reverse(plan, smp[2])    # sample's x and objective_out are the reverse of its own draws, bit for bit
        torch.cuda.synchronize()
    finally:
        F.set_small_batch_max(prev)
    # bits
    assert _same_bits(rev[1], xs) and _same_bits(rev[2], objs), "the reverse on the windows is not the small run's bits"
    assert _same_bits(smp[2], small_smp[2]), "the in-kernel draws on the windows are not the small run's bits"
    assert _same_bits(smp[0], small_smp[0]) and _same_bits(smp[1], small_smp[1]), "sample's x / objective are not the small run's bits"
    assert _same_bits(smp[0], xe) and _same_bits(smp[1], obje), "sample is not the reverse of its own draws"
    assert all(_same_bits(a, b) for a, b in zip(smp, shards)), "two shards with their row0 do not draw what one call draws"
    assert _same_bits(lv[1], small_lv[0]), "the Langevin step on the windows is not the small run's bits"
    # float64
    x64, obj64, _ = S.flow_at(p, rev[0].cpu())
    _report("reverse x", case, (rev[1].double().cpu() - x64).abs().max().item() / max(1.0, x64.abs().max().item()), REV_X)
    _report("reverse objective-rel", case, _rel_rows(rev[2], obj64), LL_REL)
    draws = torch.cat([S.draws(b - a, nz, SEED, OFFSET, a) for a, b in wins])
    _report("sample draws-abs", case, (smp[2].double().cpu() - draws).abs().max().item(), PHILOX)
    x64, obj64, _ = S.flow_at(p, smp[2].cpu())
    _report("sample x", case, (smp[0].double().cpu() - x64).abs().max().item() / max(1.0, x64.abs().max().item()), REV_X)
    _report("sample ll-rel (own outputs)", case, _rel_rows(smp[3], S.ll(smp[2].double().cpu(), smp[1].double().cpu())), LL_REL)
    # the Langevin step: z_new = z - 0.5 s^2 grad_f + s noise.  Its gate is put together from the existing ones: the draws' 1e-4 absolute
    # times s, the gradient's 1e-5 (of the largest row norm) times 0.5 s^2, and two fp32 roundings of the result
    z64 = lv[0].double().cpu()
    noise = torch.cat([torch.from_numpy(langevin_noise(b - a, nz, SEED, OFFSET + 1, a)) for a, b in wins])
    zr, _, gfr = O.langevin_prior_step(p64, z64, None, step, noise)
    _, _, llr = O.flow_log_prob(p64, z64)
    gate = step * PHILOX + 0.5 * step * step * GZ_REL * gfr.norm(dim=1).max().item() + 2 * 2.0 ** -24 * zr.abs().max().item()
    ok = O.relu_margin(p, lv[0].cpu()) >= KINK       # rows at a ReLU kink: the gradient part loosely (2 %), as above
    print("[large-batch] langevin %s: %d of %d window rows within %.0e of a kink" % (_id(case), int((~ok).sum()), ok.numel(), KINK))
    _report("langevin z_new-abs", case, (lv[1].double().cpu() - zr)[ok].abs().max().item(), gate)
    _report("langevin ll-rel", case, _rel_rows(lv[2], llr), LL_REL)
    _report("langevin gf_norm-rel", case, _rel_rows(lv[3].cpu()[ok], gfr.norm(dim=1)[ok]), GZ_REL)
    if not bool(ok.all()):
        loose = step * PHILOX + 0.5 * step * step * KINK_REL * gfr.norm(dim=1).max().item() + 2 * 2.0 ** -24 * zr.abs().max().item()
        _report("langevin kink-rows z_new-abs", case, (lv[1].double().cpu() - zr)[~ok].abs().max().item(), loose)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ P1 (+ F2): backward_params
@functools.lru_cache(maxsize=None)
def _live_reference(geo):
    """The 2 048 live rows of a geometry (the same values at every batch size: only where they sit changes), their upstream gradient,
    and the float64 gradient of L = sum_b (g_z1_b . z1_b + g_logdet_b logdet_b) over them, with respect to every parameter and to z."""
    nz, width, depth, coupling = geo
    p, p64 = _weights(geo)
    z, n_replaced = O.smooth_batch(p, L.LIVE_ROWS, nz, seed=nz * 1000 + width)
    g = torch.Generator().manual_seed(nz + width)
    g_z1, g_ld = torch.randn(L.LIVE_ROWS, nz, generator=g), torch.randn(L.LIVE_ROWS, generator=g)
    live = {k: v.clone().requires_grad_(True) for k, v in p64.items() if O.is_live_param(k)}
    q = dict(p64)
    q.update(live)
    zz = z.double().requires_grad_(True)
    z1, ld = O.flow_forward(q, zz, torch.zeros(L.LIVE_ROWS, dtype=torch.float64), coupling)
    keys = [O.block_prefix(i) + k for i in range(depth) for k in KEYS_PER_BLOCK]
    grads = torch.autograd.grad((g_z1.double() * z1).sum() + (g_ld.double() * ld).sum(), [zz] + [live[k] for k in keys])
    return z, g_z1, g_ld, n_replaced, keys, grads[1:], grads[0]


@pytest.mark.parametrize("case", L.PARAMS_CASES, ids=_id)
def test_parameter_gradients(lsnf, gpu_device, case):
    """The fast path (forward with stash and h dump, lsnf_bwd3_kernel, batch contraction), lsnf_backward_params_det on the same
    workspace and the recomputing path.  Every tensor within 2e-5 of the float64 gradient of the 2 048 live rows, dL/dz on them
    within 1e-5 and exactly 0.0 on every filler row, fast and recomputing paths within 2e-5 of each other, two runs of the fast
    path within 2e-6, two runs of the det entry bit-equal.  Below the contraction guard the dump is tiled and the contraction is
    lsnf_contract_x3_kernel, from the guard on the dump is row-major and the contraction lsnf_tn_gemm_lds_kernel<4, ...> (by the trace)."""
    F, dev = lsnf.flow, gpu_device
    geo, B = case[:4], case[4]
    nz, depth = geo[0], geo[2]
    plan, params = _plan(lsnf, dev, geo)
    zl, gl_z1, gl_ld, n_replaced, keys, refs, gz_ref = _live_reference(geo)
    with Span("params", case, L.params_gb(geo, B) + (1 << 29)):
        idx = torch.cat([torch.arange(a, b, device=dev) for a, b in L.live_runs(B)])
        z = _randn(dev, B + 3, B, nz)
        z[idx] = zl.to(dev)
        g_z1, g_ld = torch.zeros(B, nz, device=dev), torch.zeros(B, device=dev)
        g_z1[idx], g_ld[idx] = gl_z1.to(dev), gl_ld.to(dev)
        act = F.new_act_saved(plan, B, dev).fill_(float("nan"))
        ws = F.new_params_workspace(plan, B, dev, deterministic=True).fill_(float("nan"))
        stats = F.new_stats(dev)
        z1, logdet, ll, saved = F.forward(plan, z, save_for_backward=True, act_saved=act, params_ws=ws, stats=stats)
        _sums("dump-forward", case, stats, ll, logdet)
        up = dict(g_z1=g_z1, g_logdet=g_ld)
        fast, gz = F.backward_params(plan, params, z, z1, saved, want_grad_z=True, act_saved=act, workspace=ws, **up)
        fast, gz_live = [g.clone() for g in fast], gz[idx].clone()
        # dL/dz is 0.0 on every filler row: the rows of the whole batch with a non-zero entry are the live rows, no other
        nonzero = torch.nonzero((gz != 0).any(dim=1)).flatten()
        assert nonzero.numel() == L.LIVE_ROWS and bool((nonzero == idx).all()), "dL/dz is not 0.0 on the filler rows"
        del gz
        again = [g.clone() for g in F.backward_params(plan, params, z, z1, saved, act_saved=act, workspace=ws, **up)]
        det = [g.clone() for g in F.backward_params(plan, params, z, z1, saved, act_saved=act, workspace=ws, deterministic=True, **up)]
        det2 = [g.clone() for g in F.backward_params(plan, params, z, z1, saved, act_saved=act, workspace=ws, deterministic=True, **up)]
        del act, ws
        torch.cuda.empty_cache()
        slow, gz = F.backward_params(plan, params, z, z1, saved, want_grad_z=True, **up)
        slow, gz_slow = [g.clone() for g in slow], gz[idx].clone()
        nonzero = torch.nonzero((gz != 0).any(dim=1)).flatten()
        assert nonzero.numel() == L.LIVE_ROWS and bool((nonzero == idx).all()), "dL/dz of the recomputing path is not 0.0 on the filler rows"
        del gz, z, z1, logdet, ll, saved, g_z1, g_ld, up
    assert len(fast) == len(refs) == depth * 12
    assert all(_same_bits(a, b) for a, b in zip(det, det2)), "two runs of lsnf_backward_params_det differ"
    worst = {}
    for k, f, s, a, d, r in zip(keys, fast, slow, again, det, refs):
        r = r.reshape(f.shape)
        assert bool(torch.isfinite(f).all() & torch.isfinite(s).all() & torch.isfinite(d).all()), k
        for what, e in (("fast vs float64", _rel_l2(f, r)), ("recomputing vs float64", _rel_l2(s, r)), ("det vs float64", _rel_l2(d, r)),
                        ("fast vs recomputing", _rel_l2(f, s.cpu())), ("fast run-to-run", _rel_l2(a, f.cpu()))):
            if e >= worst.get(what, (-1.0, None))[0]:
                worst[what] = (e, k)
    print("[large-batch] params %s: rows_replaced=%d worst tensors %s" % (_id(case), n_replaced, {w: k for w, (_, k) in worst.items()}))
    for what, (e, _) in worst.items():
        _report("params " + what, case, e, TOL_RUN if what == "fast run-to-run" else TOL)
    _report("params dL/dz fast", case, _rel_l2(gz_live, gz_ref), GZ_REL)
    _report("params dL/dz recomputing", case, _rel_l2(gz_slow, gz_ref), GZ_REL)
    torch.cuda.empty_cache()

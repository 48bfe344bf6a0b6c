"""GPU: fused prior sampling -- `lsnf_sample` / `flow.sample` / `_netF.sample` / `langevin.sample_x`.

Anchors: (a) the draws against oracle/philox_oracle.py; (b) BIT equality of (z_out, objective_out) with `lsnf_reverse` fed the
call's own eps_out under the same dispatch (the sampling form of a reverse kernel is the same arithmetic after the row load), and of
every sharding / call form with the plain call; (c) the float64 oracle through tests/sample_restated.py.
Tolerances are the ones the suite already holds (names say where each comes from); the moment bounds follow from N.

Every test runs under the six settings of conftest.py's `kernels` fixture and under the default dispatch (`setting`), unless its
name says otherwise."""
import contextlib
import ctypes
import itertools
import math
import types

import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden
from oracle import flow_oracle as O
import sample_restated as S

pytestmark = pytest.mark.gpu

PHILOX = 1e-4        # in-kernel N(0,1) draws, absolute (tests/test_gpu_call_forms.py)
REV_X = 5e-5         # reverse: x, of max|x| (tests/test_gpu_reverse_backward.py inverse_tolerance's floor)
LL_REL = 1e-5        # log-prob, relative per row (tests/test_gpu_forward.py)
TOL_RUN = 2e-6       # parameter gradients: two runs through fp32 atomics, of each tensor's norm (tests/test_gpu_module.py)
SEED = 2 ** 63 + 12345                      # as tests/test_gpu_call_forms.py: every word of the Philox counter and key is live
OFFSET = (2 ** 32 - 1) + (5 << 32)
ROW0 = 2 ** 32 - 7                          # the batch straddles the 32-bit row boundary
SETTINGS = ["latency-kernels", "latency-kernels-bf16x3", "throughput-kernels", "throughput-kernels-bf16x3",
            "throughput-kernels-bf16x3_phased", "throughput-kernels-fp16x2"]           # conftest.py `kernels`


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


@contextlib.contextmanager
def dispatch(F, name):
    """conftest.py's `kernels` settings by name; "default" leaves the automatic dispatch in force."""
    if name == "default":
        assert F.set_math_mode(-1) == F.MATH_BF16X3 and F.set_small_batch_max(-1) == 16384
        yield
        return
    prev = F.set_small_batch_max(1 << 30 if name.startswith("latency-kernels") else 0)
    prev_math = F.set_math_mode(F.MATH_BF16X3 if name.endswith("bf16x3") else F.MATH_BF16X3_PHASED if name.endswith("bf16x3_phased")
                                else F.MATH_FP16X2 if name.endswith("fp16x2") else F.MATH_FP32)
    try:
        yield
    finally:
        F.set_small_batch_max(prev)
        F.set_math_mode(prev_math)


@pytest.fixture(params=SETTINGS + ["default"])
def setting(request, lsnf):
    with dispatch(lsnf.flow, request.param):
        yield request.param


def _params(nz, width, depth, coupling, seed=3, fcz_std=0.05):
    p = O.init_params(nz, width, depth, seed=seed, fcz_std=fcz_std)
    if coupling == 0:                    # additive: fc_zeros maps to the nz/2 shifts only (model.py:385)
        for i in range(depth):
            for k in ("f.fc_zeros.w", "f.fc_zeros.b", "f.fc_zeros.logs"):
                p[O.block_prefix(i) + k] = p[O.block_prefix(i) + k][:, : nz // 2].contiguous()
    return p


def _plan(lsnf, p, nz, width, depth, coupling, dev):
    return lsnf.prepare(lsnf.params_from_state_dict(p, depth, dev), nz, width, depth, coupling)


_CACHE = {}


def _geometry(lsnf, dev, nz, width, depth, coupling):
    key = (nz, width, depth, coupling)
    if key not in _CACHE:
        p = _params(nz, width, depth, coupling, fcz_std=0.03 if depth > 8 else 0.05)
        _CACHE[key] = (p, _plan(lsnf, p, nz, width, depth, coupling, dev))
    return _CACHE[key]


def _golden(lsnf, dev, name):
    if name not in _CACHE:
        p, g = load_golden(name)
        nz, w, d, c = int(g["meta_nz"]), int(g["meta_width"]), int(g["meta_depth"]), int(g.get("meta_coupling", 1))
        _CACHE[name] = (p, g, _plan(lsnf, p, nz, w, d, c, dev), nz)
    return _CACHE[name]


def _full(F, plan, B, ph, T=1.0):
    x, obj, eps, ll = F.sample(plan, B, ph, temperature=T, want_eps=True, want_ll=True)
    return x, obj, eps, ll


def _same_bits(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def _rel(a, ref):
    return ((a.double() - ref.double()).abs() / ref.double().abs().clamp_min(1.0)).max().item()


def _own_outputs_ll(eps, obj):
    """float64 ll from the call's own outputs."""
    return S.ll(eps.double(), obj.double())


# ------------------------------------------------------------------------------------------------- 1. the draws
@pytest.mark.parametrize("T", [1.0, 0.7, 0.0])
def test_draws_match_the_philox_oracle(lsnf, setting, gpu_device, T):
    F = lsnf.flow
    for nz, w, B in ((128, 64, 130), (100, 64, 77), (126, 127, 33), (2, 1, 33)):
        _, plan = _geometry(lsnf, gpu_device, nz, w, 2, 1)
        _, _, eps, _ = _full(F, plan, B, F.PhiloxNoise(SEED, OFFSET, ROW0), T)
        ref = S.draws(B, nz, SEED, OFFSET, ROW0, T).to(gpu_device)
        err = (eps.double() - ref).abs().max().item()
        print(f"draws {setting} nz={nz} B={B} T={T}: max abs err {err:.3e} (allowed {PHILOX * max(T, 1.0):.1e})")
        assert bool(torch.isfinite(eps).all()) and err <= PHILOX * max(T, 1.0)
        if T == 0.0:
            assert bool((eps == 0).all())


def test_draws_are_the_same_bits_in_every_setting_and_for_every_workgroup_shape(lsnf, gpu_device):
    F = lsnf.flow
    _, plan = _geometry(lsnf, gpu_device, 128, 64, 2, 1)
    ph = F.PhiloxNoise(SEED, OFFSET, ROW0)
    base = None
    for name in SETTINGS + ["default"]:
        with dispatch(F, name):
            for T in (1.0, 0.7):
                eps = _full(F, plan, 130, ph, T)[2]
                if T == 1.0:
                    base = eps if base is None else base
                    assert _same_bits(eps, base), name
                else:
                    assert _same_bits(eps, 0.7 * base) or _same_bits(eps, torch.tensor(0.7, device=gpu_device) * base), name
    with dispatch(F, "default"):
        # 16 / 32 / 64 rows per latency workgroup, the 4- and 8-wave throughput kernels
        for B in (100, 5003, 16384, 40000):
            eps = _full(F, plan, B, ph)[2]
            assert _same_bits(eps[:100], base[:100]), B
            mid = B // 2
            one = _full(F, plan, 1, F.PhiloxNoise(SEED, OFFSET, ROW0 + mid))[2]
            assert _same_bits(eps[mid:mid + 1], one), B


# ------------------------------------------------------------------------------------------------- 2. the flow, 3. ll_out
def _check_flow(lsnf, setting, dev, p, plan, nz, B, x_tol, T=1.0):
    """x_tol: gate of x against the float64 oracle, of max|x|."""
    F = lsnf.flow
    ph = F.PhiloxNoise(SEED, OFFSET + B, ROW0)
    x, obj, eps, ll = _full(F, plan, B, ph, T)
    xr, objr = F.reverse(plan, eps)
    assert _same_bits(x, xr) and _same_bits(obj, objr), (setting, nz, B)
    x64, obj64, ll64 = (t.to(dev) for t in S.flow_at(p, eps.cpu()))
    scale = max(1.0, x64.abs().max().item())
    ex = (x.double() - x64).abs().max().item() / scale
    own = _own_outputs_ll(eps, obj)
    ell = _rel(ll, own)
    print(f"flow {setting} nz={nz} B={B}: x err {ex:.3e} (allowed {x_tol:.3e}), ll vs own outputs {ell:.3e}")
    assert ex <= x_tol
    assert bool(torch.isfinite(ll).all()) and ell <= LL_REL
    return x, obj, eps, ll


def _oracle_fp32_x_error(p, eps):
    """The oracle's own fp32-vs-fp64 error of x = f^-1(eps), of max|x|: what any fp32 inverse of this stack is granted 3x of."""
    x32, _ = O.flow_reverse(O.to_dtype(p, torch.float32), eps.float(), torch.zeros(eps.shape[0]))
    x64 = S.flow_at(p, eps)[0]
    return (x32.double() - x64).abs().max().item() / max(1.0, x64.abs().max().item())


@pytest.mark.parametrize("B", [1, 33, 77])
@pytest.mark.parametrize("name", golden_names())
def test_sample_is_reverse_of_its_own_draws_golden(lsnf, setting, gpu_device, name, B):
    p, g, plan, nz = _golden(lsnf, gpu_device, name)
    tol = REV_X
    if "roundtrip" in g:                     # test_gpu_reverse_backward.inverse_tolerance
        tol = max(REV_X, 3.0 * float(np.abs(g["roundtrip"] - g["z"]).max()) / max(1.0, float(np.abs(g["z"]).max())))
    _check_flow(lsnf, setting, gpu_device, p, plan, nz, B, tol)


GEOMS = [(2, 1, 5, 1), (2, 1, 5, 0), (126, 127, 5, 1), (126, 127, 5, 0), (64, 48, 1, 1), (64, 48, 16, 1), (128, 64, 5, 0)]


@pytest.mark.parametrize("B", [1, 33, 77])
@pytest.mark.parametrize("nz,w,depth,coupling", GEOMS)
def test_sample_is_reverse_of_its_own_draws_geometries(lsnf, setting, gpu_device, nz, w, depth, coupling, B):
    p, plan = _geometry(lsnf, gpu_device, nz, w, depth, coupling)
    eps = S.draws(B, nz, SEED, OFFSET + B, ROW0)
    tol = max(REV_X, 3.0 * _oracle_fp32_x_error(p, eps))          # (no stored round trip: the oracle's own fp32 error instead)
    _check_flow(lsnf, setting, gpu_device, p, plan, nz, B, tol)


@pytest.mark.parametrize("nz,w,depth,coupling,B", [(128, 64, 5, 1, 130), (100, 64, 5, 1, 77), (20, 12, 5, 0, 33), (2, 1, 5, 1, 33)])
def test_forward_at_the_sample_returns_ll_out(lsnf, setting, gpu_device, nz, w, depth, coupling, B):
    """lsnf_forward(z_out).ll against ll_out: within max(1e-5 relative, 3 x the oracle's own fp32-vs-fp64 error of that round trip
    on that input)."""
    F = lsnf.flow
    p, plan = _geometry(lsnf, gpu_device, nz, w, depth, coupling)
    x, obj, eps, ll = _full(F, plan, B, F.PhiloxNoise(SEED, OFFSET, ROW0))
    e32 = eps.cpu()
    p32 = O.to_dtype(p, torch.float32)
    x32, _ = O.flow_reverse(p32, e32, torch.zeros(B))
    ll32 = O.flow_log_prob(p32, x32, coupling)[2]
    ll64 = S.flow_at(p, e32)[2]
    own = _rel(ll32, ll64)
    tol = max(LL_REL, 3.0 * own)
    _, _, ll_fwd, _ = F.forward(plan, x)
    err = _rel(ll_fwd, ll)
    print(f"forward-at-sample {setting} nz={nz} B={B}: {err:.3e} (allowed {tol:.3e}, oracle fp32 {own:.3e})")
    assert err <= tol
    assert _rel(ll, ll64.to(gpu_device)) <= tol


# ------------------------------------------------------------------------------------------------- 4. sharding
@pytest.mark.parametrize("cuts", [(37,), (10, 60)])
def test_shards_draw_what_one_call_draws(lsnf, setting, gpu_device, cuts):
    F = lsnf.flow
    p, plan = _geometry(lsnf, gpu_device, 128, 64, 5, 1)
    B = 100
    whole = _full(F, plan, B, F.PhiloxNoise(SEED, OFFSET, ROW0), 0.7)
    bounds = (0,) + cuts + (B,)
    parts = [_full(F, plan, b - a, F.PhiloxNoise(SEED, OFFSET, ROW0 + a), 0.7) for a, b in zip(bounds[:-1], bounds[1:])]
    for i, what in enumerate(("x", "objective", "eps", "ll")):
        assert _same_bits(torch.cat([q[i] for q in parts]), whole[i]), (setting, what)


def test_shards_of_a_large_batch_default_dispatch(lsnf, gpu_device):
    """60 000 rows on the 8-wave throughput kernel, its halves on the 4-wave one: what a wave computes does not depend on the
    workgroup shape, so the union of the shards is the one-GPU call, bit for bit."""
    F = lsnf.flow
    p, plan = _geometry(lsnf, gpu_device, 128, 64, 5, 1)
    with dispatch(F, "default"):
        whole = _full(F, plan, 60000, F.PhiloxNoise(7, 3, 0))
        parts = [_full(F, plan, 30000, F.PhiloxNoise(7, 3, a)) for a in (0, 30000)]
    for i, what in enumerate(("x", "objective", "eps", "ll")):
        assert _same_bits(torch.cat([q[i] for q in parts]), whole[i]), what


# ------------------------------------------------------------------------------------------------- 5. call forms
@pytest.mark.parametrize("nz,w,B", [(128, 64, 130), (100, 64, 77), (126, 127, 33)])
def test_null_optionals_and_misaligned_buffers(lsnf, setting, gpu_device, nz, w, B):
    F = lsnf.flow
    _, plan = _geometry(lsnf, gpu_device, nz, w, 5, 1)
    ph = F.PhiloxNoise(SEED, OFFSET, ROW0)
    full = _full(F, plan, B, ph, 0.7)
    f32 = dict(dtype=torch.float32, device=gpu_device)
    for keep in itertools.product((False, True), repeat=3):
        out = (torch.empty(B, nz, **f32),) + tuple((torch.full((B, nz) if i == 1 else (B,), 7.0, **f32) if k else None)
                                                   for i, k in enumerate(keep))
        got = F.sample(plan, B, ph, temperature=0.7, out=out)
        assert _same_bits(got[0], full[0]), keep
        for i, k in enumerate(keep):
            assert (got[i + 1] is None) if not k else _same_bits(got[i + 1], full[i + 1]), (keep, i)
    # every (B, nz) / (B) buffer 4 bytes off a 16-byte boundary, guarded by sentinels on both sides
    def off4(shape):
        n = int(np.prod(shape))
        buf = torch.full((n + 8,), 7.0, **f32)
        assert buf.data_ptr() % 16 == 0
        return buf, buf[1:1 + n].view(shape)
    bufs = [off4(s) for s in ((B, nz), (B,), (B, nz), (B,))]
    got = F.sample(plan, B, ph, temperature=0.7, out=tuple(v for _, v in bufs))
    for i in range(4):
        assert got[i].data_ptr() % 16 == 4 and _same_bits(got[i], full[i]), i
        raw = bufs[i][0]
        assert raw[0].item() == 7.0 and bool((raw[1 + got[i].numel():] == 7.0).all()), i


def test_empty_batch_and_refused_arguments(lsnf, setting, gpu_device):
    F, E = lsnf.flow, lsnf.LsnfError
    _, plan = _geometry(lsnf, gpu_device, 128, 64, 5, 1)
    ph = F.PhiloxNoise(SEED, OFFSET, ROW0)
    x, obj, eps, ll = _full(F, plan, 0, ph)
    assert x.shape == (0, 128) and obj.shape == (0,) and eps.shape == (0, 128) and ll.shape == (0,)
    B = 33
    f32 = dict(dtype=torch.float32, device=gpu_device)
    ok = lambda: (torch.empty(B, 128, **f32), torch.empty(B, **f32), torch.empty(B, 128, **f32), torch.empty(B, **f32))
    F.sample(plan, B, ph, out=ok())
    with pytest.raises(E):
        F.sample(plan, B, None)
    with pytest.raises(E):
        F.sample(plan, B, F.PhiloxNoise(SEED, OFFSET, -1))
    for T in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(E):
            F.sample(plan, B, ph, temperature=T)
    o = ok()
    with pytest.raises(E):
        F.sample(plan, B, ph, out=(o[0], o[1], o[0], o[3]))                         # eps_out == z_out
    for i, bad in ((0, torch.empty(B * 128 - 1, **f32)), (1, torch.empty(B - 1, **f32)), (2, torch.empty(B, 127, **f32)),
                   (3, torch.empty(B - 1, **f32)), (0, torch.empty(B, 128)), (3, torch.empty(B)),
                   (2, torch.empty(B, 128, dtype=torch.float64, device=gpu_device)), (1, torch.empty(2 * B, **f32)[::2])):
        o = list(ok())
        o[i] = bad
        with pytest.raises(E):
            F.sample(plan, B, ph, out=tuple(o))
    for od in (torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32, device=gpu_device),
               torch.zeros(2, dtype=torch.int64, device=gpu_device)):
        with pytest.raises(E):
            F.sample(plan, B, F.PhiloxNoise(SEED, OFFSET, 0, offset_dev=od))
    # the C entry point itself (no Python check in front)
    lib = lsnf.load_library()
    o = ok()
    c = ph._c()
    head = (ctypes.c_void_p(plan.buf.data_ptr()), 128, 64, 5, 1, B)
    tail = tuple(ctypes.c_void_p(t.data_ptr()) for t in o) + (None,)
    assert lib.lsnf_sample(*head, None, 1.0, *tail) == -1
    assert lib.lsnf_sample(*head, ctypes.byref(c), 1.0, tail[0], tail[1], tail[0], tail[3], None) == -1
    assert lib.lsnf_sample(*head, ctypes.byref(c), -1.0, *tail) == -1


# ------------------------------------------------------------------------------------------------- 6. full size
def test_full_size_rows_and_moments(lsnf, gpu_device):
    F = lsnf.flow
    nz, B = 128, 65536
    p, plan = _geometry(lsnf, gpu_device, nz, 64, 5, 1)
    with dispatch(F, "default"):
        x, obj, eps, ll = _full(F, plan, B, F.PhiloxNoise(SEED, OFFSET, ROW0))
        eps2 = _full(F, plan, B, F.PhiloxNoise(SEED, OFFSET + 1, ROW0))[2]
    idx = torch.arange(3, B, 1021)
    ref = torch.cat([S.draws(1, nz, SEED, OFFSET, ROW0 + int(r)) for r in idx])
    e_rows = eps[idx.to(gpu_device)].cpu()
    assert (e_rows.double() - ref).abs().max().item() <= PHILOX
    x64, obj64, ll64 = S.flow_at(p, e_rows)
    scale = max(1.0, x64.abs().max().item())
    ex = (x[idx.to(gpu_device)].cpu().double() - x64).abs().max().item() / scale
    el = _rel(ll[idx.to(gpu_device)].cpu(), ll64)
    print(f"full size: x err {ex:.3e} (allowed {REV_X:.1e}), ll err {el:.3e} (allowed {LL_REL:.1e})")
    assert ex <= REV_X and el <= LL_REL
    assert _rel(ll, _own_outputs_ll(eps, obj)) <= LL_REL
    # Gaussian moments of the N = B * nz draws: six standard errors of each estimator
    N = B * nz
    e = eps.double()
    mean, var = e.mean().item(), e.var(unbiased=False).item()
    col = e.mean(0).abs().max().item()
    corr = (e * eps2.double()).mean().item()
    print(f"moments: mean {mean:.3e} (6/sqrt N = {6 / math.sqrt(N):.3e}), var-1 {var - 1:.3e} ({6 * math.sqrt(2 / N):.3e}), "
          f"max |column mean| {col:.3e} ({6 / math.sqrt(B):.3e}), offset correlation {corr:.3e}")
    assert abs(mean) <= 6 / math.sqrt(N)
    assert abs(var - 1.0) <= 6 * math.sqrt(2.0 / N)
    assert col <= 6 / math.sqrt(B)
    assert abs(corr) <= 6 / math.sqrt(N)
    assert torch.unique(eps, dim=0).shape[0] == B                                   # no two rows are equal


# ------------------------------------------------------------------------------------------------- 7. one captured graph
def test_captured_graph_advances_its_own_offset(lsnf, setting, gpu_device):
    """A single-stream chain (the sample launch, then an increment of the offset_dev counter) replayed twice draws what the
    eager calls at offset and offset + 1 draw."""
    F = lsnf.flow
    B, nz = 130, 128
    p, plan = _geometry(lsnf, gpu_device, nz, 64, 5, 1)
    f32 = dict(dtype=torch.float32, device=gpu_device)
    ctr = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    ph = F.PhiloxNoise(SEED, OFFSET, ROW0, offset_dev=ctr)
    out = (torch.empty(B, nz, **f32), torch.empty(B, **f32), torch.empty(B, nz, **f32), torch.empty(B, **f32))
    eager = [_full(F, plan, B, F.PhiloxNoise(SEED, OFFSET + k, ROW0)) for k in (0, 1)]
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        F.sample(plan, B, ph, out=out)               # (warm-up off the capture: the kernel's LDS attribute is set on first use)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        F.sample(plan, B, ph, out=out)
        ctr.add_(1)
    ctr.zero_()
    for k in (0, 1):
        graph.replay()
        torch.cuda.synchronize()
        for i in range(4):
            assert _same_bits(out[i], eager[k][i]), (setting, k, i)
    assert int(ctr.item()) == 2


# ------------------------------------------------------------------------------------------------- 8. the module
def make_net(lsnf, dev, name="c3_nz128_w64_B200"):
    p, g = load_golden(name)
    nz, w, d = int(g["meta_nz"]), int(g["meta_width"]), int(g["meta_depth"])
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=d, f_flow_permutation=2, f_width=w, f_flow_coupling=int(g.get("meta_coupling", 1)))
    net = lsnf._netF(hps, nz=nz)
    net.load_state_dict(p, strict=True)
    return net.to(dev), nz, d


def test_module_sample_no_grad_is_flow_sample(lsnf, setting, gpu_device):
    F = lsnf.flow
    net, nz, _ = make_net(lsnf, gpu_device)
    ph = F.PhiloxNoise(SEED, OFFSET, ROW0)
    ref = _full(F, net._plan(), 130, ph, 0.7)
    with torch.no_grad():
        x, eps, lp = net.sample(130, ph, temperature=0.7, return_eps=True, return_log_prob=True)
        only_x = net.sample(130, ph, temperature=0.7)
        x2, lp2 = net.sample(130, ph, temperature=0.7, return_log_prob=True)
    assert (ph.seed, ph.offset, ph.row0) == (SEED, OFFSET, ROW0)                    # the generator is not advanced
    assert _same_bits(x, ref[0]) and _same_bits(eps, ref[2]) and _same_bits(lp, ref[3])
    assert _same_bits(only_x, ref[0]) and _same_bits(x2, ref[0]) and _same_bits(lp2, ref[3])
    assert not x.requires_grad and not lp.requires_grad
    for q in net.parameters():
        q.requires_grad_(False)
    x3, lp3 = net.sample(130, ph, temperature=0.7, return_log_prob=True)             # nothing requires grad: the same single launch
    assert _same_bits(x3, ref[0]) and _same_bits(lp3, ref[3]) and x3.grad_fn is None
    seeded = net.sample(130, 1234, return_eps=True)[1]
    assert _same_bits(seeded, _full(F, net._plan(), 130, F.PhiloxNoise(1234))[2])


def _grads_two_ways(lsnf, dev, B):
    """{name: grad} of loss(x, log_prob) through netF.sample, and of the same loss through the reverse bridge fed the returned eps."""
    F = lsnf.flow
    net, nz, depth = make_net(lsnf, dev)
    gen = torch.Generator().manual_seed(B)
    gx, gl = torch.randn(B, nz, generator=gen).to(dev), torch.randn(B, generator=gen).to(dev)
    ph = F.PhiloxNoise(SEED, OFFSET, ROW0)
    x, eps, lp = net.sample(B, ph, return_eps=True, return_log_prob=True)
    assert x.requires_grad and lp.requires_grad and not eps.requires_grad
    ((x * gx).sum() + (lp * gl).sum()).backward()
    a = {k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None}
    net.zero_grad(set_to_none=True)
    x2, negobj = net(eps, objective=torch.zeros(B, device=dev), reverse=True, return_obj=True)
    lp2 = -0.5 * (eps ** 2).sum(1) + math.log(2 * math.pi) + negobj
    assert _same_bits(x2, x)
    ((x2 * gx).sum() + (lp2 * gl).sum()).backward()
    b = {k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None}
    live = [k for k in a if O.is_live_param(k) and not k.endswith(".bias")]
    assert len(live) == 12 * depth and set(a) == set(b)
    return a, b, live


def test_module_sample_parameter_gradients_are_the_reverse_bridge_s(lsnf, gpu_device):
    with dispatch(lsnf.flow, "default"):
        a, b, live = _grads_two_ways(lsnf, gpu_device, 100)
        for k in live:
            assert bool(torch.isfinite(a[k]).all()) and a[k].abs().max().item() > 0 and _same_bits(a[k], b[k]), k
        a, b, live = _grads_two_ways(lsnf, gpu_device, 20000)
        for k in live:
            spread = ((a[k].double() - b[k].double()).norm() / b[k].double().norm()).item()
            assert spread <= TOL_RUN, (k, spread)


def test_module_sample_refuses_a_stale_backward_and_sample_x_advances(lsnf, gpu_device):
    F = lsnf.flow
    net, nz, _ = make_net(lsnf, gpu_device)
    opt = torch.optim.SGD(net.parameters(), lr=1e-9)          # (any step moves the parameters' version counters)
    ph = F.PhiloxNoise(SEED, OFFSET, ROW0)
    x, lp = net.sample(64, ph, return_log_prob=True)
    (x.sum() + lp.sum()).backward()
    opt.step()                                       # the parameters move between the next forward and its backward
    x, lp = net.sample(64, ph, return_log_prob=True)
    opt.step()
    with pytest.raises(lsnf.LsnfError):
        (x.sum() + lp.sum()).backward()
    netG = torch.nn.Flatten()
    want = net.sample(64, ph).detach()
    got = lsnf.langevin.sample_x(netG, net, 64, ph, temperature=1.0)
    assert ph.offset == OFFSET + 1 and (ph.seed, ph.row0) == (SEED, ROW0)
    assert got.shape == (64, nz) and _same_bits(got, want) and not got.requires_grad and bool(torch.isfinite(got).all())
    nxt = lsnf.langevin.sample_x(netG, net, 64, ph)
    assert ph.offset == OFFSET + 2 and bool(torch.isfinite(nxt).all()) and not _same_bits(nxt, got)

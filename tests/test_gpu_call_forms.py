"""GPU: every call form that include/lsnf_flow.h documents for the z-side entry points (lsnf_forward, lsnf_reverse,
lsnf_backward_z, lsnf_langevin_step) and the "NULL entry skips that tensor" form of lsnf_backward_params.

The dispatcher (csrc/lsnf_api.hip) reads the very arguments that make up these forms -- pointer identity, pointer alignment,
first_block / n_blocks, NULL optionals -- to pick a kernel and the vector width of its row accesses, so every form is held to
two anchors:
  (a) the float64 oracle (oracle.flow_oracle on to_dtype(p, float64)) on the WHOLE batch: no row mask, no sampled subset
      (batches come from oracle.smooth_batch, so the fp32 gradient of every row is well defined);
  (b) bit equality with the plain form of the same call (fresh, 16-byte aligned buffers, whole stack) wherever the same
      arithmetic must run.
Tolerances are the ones the suite already holds on whole batches (names say where each comes from); none is new.

Sizes: the small set runs under the `kernels` fixture (both kernel families x every arithmetic mode); the default-dispatch set
runs under LSNF_SMALL_BATCH_AUTO in all four arithmetic modes at 5 000 / 14 000 / 20 000 / 40 001 rows (32- and 64-row latency
workgroups, the stash-less forward's 8 192 and the reverse's 24 576 crossover, 4- and 8-wave throughput kernels with a ragged
last tile), a padded feature tile (nz 104, width 48, depth 3) and additive coupling.  The oracle of one (geometry, batch) is a
module-scoped fixture: pytest runs all tests of one batch next to each other and the oracle is evaluated once per batch."""
import contextlib
import ctypes
import types

import pytest
import torch

from oracle import flow_oracle as O
from oracle.philox_oracle import langevin_noise

pytestmark = pytest.mark.gpu

LL_REL = 1e-5        # forward: logdet / ll, relative per row (tests/test_gpu_forward.py)
Z_ABS = 1e-4         # forward: z_out, absolute (tests/test_gpu_forward.py)
REV_X = 5e-5         # reverse: x, of max|x| (tools/fuzz_parity.py)
REV_OBJ = 2e-5       # reverse: objective, of max|objective| (tools/fuzz_parity.py)
TOL_GZ = 1e-5        # dL/dz: relative L2 over the batch (tests/test_gpu_param_grads_oracle.py)
GZ_ELEM = 2e-4       # dL/dz per element, of max|ref| (tools/fuzz_parity.py grad_z)
LANGEVIN_Z = 2e-5    # Langevin z, of max|z_ref| (tools/fuzz_parity.py)
PHILOX = 1e-4        # in-kernel N(0,1) draws recovered as (z_rng - z_nonoise) / s (tests/test_gpu_langevin.py)
TOL = 2e-5           # parameter gradients: relative L2 per tensor (tests/test_gpu_param_grads_oracle.py)
TOL_RUN = 2e-6       # parameter gradients: two runs through fp32 atomics (tests/test_gpu_param_grads_oracle.py)
STEP = 0.1
SENTINEL = 7.0
PAD = 64             # floats of sentinel on either side of a guarded tensor (256 bytes: keeps the 16-byte phase)
NAN = float("nan")

# (nz, width, depth, coupling, B)
SMALL = [(128, 64, 5, 1, 77), (128, 64, 5, 1, 130), (128, 64, 5, 0, 130), (100, 64, 5, 1, 77), (100, 64, 5, 1, 130),
         (20, 10, 5, 1, 77), (20, 10, 5, 1, 130)]
DEFAULT = [(128, 64, 5, 1, 5000), (128, 64, 5, 1, 14000), (128, 64, 5, 1, 20000), (128, 64, 5, 0, 20000),
           (128, 64, 5, 1, 40001), (104, 48, 3, 1, 40001)]
SKIP = [(128, 64, 5, 1, 100), (128, 64, 5, 1, 5000), (128, 64, 5, 0, 5000), (128, 64, 5, 1, 20000)]
MODES = {"BF16X3": "MATH_BF16X3", "BF16X3_PHASED": "MATH_BF16X3_PHASED", "FP16X2": "MATH_FP16X2", "FP32": "MATH_FP32"}
# 64-bit generator arguments (LsnfRng): the batch straddles the 32-bit row boundary, the seed has its top bit set, the offset's
# low word is all ones under a non-zero high word -- every term of the counter word (offset >> 32) ^ (row >> 32) is live
PHILOX_SEED = 2 ** 63 + 12345
PHILOX_OFFSET = (2 ** 32 - 1) + (5 << 32)
ROW0_STRADDLE = 2 ** 32 - 7
ROW0_FAR = 2 ** 40 + 3


def _case_id(c):
    nz, width, depth, coupling, B = c
    return f"nz{nz}-w{width}-d{depth}-{'affine' if coupling else 'additive'}-B{B}"


@pytest.fixture(scope="module")
def lsnf():
    import lsnf_amd
    lsnf_amd.load_library()
    return lsnf_amd


def _params(nz, width, depth, coupling):
    p = O.init_params(nz, width, depth, seed=3)
    if coupling == 0:                    # additive: fc_zeros maps to the nz/2 shifts only (model.py:385)
        for i in range(depth):
            for k in ("f.fc_zeros.w", "f.fc_zeros.b", "f.fc_zeros.logs"):
                p[O.block_prefix(i) + k] = p[O.block_prefix(i) + k][:, : nz // 2].contiguous()
    return p


class Ref:
    """One (geometry, batch): seeded parameters, a smooth batch, upstream gradients / generator gradient / noise, and the
    float64 oracle of every quantity the tests compare -- on the CPU here, moved to the GPU (float64) by `on()` so that
    whole-batch comparisons cost no transfer."""

    def __init__(self, nz, width, depth, coupling, B):
        self.nz, self.width, self.depth, self.coupling, self.B = nz, width, depth, coupling, B
        self.p = _params(nz, width, depth, coupling)
        self.z, _ = O.smooth_batch(self.p, B, nz, seed=B)
        gen = torch.Generator().manual_seed(B + 1)
        self.obj = torch.randn(B, generator=gen)
        self.gz1 = torch.randn(B, nz, generator=gen)
        self.gld = torch.randn(B, generator=gen)
        self.gg = torch.randn(B, nz, generator=gen)
        self.noise = torch.randn(B, nz, generator=gen)
        self.p64 = O.to_dtype(self.p, torch.float64)
        zz = self.z.double().requires_grad_(True)
        z1, ld = O.flow_forward(self.p64, zz, self.obj.double(), coupling)
        ll = O.log_prob(z1, ld)
        (g_ll,) = torch.autograd.grad(-ll.sum(), zz, retain_graph=True)                       # d(-sum ll)/dz
        (g_a,) = torch.autograd.grad((z1 * self.gz1.double()).sum(), zz, retain_graph=True)   # upstream g_z1 alone
        # upstream g_logdet alone (additive coupling: logdet does not depend on z, the gradient is exactly zero)
        g_b = torch.autograd.grad((ld * self.gld.double()).sum(), zz)[0] if coupling else torch.zeros_like(g_a)
        x, negobj = O.flow_reverse(self.p64, self.z.double(), self.obj.double(), coupling)
        self.cpu = dict(z1=z1.detach(), ld=ld.detach(), ll=ll.detach(), g_ll=g_ll, g_a=g_a, g_b=g_b, x=x, xobj=-negobj)
        self._gpu = None
        self._draws = {}
        self._param_grads = None

    def on(self, F, dev):
        """Everything on the device: fp32 inputs, float64 references, the plan (which serves every arithmetic mode)."""
        if self._gpu is None:
            g = types.SimpleNamespace(R=self, dev=dev)
            g.params = F.params_from_state_dict(self.p, self.depth, dev)
            g.plan = F.prepare(g.params, self.nz, self.width, self.depth, self.coupling)
            for k in ("z", "obj", "gz1", "gld", "gg", "noise"):
                setattr(g, k, getattr(self, k).to(dev))
            g.ref = types.SimpleNamespace(**{k: v.to(dev) for k, v in self.cpu.items()})
            self._gpu = g
        return self._gpu

    def draws(self, dev, row0):
        """float64 (B, nz) on the device: oracle.philox_oracle's draws for (PHILOX_SEED, PHILOX_OFFSET, row0)."""
        if row0 not in self._draws:
            n = langevin_noise(self.B, self.nz, PHILOX_SEED, PHILOX_OFFSET, row0)
            assert bool((n == n).all()) and float(abs(n).max()) < 10.0
            self._draws[row0] = torch.from_numpy(n).to(dev)
        return self._draws[row0]

    def param_grads(self):
        """{key: d(-mean ll)/dtheta} in float64 (the forward is given `obj`, which does not enter any gradient)."""
        if self._param_grads is None:
            self._param_grads = O.grad_neg_mean_ll_wrt_params(self.p64, self.z.double(), self.coupling)
        return self._param_grads


@pytest.fixture(scope="module", params=SMALL, ids=[_case_id(c) for c in SMALL])
def small_ref(request):
    return Ref(*request.param)


@pytest.fixture(scope="module", params=DEFAULT, ids=[_case_id(c) for c in DEFAULT])
def default_ref(request):
    return Ref(*request.param)


@pytest.fixture(scope="module", params=SKIP, ids=[_case_id(c) for c in SKIP])
def skip_ref(request):
    return Ref(*request.param)


@contextlib.contextmanager
def _settings(F, small, mode):
    prev_small, prev_mode = F.set_small_batch_max(small), F.set_math_mode(mode)
    try:
        yield
    finally:
        F.set_small_batch_max(prev_small)
        F.set_math_mode(prev_mode)


@pytest.fixture(params=list(MODES))
def dispatch(request, lsnf):
    """The default dispatch (LSNF_SMALL_BATCH_AUTO) in one of the four arithmetic modes."""
    with _settings(lsnf.flow, lsnf.flow.SMALL_BATCH_AUTO, getattr(lsnf.flow, MODES[request.param])):
        yield request.param


def _throughput(F, B):
    """Is a batch of B rows above the small-batch threshold in force (throughput kernels)?"""
    return B > F.set_small_batch_max(-1)


def _fp16_kernels(F, B):
    """Does the two-term fp16 forward / reverse (with its bf16x3 fix-up pass) take plain calls of B rows?"""
    return F.set_math_mode(-1) == F.MATH_FP16X2 and _throughput(F, B)


def _wg_rows(row, B):
    """Rows of the workgroup (256 rows above 32 768, else 128) that holds `row`: the fp16 fix-up pass's unit of recomputation."""
    per = 256 if B > 128 * 256 else 128
    lo = (row // per) * per
    return slice(lo, min(lo + per, B))


# ---- comparisons -------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Bit equality (NaN words included)."""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _max_rel(got, ref):
    """max|got - ref| / max|ref| (tools/fuzz_parity.py `rel`)."""
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _l2_rel(got, ref):
    return ((got.double() - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def _assert_forward(G, z1, ld, ll, what):
    r = G.ref
    assert bool(torch.isfinite(z1).all() and torch.isfinite(ld).all()), what
    e_z = (z1.double() - r.z1).abs().max().item()
    e_ld = ((ld.double() - r.ld).abs() / r.ld.abs().clamp_min(1.0)).max().item()
    assert e_z <= Z_ABS * max(1.0, r.z1.abs().max().item()), (what, "z_out", e_z)
    assert e_ld <= LL_REL, (what, "logdet", e_ld)
    if ll is not None:
        e_ll = ((ll.double() - r.ll).abs() / r.ll.abs().clamp_min(1.0)).max().item()
        assert e_ll <= LL_REL, (what, "ll", e_ll)


def _assert_reverse(G, x, xobj, what):
    assert bool(torch.isfinite(x).all() and torch.isfinite(xobj).all()), what
    e_x, e_o = _max_rel(x, G.ref.x), _max_rel(xobj, G.ref.xobj)
    assert e_x <= REV_X and e_o <= REV_OBJ, (what, e_x, e_o)


def _assert_grad(got, ref, what):
    assert bool(torch.isfinite(got).all()), what
    if not bool(ref.any()):                      # (d logdet/dz of an additive stack: nothing to be relative to)
        assert not bool(got.any()), what
        return
    e_l2, e_el = _l2_rel(got, ref), _max_rel(got, ref)
    assert e_l2 <= TOL_GZ and e_el <= GZ_ELEM, (what, e_l2, e_el)


def _langevin_ref(G, gg, noise64):
    """train.py:324,326 in float64: z - 0.5 s^2 (grad_g + g_f) [+ s noise]."""
    g = G.ref.g_ll if gg is None else G.ref.g_ll + gg.double()
    z = G.z.double() - 0.5 * STEP * STEP * g
    return z if noise64 is None else z + STEP * noise64


def _assert_langevin(G, z_new, gg, noise64, what):
    ref = _langevin_ref(G, gg, noise64)
    assert bool(torch.isfinite(z_new).all()), what
    e = _max_rel(z_new, ref)
    assert e <= LANGEVIN_Z, (what, e)


def _assert_norms(G, gf, gg_norm, gg, what):
    """Per-row norms (train.py:328-329).  ||(|a_b|)_b - (|r_b|)_b||_2 <= ||a - r||_F (reverse triangle inequality row by row), so
    the vector of row norms inherits the gradient's own whole-batch bound TOL_GZ; no tolerance of its own is needed."""
    e = _l2_rel(gf, G.ref.g_ll.norm(dim=1))
    assert e <= TOL_GZ, (what, "gf_norm", e)
    if gg is not None:
        e = _l2_rel(gg_norm, gg.double().norm(dim=1))
        assert e <= TOL_GZ, (what, "gg_norm", e)


# ---- buffers -----------------------------------------------------------------------------------------------------------
class Guarded:
    """A contiguous tensor `off` floats past a 16-byte boundary, in the middle of a sentinel-filled allocation: the pointer the
    ABI sees is 4 * off bytes off alignment, and a store before or behind the tensor lands on a sentinel."""

    def __init__(self, shape, dev, off=0, src=None, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.n, self.off = n, off
        self.buf = torch.full((PAD + off + n + PAD,), SENTINEL, dtype=torch.float32, device=dev)
        self.t = self.buf[PAD + off: PAD + off + n].view(shape)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 4 * off
        if src is not None:
            self.t.copy_(src)
        elif fill is not None:
            self.t.fill_(fill)

    def untouched(self):
        lo, hi = self.buf[: PAD + self.off], self.buf[PAD + self.off + self.n:]
        return bool((lo == SENTINEL).all() and (hi == SENTINEL).all())


def _new_stash(F, G, n_saved=None):
    """NaN-filled act_saved / z_saved: every word a reader uses must have been written by the forward."""
    R = G.R
    act = F.new_act_saved(G.plan, R.B, G.dev)
    act.fill_(NAN)
    n_saved = R.depth - 1 if n_saved is None else n_saved
    saved = torch.full((n_saved, R.B, R.nz), NAN, device=G.dev) if n_saved > 0 else None
    return act, saved


def _forward(F, G, stash, z=None, obj=None):
    """The plain form: fresh, 16-byte aligned buffers, the whole stack."""
    act, saved = _new_stash(F, G) if stash else (None, None)
    z1, ld, ll, _ = F.forward(G.plan, G.z if z is None else z, G.obj if obj is None else obj, act_saved=act, z_saved_out=saved)
    return types.SimpleNamespace(z1=z1, ld=ld, ll=ll, saved=saved, act=act)


def _raw_backward_z(F, G, z_out, saved, act, g_z1, g_ld, ll_scale, g_in):
    """lsnf_backward_z exactly as given (flow.backward_z allocates its output and rebuilds a missing stash first)."""
    p = G.plan
    with torch.cuda.device(G.dev):
        rc = F._lib.load().lsnf_backward_z(F._ptr(p.buf), p.nz, p.width, p.depth, p.coupling, z_out.shape[0], F._ptr(z_out),
                                           F._ptr(saved), F._ptr(act), F._ptr(g_z1), F._ptr(g_ld), 0 if ll_scale is None else 1,
                                           float(ll_scale or 0.0), F._ptr(g_in), F._stream_ptr(G.dev))
    F._lib.check(rc, "lsnf_backward_z")
    return g_in


def _raw_langevin(F, G, z_cur, z1, saved, act, gg, noise, rng, z_new, gf=None, gg_norm=None):
    """lsnf_langevin_step on the outputs of a forward the caller ran (flow.langevin_step runs its own)."""
    p = G.plan
    with torch.cuda.device(G.dev):
        rc = F._lib.load().lsnf_langevin_step(F._ptr(p.buf), p.nz, p.width, p.depth, p.coupling, z_cur.shape[0], F._ptr(z_cur),
                                              F._ptr(z1), F._ptr(saved), F._ptr(act), F._ptr(gg), F._ptr(noise),
                                              None if rng is None else ctypes.byref(rng._c()), STEP, F._ptr(z_new), F._ptr(gf),
                                              F._ptr(gg_norm), F._stream_ptr(G.dev))
    F._lib.check(rc, "lsnf_langevin_step")
    return z_new


def _offset_variants(names):
    """Each row tensor of a call in turn at +4 and at +8 bytes, then all of them at once."""
    return [{n: o} for n in names for o in (1, 2)] + [{n: o for n in names} for o in (1, 2)]


# ---- form 1: forward in place ---------------------------------------------------------------------------------------------
def _check_forward_in_place(F, G):
    """z_out == z_in and / or logdet_out == objective.  select_forward names the same kernel as for the out-of-place call in every
    mode but one: above the threshold LSNF_MATH_FP16X2 hands an aliased call (either alias: the fix-up pass re-reads both
    inputs) to lsnf_fwd3b_kernel, the forward of LSNF_MATH_BF16X3_PHASED -- so z_out, logdet and ll are bit-equal to that
    mode's out-of-place results (whose z_out rows are also LSNF_MATH_BF16X3's), and z_out is NOT the fp16 kernel's."""
    R = G.R
    fp16 = _fp16_kernels(F, R.B)
    for stash in (False, True):
        plain = _forward(F, G, stash)
        _assert_forward(G, plain.z1, plain.ld, plain.ll, ("plain", stash))
        expect = plain
        if fp16:
            with _settings(F, 0, F.MATH_BF16X3_PHASED):
                expect = _forward(F, G, stash)
            with _settings(F, 0, F.MATH_BF16X3):
                x3 = _forward(F, G, stash)
            assert _same(x3.z1, expect.z1)
            if (R.nz, R.width) == (128, 64):
                assert not _same(plain.z1, expect.z1)          # the fp16 kernel did take the plain call
        for alias in ("both", "z", "objective"):
            zc, oc = G.z.clone(), G.obj.clone()
            z_out = zc if alias in ("both", "z") else torch.empty_like(zc)
            ld_out = oc if alias in ("both", "objective") else torch.empty_like(oc)
            ll = torch.empty_like(oc)
            act, saved = _new_stash(F, G) if stash else (None, None)
            F.forward(G.plan, zc, objective=oc, out=(z_out, ld_out, ll), act_saved=act, z_saved_out=saved)
            what = ("in place", alias, "stash" if stash else "no stash")
            _assert_forward(G, z_out, ld_out, ll, what)
            assert _same(z_out, expect.z1) and _same(ld_out, expect.ld) and _same(ll, expect.ll), what
            assert _same(saved, expect.saved) and _same(act, expect.act), what
            if fp16 and not _same(plain.z1, expect.z1):
                assert not _same(z_out, plain.z1), what
            if alias == "objective":
                assert _same(zc, G.z), what                    # an input that is not aliased is not modified
            if alias == "z":
                assert _same(oc, G.obj), what
            if stash:
                gz = F.backward_z(G.plan, z_out, saved, ll_scale=-1.0, act_saved=act)
                _assert_grad(gz, G.ref.g_ll, what)


def test_forward_in_place_small(lsnf, kernels, gpu_device, small_ref):
    _check_forward_in_place(lsnf.flow, small_ref.on(lsnf.flow, gpu_device))


def test_forward_in_place_default_dispatch(lsnf, dispatch, gpu_device, default_ref):
    _check_forward_in_place(lsnf.flow, default_ref.on(lsnf.flow, gpu_device))


# ---- form 2: reverse in place ---------------------------------------------------------------------------------------------
def _check_reverse_in_place(F, G):
    """z_out == z_in and / or objective_out == objective.  As in the forward, only LSNF_MATH_FP16X2 above the threshold selects
    another kernel for an aliased call: lsnf_rev3_kernel, the throughput reverse of LSNF_MATH_BF16X3 -- bit-equal to that mode's
    out-of-place results with the latency kernels off, and not the fp16 kernel's rows."""
    R = G.R
    fp16 = _fp16_kernels(F, R.B)
    plain = F.reverse(G.plan, G.z, G.obj)
    _assert_reverse(G, plain[0], plain[1], "plain")
    expect = plain
    if fp16:
        with _settings(F, 0, F.MATH_BF16X3):
            expect = F.reverse(G.plan, G.z, G.obj)
        if (R.nz, R.width) == (128, 64):
            assert not _same(plain[0], expect[0])              # the fp16 kernel did take the plain call
    for alias in ("both", "z", "objective"):
        zc, oc = G.z.clone(), G.obj.clone()
        z_out = zc if alias in ("both", "z") else torch.empty_like(zc)
        o_out = oc if alias in ("both", "objective") else torch.empty_like(oc)
        got = F.reverse(G.plan, zc, oc, out=(z_out, o_out))
        assert got[0] is z_out and got[1] is o_out
        _assert_reverse(G, z_out, o_out, ("in place", alias))
        assert _same(z_out, expect[0]) and _same(o_out, expect[1]), alias
        if fp16 and not _same(plain[0], expect[0]):
            assert not _same(z_out, plain[0]), alias
        if alias == "objective":
            assert _same(zc, G.z)
        if alias == "z":
            assert _same(oc, G.obj)
    x, xo = F.reverse(G.plan, G.z, None)                        # objective is the one optional argument of lsnf_reverse
    assert _same(x, plain[0]) and _max_rel(xo, G.ref.xobj - G.obj.double()) <= REV_OBJ


def test_reverse_in_place_small(lsnf, kernels, gpu_device, small_ref):
    _check_reverse_in_place(lsnf.flow, small_ref.on(lsnf.flow, gpu_device))


def test_reverse_in_place_default_dispatch(lsnf, dispatch, gpu_device, default_ref):
    _check_reverse_in_place(lsnf.flow, default_ref.on(lsnf.flow, gpu_device))


# ---- form 3: the stack in pieces, with a stash ---------------------------------------------------------------------------
def _splits(depth):
    cands = [[(0, 2), (2, depth)], [(0, 1), (1, depth - 1), (depth - 1, depth)], [(i, i + 1) for i in range(depth)]]
    out = []
    for s in cands:
        s = [(a, b) for a, b in s if b > a]
        if s not in out and s[-1][1] == depth and all(x[1] == y[0] for x, y in zip(s, s[1:])):
            out.append(s)
    return out


def _check_stack_in_pieces(F, G):
    """The stash is indexed by absolute block: a stack run in pieces (each piece its own z_saved, all of them one act_saved,
    objective chained) leaves the block outputs and the stash of the whole-stack launch, bit for bit -- every block runs the same
    arithmetic on the same fp32 input whichever launch it is part of, in both kernel families and every mode (the pipelined and
    the phase-separated forward already agree on these words).  logdet / ll are sums taken in another order: oracle bound only."""
    R = G.R
    whole = _forward(F, G, True)
    _assert_forward(G, whole.z1, whole.ld, whole.ll, "whole stack")
    for split in _splits(R.depth):
        act, _ = _new_stash(F, G, 0)
        z, ld, ll, outs = G.z, G.obj, None, []
        for a, b in split:
            _, sv = _new_stash(F, G, b - a - 1)
            z, ld, ll, _ = F.forward(G.plan, z, ld, first_block=a, n_blocks=b - a, act_saved=act, z_saved_out=sv)
            outs += ([] if sv is None else list(sv)) + [z]
        assert len(outs) == R.depth
        saved = torch.stack(outs[:-1]) if R.depth > 1 else None
        _assert_forward(G, z, ld, ll, split)
        assert _same(z, whole.z1), split
        assert _same(saved, whole.saved), split
        assert _same(act, whole.act), split
        assert saved is None or bool(torch.isfinite(saved).all()), split
        gz = F.backward_z(G.plan, z, saved, ll_scale=-1.0, act_saved=act)
        _assert_grad(gz, G.ref.g_ll, split)
        assert _same(gz, F.backward_z(G.plan, whole.z1, whole.saved, ll_scale=-1.0, act_saved=whole.act)), split
        gf, ggn = torch.empty(R.B, device=G.dev), torch.empty(R.B, device=G.dev)
        zn = _raw_langevin(F, G, G.z, z, saved, act, G.gg, G.noise, None, torch.empty_like(G.z), gf, ggn)
        _assert_langevin(G, zn, G.gg, G.noise.double(), split)
        _assert_norms(G, gf, ggn, G.gg, split)


def test_stack_in_pieces_small(lsnf, kernels, gpu_device, small_ref):
    _check_stack_in_pieces(lsnf.flow, small_ref.on(lsnf.flow, gpu_device))


def test_stack_in_pieces_default_dispatch(lsnf, dispatch, gpu_device, default_ref):
    _check_stack_in_pieces(lsnf.flow, default_ref.on(lsnf.flow, gpu_device))


# ---- form 4: alignment ---------------------------------------------------------------------------------------------------
def _check_forward_alignment(F, G):
    """z_in, z_out, z_saved at +4 / +8 bytes: row_vector_width lowers the row accesses to 1 or 2 floats.  The stash-less call
    keeps its kernel (bit-equal throughout).  With a stash, LSNF_MATH_BF16X3 above the threshold hands the call from
    lsnf_fwd3q_kernel to lsnf_fwd3b_kernel (lsnf_forward3q_covers): z_out, z_saved and the stash are bit-equal all the same
    (test_pipelined_forward_writes_the_phase_separated_stash), logdet / ll are held to the oracle only."""
    R = G.R
    d3, B, nz = R.depth - 1, R.B, R.nz
    for stash in (False, True):
        base = _forward(F, G, stash)
        _assert_forward(G, base.z1, base.ld, base.ll, ("aligned", stash))
        other_kernel = stash and F.set_math_mode(-1) == F.MATH_BF16X3 and _throughput(F, B)
        names = ("z_in", "z_out") + (("z_saved",) if stash and d3 > 0 else ())
        for offs in _offset_variants(names):
            z_in = Guarded((B, nz), G.dev, offs.get("z_in", 0), src=G.z)
            z_out = Guarded((B, nz), G.dev, offs.get("z_out", 0), fill=NAN)
            ld, ll = Guarded((B,), G.dev, fill=NAN), Guarded((B,), G.dev, fill=NAN)
            saved = Guarded((d3, B, nz), G.dev, offs.get("z_saved", 0), fill=NAN) if stash and d3 > 0 else None
            act = _new_stash(F, G, 0)[0] if stash else None
            F.forward(G.plan, z_in.t, G.obj, out=(z_out.t, ld.t, ll.t), act_saved=act,
                      z_saved_out=None if saved is None else saved.t)
            torch.cuda.synchronize()
            what = ("forward", "stash" if stash else "no stash", offs)
            assert all(g.untouched() for g in (z_in, z_out, ld, ll) + (() if saved is None else (saved,))), what
            assert _same(z_in.t, G.z), what
            _assert_forward(G, z_out.t, ld.t, ll.t, what)
            assert _same(z_out.t, base.z1), what
            if stash:
                assert _same(None if saved is None else saved.t, base.saved) and _same(act, base.act), what
            if not other_kernel:
                assert _same(ld.t, base.ld) and _same(ll.t, base.ll), what


def _check_reverse_alignment(F, G):
    R = G.R
    base = F.reverse(G.plan, G.z, G.obj)
    _assert_reverse(G, base[0], base[1], "aligned")
    for offs in _offset_variants(("z_in", "z_out")):
        z_in = Guarded((R.B, R.nz), G.dev, offs.get("z_in", 0), src=G.z)
        z_out = Guarded((R.B, R.nz), G.dev, offs.get("z_out", 0), fill=NAN)
        o_out = Guarded((R.B,), G.dev, fill=NAN)
        F.reverse(G.plan, z_in.t, G.obj, out=(z_out.t, o_out.t))
        torch.cuda.synchronize()
        assert z_in.untouched() and z_out.untouched() and o_out.untouched(), offs
        _assert_reverse(G, z_out.t, o_out.t, offs)
        assert _same(z_out.t, base[0]) and _same(o_out.t, base[1]), offs      # select_reverse does not look at alignment


def _check_backward_alignment(F, G):
    """lsnf_backward_z / lsnf_langevin_step on misaligned z_out, z_saved, g_z1, g_z_in / z_cur, grad_g, noise, z_new after a
    forward on aligned tensors (the two calls of one evaluation disagree on the vector width), and the other way round: a
    forward that wrote misaligned z_out / z_saved, read back as they are and through aligned copies.  select_backward does not
    look at alignment, so every result is bit-equal to the aligned call's."""
    R = G.R
    B, nz, d3 = R.B, R.nz, R.depth - 1
    fwd = _forward(F, G, True)
    _assert_forward(G, fwd.z1, fwd.ld, fwd.ll, "aligned forward")
    ref_up = G.ref.g_a + G.ref.g_b
    noise64 = G.noise.double()

    def backward(offs, z1, saved, act):
        a = {k: Guarded(t.shape, G.dev, offs.get(k, 0), src=t) for k, t in (("z_out", z1), ("g_z1", G.gz1))}
        if saved is not None:
            a["z_saved"] = Guarded(saved.shape, G.dev, offs.get("z_saved", 0), src=saved)
        a["g_z_in"] = Guarded((B, nz), G.dev, offs.get("g_z_in", 0), fill=NAN)
        _raw_backward_z(F, G, a["z_out"].t, a["z_saved"].t if saved is not None else None, act, a["g_z1"].t, G.gld, None,
                        a["g_z_in"].t)
        torch.cuda.synchronize()
        assert all(g.untouched() for g in a.values()), ("backward_z", offs)
        assert _same(a["z_out"].t, z1) and _same(a["g_z1"].t, G.gz1)
        return a["g_z_in"].t

    def langevin(offs, z1, saved, act):
        a = {k: Guarded(t.shape, G.dev, offs.get(k, 0), src=t)
             for k, t in (("z_cur", G.z), ("z_out", z1), ("grad_g", G.gg), ("noise", G.noise))}
        if saved is not None:
            a["z_saved"] = Guarded(saved.shape, G.dev, offs.get("z_saved", 0), src=saved)
        a["z_new"] = Guarded((B, nz), G.dev, offs.get("z_new", 0), fill=NAN)
        gf, ggn = Guarded((B,), G.dev, fill=NAN), Guarded((B,), G.dev, fill=NAN)
        _raw_langevin(F, G, a["z_cur"].t, a["z_out"].t, a["z_saved"].t if saved is not None else None, act, a["grad_g"].t,
                      a["noise"].t, None, a["z_new"].t, gf.t, ggn.t)
        torch.cuda.synchronize()
        assert all(g.untouched() for g in list(a.values()) + [gf, ggn]), ("langevin_step", offs)
        assert _same(a["z_cur"].t, G.z)
        return a["z_new"].t, gf.t, ggn.t

    for act in (fwd.act, None):                 # from the stash; recomputing kernels (NULL act_saved, exactly as given)
        g_base = backward({}, fwd.z1, fwd.saved, act)
        _assert_grad(g_base, ref_up, ("backward_z aligned", act is not None))
        l_base = langevin({}, fwd.z1, fwd.saved, act)
        _assert_langevin(G, l_base[0], G.gg, noise64, ("langevin aligned", act is not None))
        _assert_norms(G, l_base[1], l_base[2], G.gg, ("langevin aligned", act is not None))
        sv = ("z_saved",) if d3 > 0 else ()
        b_variants = _offset_variants(("z_out",) + sv + ("g_z1", "g_z_in"))
        l_variants = _offset_variants(("z_cur", "z_out") + sv + ("grad_g", "noise", "z_new"))
        if act is None:                         # (the recomputing kernels: all tensors at once only)
            b_variants, l_variants = b_variants[-2:], l_variants[-2:]
        for offs in b_variants:
            g = backward(offs, fwd.z1, fwd.saved, act)
            _assert_grad(g, ref_up, ("backward_z", offs))
            assert _same(g, g_base), ("backward_z", offs)
        for offs in l_variants:
            zn, gf, ggn = langevin(offs, fwd.z1, fwd.saved, act)
            _assert_langevin(G, zn, G.gg, noise64, ("langevin", offs))
            _assert_norms(G, gf, ggn, G.gg, ("langevin", offs))
            assert _same(zn, l_base[0]) and _same(gf, l_base[1]) and _same(ggn, l_base[2]), ("langevin", offs)
    # the other way round: the forward writes misaligned z_out / z_saved (and decides its kernel from them)
    g_base = backward({}, fwd.z1, fwd.saved, fwd.act)
    l_base = langevin({}, fwd.z1, fwd.saved, fwd.act)
    for off in (1, 2):
        z_out = Guarded((B, nz), G.dev, off, fill=NAN)
        saved = Guarded((d3, B, nz), G.dev, off, fill=NAN) if d3 > 0 else None
        act = _new_stash(F, G, 0)[0]
        F.forward(G.plan, G.z, G.obj, out=(z_out.t, torch.empty(B, device=G.dev), None), want_ll=False, act_saved=act,
                  z_saved_out=None if saved is None else saved.t)
        sv_t = None if saved is None else saved.t
        # read back in place (misaligned), and through aligned copies (the backward then runs wider rows than the forward did)
        for z1_b, sv_b in ((z_out.t, sv_t), (z_out.t.clone(), None if sv_t is None else sv_t.clone())):
            g_in = _raw_backward_z(F, G, z1_b, sv_b, act, G.gz1, G.gld, None, torch.empty_like(G.z))
            _assert_grad(g_in, ref_up, ("misaligned forward, backward_z", off))
            assert _same(g_in, g_base), off
            zn = _raw_langevin(F, G, G.z, z1_b, sv_b, act, G.gg, G.noise, None, torch.empty_like(G.z))
            _assert_langevin(G, zn, G.gg, noise64, ("misaligned forward, langevin", off))
            assert _same(zn, l_base[0]), off
        assert z_out.untouched() and (saved is None or saved.untouched())


def test_forward_alignment_small(lsnf, kernels, gpu_device, small_ref):
    _check_forward_alignment(lsnf.flow, small_ref.on(lsnf.flow, gpu_device))


def test_forward_alignment_default_dispatch(lsnf, dispatch, gpu_device, default_ref):
    _check_forward_alignment(lsnf.flow, default_ref.on(lsnf.flow, gpu_device))


def test_reverse_alignment_small(lsnf, kernels, gpu_device, small_ref):
    _check_reverse_alignment(lsnf.flow, small_ref.on(lsnf.flow, gpu_device))


def test_reverse_alignment_default_dispatch(lsnf, dispatch, gpu_device, default_ref):
    _check_reverse_alignment(lsnf.flow, default_ref.on(lsnf.flow, gpu_device))


def test_backward_and_langevin_alignment_small(lsnf, kernels, gpu_device, small_ref):
    _check_backward_alignment(lsnf.flow, small_ref.on(lsnf.flow, gpu_device))


def test_backward_and_langevin_alignment_default_dispatch(lsnf, dispatch, gpu_device, default_ref):
    _check_backward_alignment(lsnf.flow, default_ref.on(lsnf.flow, gpu_device))


# ---- form 5: upstream-gradient forms of lsnf_backward_z ------------------------------------------------------------------
def _check_upstream_gradient_forms(F, G):
    """(g_z1, g_logdet), g_z1 alone, g_logdet alone, ll_mode with ll_scale -1 and 0.37 -- from the stash and with act_saved
    NULL (the recomputing kernels) -- against autograd over the oracle in float64 (the backward is linear in its upstream)."""
    r = G.ref
    fwd = _forward(F, G, True)
    forms = [("both", G.gz1, G.gld, None, r.g_a + r.g_b), ("g_z1", G.gz1, None, None, r.g_a), ("g_logdet", None, G.gld, None, r.g_b),
             ("ll -1", None, None, -1.0, r.g_ll), ("ll 0.37", None, None, 0.37, -0.37 * r.g_ll)]
    for act in (fwd.act, None):
        for name, g_z1, g_ld, scale, ref in forms:
            got = _raw_backward_z(F, G, fwd.z1, fwd.saved, act, g_z1, g_ld, scale, torch.full_like(G.z, NAN))
            _assert_grad(got, ref, (name, "stash" if act is not None else "recompute"))


def test_upstream_gradient_forms_small(lsnf, kernels, gpu_device, small_ref):
    _check_upstream_gradient_forms(lsnf.flow, small_ref.on(lsnf.flow, gpu_device))


def test_upstream_gradient_forms_default_dispatch(lsnf, dispatch, gpu_device, default_ref):
    _check_upstream_gradient_forms(lsnf.flow, default_ref.on(lsnf.flow, gpu_device))


# ---- form 6: Langevin forms -----------------------------------------------------------------------------------------------
def _check_langevin_forms(F, G):
    """{no noise, noise tensor, in-kernel Philox} x {grad_g NULL, tensor} x {z_new == z_cur} x {gf_norm / gg_norm NULL}."""
    R = G.R
    ph = F.PhiloxNoise(PHILOX_SEED, PHILOX_OFFSET, row0=ROW0_STRADDLE)
    ll_ref = G.ref.ll - G.obj.double()
    for kind, noise, n64 in (("none", None, None), ("tensor", G.noise, G.noise.double()), ("philox", ph, R.draws(G.dev, ROW0_STRADDLE))):
        first = {}
        for gg in (None, G.gg):
            for inplace in (False, True):
                for norms in (True, False):
                    what = (kind, "grad_g" if gg is not None else "no grad_g", inplace, norms)
                    zc = G.z.clone()
                    zn, ll, gf, ggn = F.langevin_step(G.plan, zc, gg, noise, STEP, inplace=inplace, want_norms=norms)
                    assert (zn.data_ptr() == zc.data_ptr()) == inplace and (inplace or _same(zc, G.z)), what
                    _assert_langevin(G, zn, gg, n64, what)
                    assert ((ll.double() - ll_ref).abs() / ll_ref.abs().clamp_min(1.0)).max().item() <= LL_REL, what
                    if norms:
                        assert (ggn is None) == (gg is None), what
                        _assert_norms(G, gf, ggn, gg, what)
                    else:
                        assert gf is None and ggn is None, what
                    key = gg is not None                      # in place or not, norms or not: one kernel, the same z
                    assert _same(zn, first.setdefault(key, zn.clone())), what


def _check_philox_64bit(F, G):
    """LsnfRng with row0 + row crossing 2^32, row0 beyond 2^40, a seed >= 2^63 and an offset with both words live: the draws,
    recovered as (z_rng - z_nonoise) / s, against oracle.philox_oracle on the whole batch; a shard that starts at row r with
    row0 + r draws rows r.. of the unsharded call, bit for bit, below, on and past the 32-bit boundary."""
    R = G.R
    fwd = _forward(F, G, True, obj=torch.zeros_like(G.obj))
    base = _raw_langevin(F, G, G.z, fwd.z1, fwd.saved, fwd.act, G.gg, None, None, torch.empty_like(G.z))
    _assert_langevin(G, base, G.gg, None, "no noise")
    for row0 in (ROW0_STRADDLE, ROW0_FAR):
        ph = F.PhiloxNoise(PHILOX_SEED, PHILOX_OFFSET, row0=row0)
        z_rng = _raw_langevin(F, G, G.z, fwd.z1, fwd.saved, fwd.act, G.gg, None, ph, torch.empty_like(G.z))
        draws = R.draws(G.dev, row0)
        e = ((z_rng.double() - base.double()) / STEP - draws).abs().max().item()
        assert e <= PHILOX, (row0, e)
        _assert_langevin(G, z_rng, G.gg, draws, row0)
    ph = F.PhiloxNoise(PHILOX_SEED, PHILOX_OFFSET, row0=ROW0_STRADDLE)
    full = F.langevin_step(G.plan, G.z, G.gg, ph, STEP)[0]
    for r in (3, 7, 11):                                       # global rows 2^32 - 4, 2^32, 2^32 + 4
        shard = F.langevin_step(G.plan, G.z[r:].contiguous(), G.gg[r:].contiguous(),
                                F.PhiloxNoise(PHILOX_SEED, PHILOX_OFFSET, row0=ROW0_STRADDLE + r), STEP)[0]
        assert _same(shard, full[r:]), r
    # the high row word matters: the same rows 2^32 further on draw other numbers
    other = F.langevin_step(G.plan, G.z, G.gg, F.PhiloxNoise(PHILOX_SEED, PHILOX_OFFSET, row0=ROW0_STRADDLE + 2 ** 32), STEP)[0]
    assert not bool((other == full).all(dim=1).any())


def test_langevin_forms_small(lsnf, kernels, gpu_device, small_ref):
    _check_langevin_forms(lsnf.flow, small_ref.on(lsnf.flow, gpu_device))


def test_langevin_forms_default_dispatch(lsnf, dispatch, gpu_device, default_ref):
    _check_langevin_forms(lsnf.flow, default_ref.on(lsnf.flow, gpu_device))


def test_philox_64bit_counters_small(lsnf, kernels, gpu_device, small_ref):
    _check_philox_64bit(lsnf.flow, small_ref.on(lsnf.flow, gpu_device))


def test_philox_64bit_counters_default_dispatch(lsnf, dispatch, gpu_device, default_ref):
    _check_philox_64bit(lsnf.flow, default_ref.on(lsnf.flow, gpu_device))


# ---- form 7: skipped gradients --------------------------------------------------------------------------------------------
def _check_skipped_gradients(F, G, path):
    """grads_host: "a NULL entry skips that tensor".  All tensors of one block, one tensor kind in every block, all but one
    tensor: the tensors that are written equal the all-60 call's (bit for bit up to 1 024 rows, TOL_RUN above: fp32 atomics)
    and the oracle's, and the sentinel-filled slots behind the skipped entries are not touched.  path: "fast" (the forward
    keeps the stash and the h dump, the backward runs from them) or "recompute"."""
    R, dev = G.R, G.dev
    n = R.depth * 12
    keys = [O.block_prefix(i) + k for i in range(R.depth) for k in F.BLOCK_PARAM_KEYS]
    sizes = [t.numel() for t in G.params]
    ref = R.param_grads()
    patterns = {"none": set(), "one block": set(range(24, 36)), "one kind": set(range(6, n, 12)), "all but one": set(range(n)) - {27}}
    act = ws = None
    if path == "fast":
        act, _ = _new_stash(F, G, 0)
        ws = F.new_params_workspace(G.plan, R.B, dev)
        ws.fill_(NAN)
    z1, _, _, saved = F.forward(G.plan, G.z, G.obj, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
    if ws is None:
        ws = F.new_params_workspace(G.plan, R.B, dev)
    results = {}
    for name, skipped in patterns.items():
        flat = torch.full((sum(sizes),), SENTINEL, device=dev)
        views = list(flat.split(sizes))
        garr = (ctypes.c_void_p * n)(*[None if i in skipped else v.data_ptr() for i, v in enumerate(views)])
        parr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in G.params])
        p = G.plan
        with torch.cuda.device(dev):
            rc = F._lib.load().lsnf_backward_params(F._ptr(p.buf), parr, garr, p.nz, p.width, p.depth, p.coupling, R.B,
                                                    F._ptr(G.z), F._ptr(z1), F._ptr(saved), F._ptr(act), None, None, 1,
                                                    -1.0 / R.B, None, F._ptr(ws), F._stream_ptr(dev))
        F._lib.check(rc, "lsnf_backward_params")
        torch.cuda.synchronize()
        results[name] = views
        for i, v in enumerate(views):
            if i in skipped:
                assert bool((v == SENTINEL).all()), (name, keys[i])
                continue
            e = _l2_rel(v.cpu(), ref[keys[i]].reshape(-1))
            assert e <= TOL, (name, keys[i], e)
            full = results["none"][i]
            if R.B <= 1024:
                assert _same(v, full), (name, keys[i])
            else:
                e = _l2_rel(v, full.double())
                assert e <= TOL_RUN, (name, keys[i], e)




@pytest.mark.parametrize("path", ["recompute", "fast"])
def test_backward_params_skips_null_entries_small(lsnf, kernels, gpu_device, small_ref, path):
    if path == "fast" and not lsnf.flow.params_fast_path():
        path = "recompute"           # LSNF_MATH_FP32 has no fast path: act_saved is then ignored, as the header documents
    _check_skipped_gradients(lsnf.flow, small_ref.on(lsnf.flow, gpu_device), path)


@pytest.mark.parametrize("path", ["recompute", "fast"])
def test_backward_params_skips_null_entries(lsnf, gpu_device, skip_ref, path):
    """B = 100, 5 000 (additive too) and 20 000 rows under the default dispatch and arithmetic: at 20 000 rows the fast path is the
    tiled dump + the bf16-pipe contraction, the recomputing path the LDS-staged fp32 contraction."""
    F = lsnf.flow
    with _settings(F, F.SMALL_BATCH_AUTO, F.MATH_BF16X3):
        _check_skipped_gradients(F, skip_ref.on(F, gpu_device), path)


# ---- form 8: non-finite rows stay in their row -----------------------------------------------------------------------------
def _check_non_finite_rows(F, G):
    """One row carries NaN, +Inf or 1e30 in one element (a row in the middle of a workgroup; the very last row): every other
    row of the forward (block outputs included), the reverse, the backward and the Langevin step is bit-equal to the run on the
    clean batch.  LSNF_MATH_FP16X2 above the threshold recomputes the workgroup of a row that leaves fp16's range in bf16x3
    (documented in the header): there the comparison leaves that workgroup out.  Values only -- every address stays in bounds."""
    R = G.R
    B = R.B

    def run(z):
        f = _forward(F, G, True, z=z)
        x, xo = F.reverse(G.plan, z, G.obj)
        gz = _raw_backward_z(F, G, f.z1, f.saved, f.act, G.gz1, G.gld, None, torch.empty_like(z))
        gf = torch.empty(B, device=G.dev)
        zn = _raw_langevin(F, G, z, f.z1, f.saved, f.act, G.gg, G.noise, None, torch.empty_like(z), gf)
        rows = [f.z1, f.ld, f.ll, x, xo, gz, zn, gf]
        return rows + ([] if f.saved is None else list(f.saved))

    clean = run(G.z)
    _assert_forward(G, clean[0], clean[1], clean[2], "clean")
    _assert_reverse(G, clean[3], clean[4], "clean")
    _assert_grad(clean[5], G.ref.g_a + G.ref.g_b, "clean")
    _assert_langevin(G, clean[6], G.gg, G.noise.double(), "clean")
    for row in (B // 2 + 5, B - 1):
        keep = torch.ones(B, dtype=torch.bool, device=G.dev)
        if _fp16_kernels(F, B):
            keep[_wg_rows(row, B)] = False
        keep[row] = False
        for value in (NAN, float("inf"), 1e30):
            z = G.z.clone()
            z[row, (R.nz // 2 + 3) % R.nz] = value
            dirty = run(z)
            for i, (a, b) in enumerate(zip(dirty, clean)):
                assert _same(a[keep], b[keep]), (row, value, i)


def test_non_finite_rows_small(lsnf, kernels, gpu_device, small_ref):
    _check_non_finite_rows(lsnf.flow, small_ref.on(lsnf.flow, gpu_device))


def test_non_finite_rows_default_dispatch(lsnf, dispatch, gpu_device, default_ref):
    _check_non_finite_rows(lsnf.flow, default_ref.on(lsnf.flow, gpu_device))

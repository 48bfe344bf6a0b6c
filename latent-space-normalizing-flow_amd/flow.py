"""Functional host API over the C ABI: prepared weights ("plan") + forward / reverse /
backward of the flow-prior stack on device-resident fp32 tensors.

PyTorch is plumbing here (device memory, streams); every number is produced by the HIP
kernels in csrc/.  All functions raise on CPU tensors: there is no CPU path."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import LSNF_PARAMS_PER_BLOCK, LsnfError

# order of the live tensors of one coupling block at the ABI (include/lsnf_flow.h)
BLOCK_PARAM_KEYS = (
    "actnorm.b", "actnorm.logs", "invertible_1x1_conv.w",
    "f.fc_1.w", "f.fc_1.actnorm.b", "f.fc_1.actnorm.logs",
    "f.fc_2.w", "f.fc_2.actnorm.b", "f.fc_2.actnorm.logs",
    "f.fc_zeros.w", "f.fc_zeros.b", "f.fc_zeros.logs",
)


def block_prefix(i: int, level: int = 0) -> str:
    return f"revnet2d_s.{level}.revnet2d_step_s.{i}."


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


# ---- argument checks: the C ABI takes bare pointers, so this file is the only place that can know how large a caller's tensor
# is.  Every tensor of every call goes through one of the rules below before anything is launched; each rule is written once.
def _need_cuda(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise LsnfError(f"{name} must live on the GPU (got {t.device}); this library has no CPU path")
    if t.dtype != torch.float32:
        raise LsnfError(f"{name} must be float32 (got {t.dtype})")
    if not t.is_contiguous():
        raise LsnfError(f"{name} must be contiguous")


def _anchor(t: torch.Tensor, name: str, plan: Optional["FlowPlan"], nz: Optional[int] = None) -> int:
    """The (B, nz) tensor that defines B and the call's device, which must be the plan's (nz: for a call without a plan).
    Returns B."""
    _need_cuda(t, name)
    nz = plan.nz if nz is None else nz
    if t.dim() != 2 or t.shape[1] != nz:
        raise LsnfError(f"{name} must be (B, {nz}), got {tuple(t.shape)}")
    if plan is not None and plan.buf.device != t.device:
        raise LsnfError(f"the plan lives on {plan.buf.device}, {name} on {t.device}")
    return t.shape[0]


def _check_in(t: Optional[torch.Tensor], name: str, n: int, device, at_least: bool = False, hint: str = ""):
    """A tensor a kernel reads (None = an optional one left out): on the call's device, float32, contiguous, with the n elements
    the kernel reads (at_least: a stash-like buffer, which may be larger)."""
    if t is None:
        return
    if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
        _need_cuda(t, name)
        raise LsnfError(f"{name} lives on {t.device}, the call's tensors on {device}")
    k = t.numel()
    if k < n or (k > n and not at_least):
        raise LsnfError(f"{name} has {k} elements, the kernel reads {n}" + (f" ({hint})" if hint else ""))


def _check_like(t: Optional[torch.Tensor], name: str, anchor: torch.Tensor, anchor_name: str):
    """A row tensor a kernel reads that must have the anchor's very shape."""
    _check_in(t, name, anchor.numel(), anchor.device)
    if t is not None and t.shape != anchor.shape:
        raise LsnfError(f"{name} must have the shape of {anchor_name}")


def _check_out(t: torch.Tensor, name: str, need: int, device, dtype=torch.float32, hint: str = ""):
    """A buffer a kernel writes: on the call's device, of the dtype the kernel stores, contiguous, large enough."""
    if not t.is_cuda or t.device != device:
        raise LsnfError(f"{name} must live on {device} (got {t.device})")
    if t.dtype != dtype:
        raise LsnfError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise LsnfError(f"{name} must be contiguous")
    if t.numel() < need:
        raise LsnfError(f"{name} has {t.numel()} elements, the kernel writes {need}" + (f" (allocate it {hint})" if hint else ""))


_stash_sizes: dict = {}       # (nz, width, depth, B) -> (floats of act_saved, floats of the parameter-gradient workspace)


def _stash_floats(plan: "FlowPlan", B: int) -> Tuple[int, int]:
    """`lsnf_act_saved_floats` and `lsnf_backward_params_workspace_floats` of B rows: functions of the geometry alone, so they are
    asked once per (geometry, B) instead of crossing ctypes in every call."""
    key = (plan.nz, plan.width, plan.depth, B)
    n = _stash_sizes.get(key)
    if n is None:
        lib = _lib.load()
        if len(_stash_sizes) >= 1024:
            _stash_sizes.clear()
        n = _stash_sizes[key] = (lib.lsnf_act_saved_floats(*key), lib.lsnf_backward_params_workspace_floats(*key))
    return n


_det_sizes: dict = {}         # (nz, width, depth, B) -> floats of the deterministic parameter-gradient workspace


def _det_floats(plan: "FlowPlan", B: int) -> int:
    """`lsnf_backward_params_det_workspace_floats` of B rows, asked once per (geometry, B) -- and only by deterministic calls: the
    default path never enters the query."""
    key = (plan.nz, plan.width, plan.depth, B)
    n = _det_sizes.get(key)
    if n is None:
        if len(_det_sizes) >= 1024:
            _det_sizes.clear()
        n = _det_sizes[key] = _lib.load().lsnf_backward_params_det_workspace_floats(*key)
    return n


def _check_stash_out(plan: "FlowPlan", B: int, device, act_saved, params_ws):
    """The two stash buffers a forward / stash-keeping reverse fills (either may be None)."""
    if act_saved is not None:
        _check_out(act_saved, "act_saved", _stash_floats(plan, B)[0], device, hint="from new_act_saved()")
    if params_ws is not None:
        _check_out(params_ws, "params_ws", _stash_floats(plan, B)[1], device, hint="from new_params_workspace()")


def _check_stash(plan: "FlowPlan", B: int, device, z_saved, act_saved, need_act: bool):
    """What a backward reads of the forward it belongs to: the block outputs (depth > 1) and the activation stash."""
    if act_saved is None and need_act:
        raise LsnfError("act_saved is required: the stash of the forward at these rows, forward(plan, x, ..., act_saved=new_act_saved(plan, B, "
                        "device)) or reverse(..., act_saved=)")
    if z_saved is None and plan.depth > 1 and B > 0:
        raise LsnfError("z_saved (the block outputs of the forward) is required for depth > 1")
    _check_in(z_saved, "z_saved", (plan.depth - 1) * B * plan.nz, device, at_least=True)
    if act_saved is not None:
        _check_in(act_saved, "act_saved", _stash_floats(plan, B)[0], device, at_least=True, hint="the stash of B rows, new_act_saved()")


def _check_params(params: Sequence[torch.Tensor], nz: int, width: int, depth: int, coupling: int, device=None, on: str = "",
                  exact_shape: bool = False):
    """The depth*12 parameter tensors: their count, float32 / contiguous, one device (`device`, the one of `on`; None: the first
    tensor's), and the geometry's size for each (exact_shape: the registered shape, else its element count).  Returns the device."""
    if len(params) != depth * LSNF_PARAMS_PER_BLOCK:
        raise LsnfError(f"expected {depth * LSNF_PARAMS_PER_BLOCK} parameter tensors, got {len(params)}")
    shapes = _param_shapes(nz, width, coupling)
    for i, t in enumerate(params):
        name = f"param[{i}] ({BLOCK_PARAM_KEYS[i % LSNF_PARAMS_PER_BLOCK]})"
        want = shapes[i % LSNF_PARAMS_PER_BLOCK]
        _need_cuda(t, name)
        if device is None:
            device, on = t.device, "param[0]"
        if t.device != device:
            raise LsnfError(f"{name} lives on {t.device}, {on} on {device}")
        if exact_shape and tuple(t.shape) != want:
            raise LsnfError(f"{name} has shape {tuple(t.shape)}, expected {want}")
        if t.numel() != want[0] * want[1]:
            raise LsnfError(f"{name} has {t.numel()} elements, expected {want[0] * want[1]}")
    return device


def _param_table(params: Sequence[torch.Tensor]):
    return (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])


def _plan_head(plan: "FlowPlan"):
    """The five leading arguments every entry point that runs the stack takes."""
    return plan.buf.data_ptr(), plan.nz, plan.width, plan.depth, plan.coupling


def _call(name: str, device, *args, may_refuse: bool = False) -> int:
    """The one way into a launching entry point: `name(*args, stream)` on the current stream of `device`, with that device current;
    a refusal raises LsnfError (may_refuse: it is returned instead -- the caller has another way)."""
    with torch.cuda.device(device):
        rc = getattr(_lib.load(), name)(*args, torch.cuda.current_stream(device).cuda_stream)
    if rc and not may_refuse:
        _lib.check(rc, name)
    return rc


def _stream_buffers(plan: "FlowPlan", attr: str, B: int, device, make):
    """Buffers kept on the plan between calls, one set per (batch size, device, stream): two streams sharing one plan must not
    share them, and a stream keeps one batch size at a time."""
    cache = plan.__dict__.setdefault(attr, {})
    key = (B, device, torch.cuda.current_stream(device).cuda_stream)
    bufs = cache.get(key)
    if bufs is None:
        for k in [k for k in cache if k[2] == key[2]]:
            del cache[k]
        bufs = cache[key] = make()
    return bufs


@dataclass
class FlowPlan:
    """Prepared (folded, padded, fragment-ordered) weights of one `_netF`, device resident."""
    nz: int
    width: int
    depth: int
    coupling: int
    buf: torch.Tensor        # fp32 plan buffer
    scratch: torch.Tensor    # float64 LU workspace (kept so re-preparation allocates nothing)

    @property
    def device(self):
        return self.buf.device

    def logabsdet(self) -> torch.Tensor:
        """(depth,) float64: log|det W_i| computed by the Gauss-Jordan kernel."""
        n = self.nz
        per = n * n + 8
        return self.scratch.view(self.depth, per)[:, n * n].clone()

    def winv(self) -> torch.Tensor:
        """(depth, nz, nz) float64 inverse of every 1x1-conv matrix."""
        n = self.nz
        per = n * n + 8
        return self.scratch.view(self.depth, per)[:, : n * n].reshape(self.depth, n, n).clone()


def alloc_plan(nz: int, width: int, depth: int, coupling: int, device) -> FlowPlan:
    lib = _lib.load()
    nfl = lib.lsnf_plan_floats(nz, width, depth, coupling)
    if nfl == 0:
        raise LsnfError(f"unsupported geometry nz={nz} width={width} depth={depth} coupling={coupling}")
    nsc = lib.lsnf_prepare_scratch_bytes(nz, width, depth)
    buf = torch.empty(nfl, dtype=torch.float32, device=device)
    scratch = torch.empty(nsc // 8, dtype=torch.float64, device=device)
    return FlowPlan(nz, width, depth, coupling, buf, scratch)


def prepare(params: Sequence[torch.Tensor], nz: int, width: int, depth: int, coupling: int = 1,
            plan: Optional[FlowPlan] = None) -> FlowPlan:
    """params: depth*12 device tensors in BLOCK_PARAM_KEYS order per block.
    Replaces the batch-independent work the reference redoes on every call (model.py:182,193,264,349)."""
    lib = _lib.load()
    dev = _check_params(params, nz, width, depth, coupling)
    if plan is None:
        plan = alloc_plan(nz, width, depth, coupling, dev)
    else:       # lsnf_prepare writes what the ARGUMENTS' geometry says into the plan's buffers
        if _plan_head(plan)[1:] != (nz, width, depth, coupling):
            raise LsnfError(f"plan= is one of (nz, width, depth, coupling) = {_plan_head(plan)[1:]}, the call's arguments say "
                            f"{(nz, width, depth, coupling)}")
        _check_out(plan.buf, "plan.buf", lib.lsnf_plan_floats(nz, width, depth, coupling), dev, hint="with alloc_plan()")
        _check_out(plan.scratch, "plan.scratch", lib.lsnf_prepare_scratch_bytes(nz, width, depth) // 8, dev, torch.float64,
                   "with alloc_plan()")
    _call("lsnf_prepare", dev, _param_table(params), nz, width, depth, coupling, _ptr(plan.buf), _ptr(plan.scratch))
    return plan


def _param_shapes(nz: int, width: int, coupling: int) -> List[Tuple[int, ...]]:
    """Shapes of one block's 12 live tensors as the reference registers them (vectors are (1, n))."""
    half = nz // 2
    n_out = nz if coupling == 1 else half
    return [(1, nz), (1, nz), (nz, nz), (half, width), (1, width), (1, width), (width, width), (1, width), (1, width),
            (width, n_out), (1, n_out), (1, n_out)]


def actnorm_init_workspace_bytes(nz: int, width: int, depth: int, coupling: int, B: int) -> int:
    """Bytes of device workspace `actnorm_init` needs (0 on an unsupported geometry or B < 1)."""
    return int(_lib.load().lsnf_actnorm_init_workspace_bytes(int(nz), int(width), int(depth), int(coupling), int(B)))


def actnorm_init(params: Sequence[torch.Tensor], z: torch.Tensor, nz: int, width: int, depth: int, coupling: int = 1,
                 workspace: Optional[torch.Tensor] = None) -> None:
    """Data-dependent actnorm init (reference `_netF.forward(z, objective, init=True)`, model.py:238-241,253-262): fits
    every block's actnorm and its two fc actnorms to the batch z, in place -- tensors 0, 1, 4, 5, 7, 8 of each block
    (BLOCK_PARAM_KEYS order) are overwritten, the other six are read.  Asynchronous on the current stream.  Plans
    prepared from these tensors are stale afterwards (`prepare` again).
    workspace: None (allocated here) or a device buffer of at least `actnorm_init_workspace_bytes()` bytes.
    Every argument is checked before anything is launched; a bad one raises LsnfError."""
    lib = _lib.load()
    nz, width, depth, coupling = int(nz), int(width), int(depth), int(coupling)
    need = lib.lsnf_actnorm_init_workspace_bytes(nz, width, depth, coupling, 1)
    if need == 0:
        raise LsnfError(f"unsupported geometry nz={nz} width={width} depth={depth} coupling={coupling}")
    B = _anchor(z, "z", None, nz)
    if B < 1:
        raise LsnfError("actnorm_init needs a non-empty batch")
    _check_params(params, nz, width, depth, coupling, z.device, "z", exact_shape=True)
    need = lib.lsnf_actnorm_init_workspace_bytes(nz, width, depth, coupling, B)
    if workspace is None:
        workspace = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=z.device)
    else:
        if not workspace.is_cuda or workspace.device != z.device:
            raise LsnfError(f"workspace must live on {z.device} (got {workspace.device})")
        if not workspace.is_contiguous():
            raise LsnfError("workspace must be contiguous")
        if workspace.numel() * workspace.element_size() < need:
            raise LsnfError(f"workspace has {workspace.numel() * workspace.element_size()} bytes, "
                            f"lsnf_actnorm_init needs {need} (actnorm_init_workspace_bytes())")
        if workspace.data_ptr() % 16:
            raise LsnfError("workspace must be 16-byte aligned")
    _call("lsnf_actnorm_init", z.device, _param_table(params), nz, width, depth, coupling, B, _ptr(z), _ptr(workspace))


def params_from_state_dict(sd, depth: int, device=None) -> List[torch.Tensor]:
    """Pick the 12 live tensors per block out of a reference-keyed state_dict."""
    out = []
    for i in range(depth):
        pre = block_prefix(i)
        for k in BLOCK_PARAM_KEYS:
            t = sd[pre + k]
            if device is not None:
                t = t.to(device)
            out.append(t.detach().to(torch.float32).contiguous())
    return out


def forward(plan: FlowPlan, z: torch.Tensor, objective: Optional[torch.Tensor] = None, *,
            first_block: int = 0, n_blocks: Optional[int] = None, want_ll: bool = True,
            save_for_backward: bool = False, out: Optional[Tuple[torch.Tensor, ...]] = None,
            stats: Optional[torch.Tensor] = None, act_saved: Optional[torch.Tensor] = None,
            z_saved_out: Optional[torch.Tensor] = None, params_ws: Optional[torch.Tensor] = None):
    """One launch: blocks [first_block, first_block+n_blocks) on (B, nz) rows.
    Returns (z_out, logdet, ll or None, z_saved or None).  model.py:473-483 + train.py:317-319.
    act_saved: optional buffer from `new_act_saved()`, filled with the sigmoid / relu-mask stash that lets
    `backward_z` / the Langevin step skip recomputing the coupling MLP.
    stats: optional buffer from `new_stats()`; afterwards stats[4] = sum ll, stats[5] = sum logdet, stats[6] = B
    (summed inside the kernel -- no separate reduction launch).
    params_ws: optional workspace from `new_params_workspace()` (with act_saved and the block outputs): the forward also
    writes the hidden activations there, so that `backward_params(..., act_saved=, workspace=)` runs from the stash."""
    B, dev = _anchor(z, "z", plan), z.device
    n_blocks = plan.depth - first_block if n_blocks is None else n_blocks
    _check_in(objective, "objective", B, dev)
    if out is not None:
        z_out, logdet, ll = out
    else:
        z_out = torch.empty_like(z)
        logdet = torch.empty(B, dtype=torch.float32, device=dev)
        ll = torch.empty(B, dtype=torch.float32, device=dev) if want_ll else None
    saved = z_saved_out                     # caller-owned (n_blocks-1, B, nz) buffer for the block outputs, or
    if saved is None and save_for_backward and n_blocks > 1:
        saved = torch.empty((n_blocks - 1, B, plan.nz), dtype=torch.float32, device=dev)
    _check_out(z_out, "out[0] (z_out)", B * plan.nz, dev)
    _check_out(logdet, "out[1] (logdet)", B, dev)
    if ll is not None:
        _check_out(ll, "out[2] (ll)", B, dev)
    if saved is not None:
        _check_out(saved, "z_saved", max(n_blocks - 1, 0) * B * plan.nz, dev)
    if stats is not None:               # ABI v5: 264 doubles (8 + 64 sub-accumulators of 4); the kernel writes all of them
        _check_out(stats, "stats", STATS_DOUBLES, dev, torch.float64, "from new_stats()")
    _check_stash_out(plan, B, dev, act_saved, params_ws)
    args = _forward_args(plan, first_block, n_blocks, z, objective, z_out, logdet, ll, saved, act_saved, params_ws)
    _call("lsnf_forward", dev, *args, _ptr(stats))
    return z_out, logdet, ll, saved


def _forward_args(plan: FlowPlan, first_block: int, n_blocks: int, z, objective, z_out, logdet, ll, saved, act_saved, params_ws):
    """The arguments of `lsnf_forward` in ABI order, up to `stats` and the stream (which vary from call to call)."""
    return _plan_head(plan) + (first_block, n_blocks, z.shape[0], _ptr(z), _ptr(objective), _ptr(z_out), _ptr(logdet), _ptr(ll),
                               _ptr(saved), _ptr(act_saved), _ptr(params_ws))


class BoundForward:
    """`forward(plan, z, out=..., stats=...)` with everything but the `stats` row bound and checked ONCE: a call is then one ctypes
    call on the current stream (~4 us of host time instead of ~12: tensor checks, size queries and pointer extraction are what a
    20 us strong-scaling shard launch cannot afford per step, tools/host_cost_allreduce.py).  Same launch, same results.

        fw = BoundForward(plan, z, out)          # buffers as for forward(); the plan is re-read at every call (data_ptr is stable)
        fw(stats_row)                            # == forward(plan, z, out=out, stats=stats_row)
    The caller keeps z / out / the plan alive and on the device that is current at call time."""

    def __init__(self, plan: FlowPlan, z: torch.Tensor, out, objective: Optional[torch.Tensor] = None, act_saved: Optional[torch.Tensor] = None,
                 z_saved_out: Optional[torch.Tensor] = None):
        probe = new_stats(z.device)
        forward(plan, z, objective, out=out, stats=probe, act_saved=act_saved, z_saved_out=z_saved_out)       # every check of forward(), once
        self._keep = (plan, z, out, objective, act_saved, z_saved_out)
        self._lib = _lib.load()
        self._dev = z.device
        self._head = _forward_args(plan, 0, plan.depth, z, objective, out[0], out[1], out[2], z_saved_out, act_saved, None)

    def __call__(self, stats: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None) -> None:
        """stream: the stream to launch on (default: the current one) -- passing it saves the `with torch.cuda.stream(...)` around the call."""
        if stats is not None and (stats.dtype != torch.float64 or stats.numel() < STATS_DOUBLES or stats.device != self._dev):
            raise LsnfError("stats must be a float64 buffer of LSNF_STATS_DOUBLES doubles on the call's device (new_stats())")
        sp = (torch.cuda.current_stream(self._dev) if stream is None else stream).cuda_stream
        rc = self._lib.lsnf_forward(*self._head, None if stats is None else stats.data_ptr(), sp)
        if rc:
            _lib.check(rc, "lsnf_forward")


SMALL_BATCH_AUTO = -2


def set_small_batch_max(rows: int) -> int:
    """Batches <= rows use the small-batch (latency) kernels (one threshold for every entry point).  rows >= 0 sets it,
    SMALL_BATCH_AUTO goes back to the built-in crossover of the arithmetic mode; both return the previous SETTING (a row
    count or SMALL_BATCH_AUTO), so `prev = set(x); ...; set(prev)` restores exactly.  rows == -1 only queries the threshold
    in force."""
    return _lib.load().lsnf_set_small_batch_max(int(rows))


MATH_FP32, MATH_BF16X3, MATH_FP16X2, MATH_BF16X3_PHASED = 0, 1, 3, 5


def set_math_mode(mode: int) -> int:
    """Arithmetic of the GEMMs (include/lsnf_flow.h): MATH_BF16X3 (default: error-free three-way bf16 split, 24 operand
    bits, six bf16 MFMAs per product; 16x16x32 MFMA, the throughput forward software-pipelined where it applies),
    MATH_BF16X3_PHASED (the same without the pipelined forward), MATH_FP32 (fp32 MFMA) or MATH_FP16X2
    (opt-in, NARROWER than fp32: two-term fp16 split, three fp16 MFMAs per product, range-guarded by a bf16x3 fix-up pass).
    Returns the previous mode (mode < 0: query)."""
    return _lib.load().lsnf_set_math_mode(int(mode))


def new_act_saved(plan: "FlowPlan", B: int, device) -> torch.Tensor:
    """Uninitialised activation stash for `forward(..., act_saved=)` on a batch of B rows."""
    return torch.empty(max(_stash_floats(plan, int(B))[0], 1), dtype=torch.float32, device=device)


def params_fast_path() -> bool:
    """True if the math mode in force lets `backward_params` run from the forward's stash (every bf16x3-family mode)."""
    return bool(_lib.load().lsnf_params_fast_path())


def new_params_workspace(plan: "FlowPlan", B: int, device, deterministic: bool = False) -> torch.Tensor:
    """Uninitialised workspace of `backward_params` for a batch of B rows (also the `params_ws` of `forward`).
    deterministic: the larger workspace of `backward_params(..., deterministic=True)` -- the same layout followed by the
    per-chunk partials (`lsnf_backward_params_det_workspace_floats`); it serves the forward and the default call as well."""
    n = _det_floats(plan, int(B)) if deterministic else _stash_floats(plan, int(B))[1]
    return torch.empty(max(n, 4), dtype=torch.float32, device=device)


STATS_DOUBLES = 264          # include/lsnf_flow.h LSNF_STATS_DOUBLES


def new_stats(device) -> torch.Tensor:
    """Zero-initialised accumulator (LSNF_STATS_DOUBLES = 264 doubles) for `forward(..., stats=)` (one per stream)."""
    return torch.zeros(STATS_DOUBLES, dtype=torch.float64, device=device)


def reverse_keep_supported(plan: FlowPlan, B: int) -> bool:
    """True if `reverse` / `sample` can keep the backward's stash for a batch of B rows (`lsnf_reverse_keep_covers`): the
    latency bf16x3 reverse, i.e. a bf16x3-family math mode and B up to the small-batch threshold in force."""
    return bool(_lib.load().lsnf_reverse_keep_covers(*_plan_head(plan)[1:], int(B)))


def _keep_buffers(plan: FlowPlan, B: int, device, save_for_backward: bool, act_saved, params_ws):
    """The block-output buffer of a stash-keeping reverse / sample (or None), after the size checks of all three buffers."""
    saved = None
    if save_for_backward and plan.depth > 1:
        saved = torch.empty((plan.depth - 1, B, plan.nz), dtype=torch.float32, device=device)
    _check_stash_out(plan, B, device, act_saved, params_ws)
    return saved


def reverse(plan: FlowPlan, z: torch.Tensor, objective: Optional[torch.Tensor] = None, *,
            out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, save_for_backward: bool = False,
            act_saved: Optional[torch.Tensor] = None, params_ws: Optional[torch.Tensor] = None,
            z_saved_out: Optional[torch.Tensor] = None):
    """model.py:484-498: returns (z_out, objective_out) with objective_out = objective - sum log|det J|.
    out: optional caller-owned (z_out, objective_out); either may be the input itself (in-place call).
    save_for_backward / act_saved / params_ws (as `forward`'s): the same launch, same bits, also keeps what the FORWARD at
    x = z_out would -- the block outputs, the activation stash, h1 / h2 for the parameter gradients -- so that
    `reverse_backward_z(plan, z, saved, act_saved, ...)` and `backward_params(plan, params, x, z, saved, ..., act_saved=,
    workspace=)` need no second pass over x.  The return is then (z_out, objective_out, saved).  Only where
    `reverse_keep_supported(plan, B)`; elsewhere the call raises.  z_saved_out: optional caller-owned (depth-1, B, nz) buffer for
    `saved` (implies save_for_backward)."""
    B, dev = _anchor(z, "z", plan), z.device
    _check_in(objective, "objective", B, dev)
    if out is not None:
        z_out, obj_out = out
        _check_out(z_out, "out[0] (z_out)", B * plan.nz, dev)
        _check_out(obj_out, "out[1] (objective_out)", B, dev)
    else:
        z_out = torch.empty_like(z)
        obj_out = torch.empty(B, dtype=torch.float32, device=dev)
    args = _plan_head(plan) + (B, _ptr(z), _ptr(objective), _ptr(z_out), _ptr(obj_out))
    if save_for_backward or act_saved is not None or params_ws is not None or z_saved_out is not None:
        if z_saved_out is not None:
            _check_out(z_saved_out, "z_saved_out", (plan.depth - 1) * B * plan.nz, dev)
        saved = _keep_buffers(plan, B, dev, save_for_backward and z_saved_out is None, act_saved, params_ws)
        if z_saved_out is not None and plan.depth > 1:
            saved = z_saved_out
        _call("lsnf_reverse_keep", dev, *args, _ptr(saved), _ptr(act_saved), _ptr(params_ws))
        return z_out, obj_out, saved
    _call("lsnf_reverse", dev, *args)
    return z_out, obj_out


def backward_z(plan: FlowPlan, z_out: torch.Tensor, z_saved: Optional[torch.Tensor],
               g_z1: Optional[torch.Tensor] = None, g_logdet: Optional[torch.Tensor] = None,
               ll_scale: Optional[float] = None, act_saved: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dL/dz_in of the full stack (train.py:323).  Either pass upstream gradients (g_z1, g_logdet) or
    ll_scale for L = ll_scale * sum_b ll_b (train.py:320: ll_scale = -1).  act_saved: the stash the forward
    filled (same batch), or None: the stash is then rebuilt from the block outputs (`lsnf_restash`, bf16 matrix pipe;
    in MATH_FP32 the fp32 backward recomputes the coupling MLP itself)."""
    B, dev = _anchor(z_out, "z_out", plan), z_out.device
    _check_stash(plan, B, dev, z_saved, act_saved, False)
    _check_in(g_z1, "g_z1", B * plan.nz, dev)
    _check_in(g_logdet, "g_logdet", B, dev)
    if act_saved is None and B > 0 and params_fast_path():
        # the rebuilt stash lives on the plan -- ~1.4 KB per row, not re-allocated per call (and not inside a graph capture); if the
        # rebuild is refused, lsnf_backward_z recomputes the MLP itself (act_saved NULL)
        buf = _stream_buffers(plan, "_restash_buffers", B, dev, lambda: new_act_saved(plan, B, dev))
        if _call("lsnf_restash", dev, *_plan_head(plan), B, _ptr(z_out), _ptr(z_saved), _ptr(buf), may_refuse=True) == 0:
            act_saved = buf
    g_in = torch.empty_like(z_out)
    _call("lsnf_backward_z", dev, *_plan_head(plan), B, _ptr(z_out), _ptr(z_saved), _ptr(act_saved), _ptr(g_z1), _ptr(g_logdet),
          0 if ll_scale is None else 1, float(ll_scale or 0.0), _ptr(g_in))
    return g_in


def reverse_backward_z(plan: FlowPlan, z_out: torch.Tensor, z_saved: Optional[torch.Tensor], act_saved: torch.Tensor,
                       g_x: Optional[torch.Tensor] = None, g_obj: Optional[torch.Tensor] = None, *,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Backward of `reverse` w.r.t. its input: with x = reverse(eps)[0], returns dL/d eps for upstream gradients g_x = dL/dx
    (or None = 0) and g_obj = dL/d objective_out (or None = 0); dL/d objective is g_obj itself.
    z_out / z_saved / act_saved: what `forward(plan, x, save_for_backward=True, act_saved=new_act_saved(...))` returned and
    filled (the forward evaluated AT x; the stash is required, from any math mode / kernel family).  out: optional (B, nz)
    buffer for the result, may be g_x itself.  One launch, asynchronous on the current stream.
    The parameter gradients of the reverse are `backward_params` of that forward with g_z1 = -result, g_logdet = -g_obj."""
    B, dev = _anchor(z_out, "z_out", plan), z_out.device
    _check_stash(plan, B, dev, z_saved, act_saved, True)
    _check_like(g_x, "g_x", z_out, "z_out")
    _check_in(g_obj, "g_obj", B, dev)
    g_in = torch.empty_like(z_out) if out is None else out
    _check_out(g_in, "out (g_z_in)", B * plan.nz, dev)
    _call("lsnf_reverse_backward_z", dev, *_plan_head(plan), B, _ptr(z_out), _ptr(z_saved), _ptr(act_saved), _ptr(g_x), _ptr(g_obj),
          _ptr(g_in))
    return g_in


class PhiloxNoise:
    """In-kernel N(0,1) noise for `langevin_step` (include/lsnf_flow.h `LsnfRng`): a pure function of
    (seed, offset, row0 + row, column).  `offset` must differ from step to step (`.step()` returns the next one);
    `row0` is the global index of the shard's first row, so that row-sharded chains draw what one GPU would;
    `offset_dev` is an optional int64/uint64 device scalar added to `offset` (advance it inside a captured graph)."""
    __slots__ = ("seed", "offset", "row0", "offset_dev")

    def __init__(self, seed: int, offset: int = 0, row0: int = 0, offset_dev: Optional[torch.Tensor] = None):
        self.seed, self.offset, self.row0, self.offset_dev = int(seed), int(offset), int(row0), offset_dev

    def step(self, n: int = 1) -> "PhiloxNoise":
        """A NEW generator n steps further on (this one is unchanged)."""
        return PhiloxNoise(self.seed, self.offset + n, self.row0, self.offset_dev)

    def advance(self, n: int = 1) -> "PhiloxNoise":
        """Moves THIS generator n steps on, in place (the K-step sampler calls it with K when it returns, so that a
        generator kept across training iterations never repeats a draw)."""
        self.offset += int(n)
        return self

    def _c(self):
        mask = (1 << 64) - 1
        dev = None if self.offset_dev is None else self.offset_dev.data_ptr()
        return _lib.LsnfRng(self.seed & mask, self.offset & mask, dev, self.row0)


def _noise_args(noise, anchor: Optional[torch.Tensor], anchor_name: str, device):
    """The noise argument of a call -- None, a tensor shaped like the anchor, or a `PhiloxNoise` -- as the ABI's pair
    (noise tensor or None, LsnfRng by reference or None)."""
    if not isinstance(noise, PhiloxNoise):
        _check_like(noise, "noise", anchor, anchor_name)
        return noise, None
    od = noise.offset_dev
    if od is not None and (od.device != device or od.dtype not in (torch.int64, torch.uint64) or od.numel() != 1):
        raise LsnfError(f"offset_dev must be one 64-bit integer on {device}")
    return None, ctypes.byref(noise._c())


def sample(plan: FlowPlan, B: int, rng: PhiloxNoise, *, temperature: float = 1.0, want_eps: bool = False,
           want_ll: bool = False, out: Optional[Tuple[Optional[torch.Tensor], ...]] = None, save_for_backward: bool = False,
           act_saved: Optional[torch.Tensor] = None, params_ws: Optional[torch.Tensor] = None):
    """Fused prior sampling (`lsnf_sample`; train.py:472-475 without the `randn` launch and its (B, nz) tensor): ONE launch draws
    eps = temperature * N(0,1) inside the reverse kernel -- a pure function of (rng.seed, rng.offset, rng.row0 + row, column),
    so row-sharded calls with matching `row0` draw what one call would -- and returns (x, objective_out, eps or None, ll or None):
    x, objective_out = what `reverse(plan, eps)` returns, bit for bit; ll = -0.5*sum eps^2 + log(2 pi) - objective_out, the
    log-density of x under the flow prior.  `rng` is not advanced: pass `rng.step()` (or advance it) for the next call.
    out: optional caller-owned (x, objective_out, eps, ll) on the plan's device; each of the last three may be None (not
    written; want_eps / want_ll then do not apply).  Every buffer is checked before anything is launched.
    save_for_backward / act_saved / params_ws: as `reverse`'s (`lsnf_sample_keep`); the return is then (x, objective_out, eps, ll,
    saved), and eps -- the last block's output, which the backward reads -- is always returned (with `out`, out[2] is required)."""
    B = int(B)
    dev = plan.device
    keep = save_for_backward or act_saved is not None or params_ws is not None
    want_eps = want_eps or keep
    if not isinstance(rng, PhiloxNoise):
        raise LsnfError("rng must be a flow.PhiloxNoise (the draw is made inside the kernel; there is no tensor form)")
    if B < 0:
        raise LsnfError(f"B must be >= 0 (got {B})")
    _need_cuda(plan.buf, "plan.buf")         # there is no anchor tensor: the call's device is the plan's
    c = _noise_args(rng, None, "", dev)[1]
    if out is not None:
        if len(out) != 4:
            raise LsnfError("out must be (x, objective_out, eps, ll); the last three may be None")
        x, obj, eps, ll = out
        if x is None:
            raise LsnfError("out[0] (x) is required")
    else:
        f32 = dict(dtype=torch.float32, device=dev)
        x, obj = torch.empty((B, plan.nz), **f32), torch.empty(B, **f32)
        eps = torch.empty((B, plan.nz), **f32) if want_eps else None
        ll = torch.empty(B, **f32) if want_ll else None
    _check_out(x, "out[0] (x)", B * plan.nz, dev)
    if obj is not None:
        _check_out(obj, "out[1] (objective_out)", B, dev)
    if eps is not None:
        _check_out(eps, "out[2] (eps)", B * plan.nz, dev)
        if B and eps.data_ptr() == x.data_ptr():
            raise LsnfError("out[2] (eps) must not alias out[0] (x)")
    if ll is not None:
        _check_out(ll, "out[3] (ll)", B, dev)
    args = _plan_head(plan) + (B, c, float(temperature), _ptr(x), _ptr(obj), _ptr(eps), _ptr(ll))
    if keep:
        if eps is None:
            raise LsnfError("out[2] (eps) is required with save_for_backward / act_saved / params_ws")
        saved = _keep_buffers(plan, B, dev, save_for_backward, act_saved, params_ws)
        _call("lsnf_sample_keep", dev, *args, _ptr(saved), _ptr(act_saved), _ptr(params_ws))
        return x, obj, eps, ll, saved
    _call("lsnf_sample", dev, *args)
    return x, obj, eps, ll


def langevin_step(plan: FlowPlan, z: torch.Tensor, grad_g: Optional[torch.Tensor], noise,
                  step_size: float, *, inplace: bool = False, want_norms: bool = True, reuse_buffers: bool = False):
    """One flow-prior Langevin update (train.py:316-329) in two launches: forward (keeps block outputs) and the
    fused backward+update.  `noise`: None, a (B, nz) tensor of N(0,1) draws, or a `PhiloxNoise` (drawn inside the
    kernel).  Returns (z_new, ll, gf_norm, gg_norm); ll is the log-prob of the INPUT z
    (f_log_lkhd = -ll.sum(), train.py:320).  reuse_buffers: keep the intermediate buffers (block outputs, activation stash,
    z1, logdet, ll, norms: ~4 KB per row) on the plan between calls of the same batch size instead of asking the
    allocator for them every step -- the returned ll / norms are then overwritten by the next call (the K-step sampler
    consumes them at once)."""
    B, dev = _anchor(z, "z", plan), z.device
    _check_like(grad_g, "grad_g", z, "z")
    noise, rng = _noise_args(noise, z, "z", dev)

    def make():
        f32 = dict(dtype=torch.float32, device=dev)
        return {"act": new_act_saved(plan, B, dev), "out": (torch.empty_like(z), torch.empty(B, **f32), torch.empty(B, **f32)),
                "saved": torch.empty((plan.depth - 1, B, plan.nz), **f32) if plan.depth > 1 else None,
                "gf": torch.empty(B, **f32), "gg": torch.empty(B, **f32)}
    bufs = _stream_buffers(plan, "_langevin_buffers", B, dev, make) if reuse_buffers else make()
    act, saved = bufs["act"], bufs["saved"]
    _check_stash(plan, B, dev, saved, act, True)
    z1, logdet, ll, _ = forward(plan, z, None, want_ll=True, out=bufs["out"], act_saved=act, z_saved_out=saved)
    z_new = z if inplace else torch.empty_like(z)
    gf = bufs["gf"] if want_norms else None
    gg = bufs["gg"] if (want_norms and grad_g is not None) else None
    _call("lsnf_langevin_step", dev, *_plan_head(plan), B, _ptr(z), _ptr(z1), _ptr(saved), _ptr(act), _ptr(grad_g), _ptr(noise), rng,
          float(step_size), _ptr(z_new), _ptr(gf), _ptr(gg))
    return z_new, ll, gf, gg


def reverse_langevin_step(plan: FlowPlan, eps: torch.Tensor, z_saved: Optional[torch.Tensor], act_saved: torch.Tensor,
                          grad_g: Optional[torch.Tensor], noise, step_size: float, *, inplace: bool = False,
                          out: Optional[Tuple[Optional[torch.Tensor], ...]] = None, want_g: bool = False, want_norms: bool = True):
    """One base-space Langevin update in ONE launch (`lsnf_reverse_langevin_step`): with x = reverse(eps)[0] and
    g_eps = J_{f^-1}(eps)^T grad_g (`reverse_backward_z(plan, eps, z_saved, act_saved, grad_g)`'s bits),
        eps_new = eps - 0.5 s^2 (eps + g_eps) + s * noise         (fp32: t = eps + g; u = fma(-0.5 s^2, t, eps); fma(s, noise, u)).
    eps / z_saved / act_saved: the last block's output (= eps), the block outputs and the stash of the forward AT x -- from
    `forward(plan, x, ...)`, or kept by `reverse(plan, eps, save_for_backward=True, act_saved=...)`.  grad_g: dL/dx or None (= 0).
    `noise`: None, a (B, nz) tensor of N(0,1) draws, or a `PhiloxNoise` (drawn inside the kernel: the same draw as `sample`'s eps at
    temperature 1, and the same result bits as passing that tensor).
    Returns (eps_new, g_eps or None, g_norm or None, eps_norm or None): g_norm / eps_norm (B) = the per-row 2-norms of g_eps and of
    the INPUT eps (want_norms), g_eps with want_g.  inplace: eps_new is eps itself.  out: optional caller-owned
    (eps_new, g_eps, g_norm, eps_norm), each may be None (then allocated if wanted); out[1] may be grad_g.  Asynchronous on the
    current stream; nothing but the launch, so it can be captured in a graph."""
    B, dev = _anchor(eps, "eps", plan), eps.device
    _check_stash(plan, B, dev, z_saved, act_saved, True)
    _check_like(grad_g, "grad_g", eps, "eps")
    noise, rng = _noise_args(noise, eps, "eps", dev)
    eps_new = g_eps = g_norm = eps_norm = None
    if out is not None:
        if len(out) != 4:
            raise LsnfError("out must be (eps_new, g_eps, g_norm, eps_norm); each may be None")
        eps_new, g_eps, g_norm, eps_norm = out
    if inplace:
        if eps_new is not None and eps_new.data_ptr() != eps.data_ptr():
            raise LsnfError("inplace=True writes eps itself: out[0] must be None (or eps)")
        eps_new = eps
    f32 = dict(dtype=torch.float32, device=dev)
    if eps_new is None:
        eps_new = torch.empty_like(eps)
    if g_eps is None and want_g:
        g_eps = torch.empty_like(eps)
    if g_norm is None and want_norms:
        g_norm = torch.empty(B, **f32)
    if eps_norm is None and want_norms:
        eps_norm = torch.empty(B, **f32)
    _check_out(eps_new, "out[0] (eps_new)", B * plan.nz, dev)
    if g_eps is not None:
        _check_out(g_eps, "out[1] (g_eps)", B * plan.nz, dev)
    for name, t in (("out[2] (g_norm)", g_norm), ("out[3] (eps_norm)", eps_norm)):
        if t is not None:
            _check_out(t, name, B, dev)
    _call("lsnf_reverse_langevin_step", dev, *_plan_head(plan), B, _ptr(eps), _ptr(z_saved), _ptr(act_saved), _ptr(grad_g), _ptr(noise),
          rng, float(step_size), _ptr(eps_new), _ptr(g_eps), _ptr(g_norm), _ptr(eps_norm))
    return eps_new, g_eps, g_norm, eps_norm


def backward_params(plan: FlowPlan, params: Sequence[torch.Tensor], z_in: torch.Tensor, z_out: torch.Tensor,
                    z_saved: Optional[torch.Tensor], g_z1: Optional[torch.Tensor] = None,
                    g_logdet: Optional[torch.Tensor] = None, ll_scale: Optional[float] = None,
                    want_grad_z: bool = False, want_flat: bool = False, reuse_buffers: bool = False,
                    act_saved: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, *,
                    deterministic: bool = False):
    """dL/dtheta for the depth*12 live tensors (train.py:406-411).  Returns a list of gradients shaped like
    `params` (and dL/dz_in as a second value if want_grad_z; and, last, the ONE flat buffer the gradients are views
    of if want_flat -- a global norm / clip is then one reduction instead of 60).  reuse_buffers: keep the flat
    gradient buffer, its 60 views, the pointer tables and the workspace on the plan between calls (as long as the
    parameter storages and B do not change) -- the returned gradient tensors are then THE SAME objects every call,
    overwritten in place (an optimizer that consumes .grad before the next call does not notice; ~0.2 ms of host time).
    act_saved + workspace: the stash and the `params_ws` the forward of THIS evaluation was given -- the backward then runs
    from the stash on the bf16 matrix pipe instead of recomputing the coupling MLP in fp32 (`params_fast_path()`).
    deterministic: `lsnf_backward_params_det` -- every sum over the batch in a fixed order, so the same inputs (and build, math
    mode, small-batch threshold) give the same bits on every run, stream, graph replay and device; a `workspace` must then come from
    `new_params_workspace(..., deterministic=True)`.  Not torch's global determinism flag: this keyword alone decides."""
    B, dev, head = _anchor(z_out, "z_out", plan), z_out.device, _plan_head(plan)
    _check_in(z_in, "z_in", B * plan.nz, dev)
    if (act_saved is None) != (workspace is None):
        raise LsnfError("act_saved and workspace go together: both from the forward of this evaluation")
    _check_stash(plan, B, dev, z_saved, act_saved, False)
    _check_in(g_z1, "g_z1", B * plan.nz, dev)
    _check_in(g_logdet, "g_logdet", B, dev)
    deterministic = bool(deterministic)
    ws_floats = _det_floats(plan, B) if deterministic else _stash_floats(plan, B)[1]
    _check_in(workspace, "workspace", ws_floats, dev, at_least=True,
              hint="new_params_workspace(deterministic=True)" if deterministic else "new_params_workspace()")
    # (workspace is None: the kept state owns a workspace only then -- a call without one must not find the empty one that a call
    #  with a caller-owned workspace left)
    key = (tuple(p.data_ptr() for p in params), B, dev, want_grad_z, torch.cuda.current_stream(dev).cuda_stream, deterministic,
           workspace is None)
    st = plan.__dict__.get("_bp_state") if reuse_buffers else None     # (keyed by stream too: a second stream re-allocates)
    if st is None or st["key"] != key:
        # the gradient views below are shaped like the tensors handed over and the kernels write what the geometry says: check them
        _check_params(params, *head[1:], dev, "z_out")
        # one flat gradient buffer, handed out as views (60 separate allocations cost ~200 us of host time)
        raw = [p.detach() for p in params]
        sizes = [t.numel() for t in raw]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        grads = [g.view(t.shape) for g, t in zip(flat.split(sizes), raw)]
        nws = ws_floats if workspace is None else 0
        base, o, offs = flat.data_ptr(), 0, []
        for n in sizes:
            offs.append(base + o * 4)
            o += n
        st = {"key": key, "flat": flat, "grads": grads,
              "g_in": torch.empty_like(z_out) if want_grad_z else None,
              "ws": torch.empty(nws, dtype=torch.float32, device=dev),
              "parr": _param_table(raw), "garr": (ctypes.c_void_p * len(raw))(*offs)}
        if reuse_buffers:
            plan.__dict__["_bp_state"] = st
    flat, grads, g_in, ws, parr, garr = st["flat"], st["grads"], st["g_in"], st["ws"], st["parr"], st["garr"]
    if workspace is not None:
        ws = workspace
    _call("lsnf_backward_params_det" if deterministic else "lsnf_backward_params", dev, head[0], parr, garr, *head[1:], B,
          _ptr(z_in), _ptr(z_out), _ptr(z_saved), _ptr(act_saved), _ptr(g_z1), _ptr(g_logdet),
          0 if ll_scale is None else 1, float(ll_scale or 0.0), _ptr(g_in), _ptr(ws))
    out = (grads,) + ((g_in,) if want_grad_z else ()) + ((flat,) if want_flat else ())
    return out if len(out) > 1 else grads


# ---- optimizer step of the flow (include/lsnf_flow.h lsnf_adam_step) ---------------------------------------------------
ADAM_MAX_GROUPS, ADAM_STEP_OFFSET, ADAM_PARTIALS_OFFSET, ADAM_NORM_OFFSET, ADAM_HEADER_BYTES = 256, 0, 2048, 4096, 4160
ADAM_AMSGRAD, ADAM_DECOUPLED, ADAM_MAXIMIZE, ADAM_EMA, ADAM_SKIP_NONFINITE, ADAM_SKIPPED_OFFSET = 1, 2, 4, 8, 16, 4104
_adam_tables: dict = {}       # state address -> (key, params table, grads table): the ctypes arrays of the last call on that state


def _adam_size_flags(amsgrad: bool, ema: bool) -> int:
    return (ADAM_AMSGRAD if amsgrad else 0) | (ADAM_EMA if ema else 0)


def adam_state_bytes(nz: int, width: int, depth: int, coupling: int = 1, amsgrad: bool = False, ema: bool = False) -> int:
    """Bytes of the optimizer state of `adam_step` (0 on an unsupported geometry); amsgrad / ema: with the array each adds."""
    geo, flags = (int(nz), int(width), int(depth), int(coupling)), _adam_size_flags(amsgrad, ema)
    lib = _lib.load()
    return int(lib.lsnf_adam_state_bytes_ex(*geo, flags) if flags else lib.lsnf_adam_state_bytes(*geo))


def new_adam_state(nz: int, width: int, depth: int, coupling: int, device, amsgrad: bool = False, ema: bool = False) -> torch.Tensor:
    """A fresh (all-zero) optimizer state for `adam_step`: one float32 buffer holding the header (step counters, norm
    partials, the last norm, the skipped count) followed by m and v, flat in ABI tensor order (`adam_state_views`), then vmax
    (amsgrad) and the weight average (ema) in the same order (`adam_state_extra_views`).  A state serves the amsgrad / ema it
    was made for: pass the same two to every `adam_step` on it."""
    need = adam_state_bytes(nz, width, depth, coupling, amsgrad, ema)
    if need == 0:
        raise LsnfError(f"unsupported geometry nz={nz} width={width} depth={depth} coupling={coupling}")
    return torch.zeros(need // 4, dtype=torch.float32, device=device)


def adam_state_views(state: torch.Tensor, nz: int, width: int, depth: int, coupling: int = 1):
    """(steps, norm, m, v) as views of `state`: steps = the int64 step counters (one per workgroup of the update launch, those in
    use all equal; steps[0] is the step count, and setting the step means filling all of them), norm = the last pre-clip norm (0-dim), m / v = lists of depth*12 tensors
    shaped like the parameters."""
    shapes = _param_shapes(nz, width, coupling) * depth
    sizes = [a * b for a, b in shapes]
    n4 = (sum(sizes) + 3) // 4 * 4
    h = ADAM_HEADER_BYTES // 4
    steps = state[ADAM_STEP_OFFSET // 4: ADAM_STEP_OFFSET // 4 + 2 * ADAM_MAX_GROUPS].view(torch.int64)
    norm = state[ADAM_NORM_OFFSET // 4]
    m = [t.view(sh) for t, sh in zip(state[h: h + sum(sizes)].split(sizes), shapes)]
    v = [t.view(sh) for t, sh in zip(state[h + n4: h + n4 + sum(sizes)].split(sizes), shapes)]
    return steps, norm, m, v


def adam_state_extra_views(state, nz: int, width: int, depth: int, coupling: int = 1, amsgrad: bool = False, ema: bool = False):
    """(vmax | None, ema | None, skipped) as views of a state made with these amsgrad / ema: vmax (amsgrad's running maximum of
    v) and ema (the weight average) are lists of depth*12 tensors shaped like the parameters, None without the option;
    skipped = the int64 count of steps that SKIP_NONFINITE refused (0-dim; in the header of every state).  Launches nothing."""
    shapes = _param_shapes(nz, width, coupling) * depth
    sizes = [a * b for a, b in shapes]
    n4 = (sum(sizes) + 3) // 4 * 4
    h = ADAM_HEADER_BYTES // 4
    if state.numel() < h + (2 + bool(amsgrad) + bool(ema)) * n4:
        raise LsnfError(f"state has {state.numel()} floats: not one of new_adam_state(amsgrad={bool(amsgrad)}, ema={bool(ema)})")

    def array(k):
        return [t.view(sh) for t, sh in zip(state[h + k * n4: h + k * n4 + sum(sizes)].split(sizes), shapes)]
    skipped = state[ADAM_SKIPPED_OFFSET // 4: ADAM_SKIPPED_OFFSET // 4 + 2].view(torch.int64)[0]
    return (array(2) if amsgrad else None), (array(2 + bool(amsgrad)) if ema else None), skipped


def adam_step(params: Sequence[torch.Tensor], grads: Sequence[Optional[torch.Tensor]], state: torch.Tensor,
              nz: int, width: int, depth: int, coupling: int = 1, *, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
              eps: float = 1e-8, weight_decay: float = 0.0, max_norm: Optional[float] = None,
              lr_dev: Optional[torch.Tensor] = None, want_norm: bool = False, amsgrad: bool = False, maximize: bool = False,
              decoupled_weight_decay: bool = False, ema_decay: Optional[float] = None,
              skip_nonfinite: bool = False) -> Optional[torch.Tensor]:
    """Global-norm clip + Adam on the device (`lsnf_adam_step`; train.py:413-415): updates the depth*12 tensors `params` in
    place from `grads` (a None entry skips that tensor: parameter, m and v keep their bits, as torch treats `grad is None`)
    and the moments in `state` (`new_adam_state`).  torch.optim.Adam's arithmetic (L2 weight decay);
    max_norm: clip the global gradient norm first (`clip_grad_norm_`'s formula), None = no clipping.  lr_dev: one float32 on
    the device that replaces `lr` (schedules under a captured graph).  Returns the pre-clip global norm as a 0-dim view of the
    state's norm slot when max_norm is given or want_norm or skip_nonfinite is set (the norm launch runs only then), else None.
    Variants (`lsnf_adam_step_ex`; none set: the call above, bit for bit): amsgrad, maximize, decoupled_weight_decay (AdamW:
    p *= 1 - lr * weight_decay instead of g += weight_decay * p) as in torch; ema_decay: keep an exponential moving average of
    the written parameters in the state (a tensor without a gradient takes part; the average starts from the parameters the
    first step finds); skip_nonfinite: a step whose gradient norm is inf or NaN writes nothing but the norm and the state's
    skipped count.  amsgrad and ema_decay need a state made with them and are passed at every call on it.
    One or two launches on the current stream, no synchronisation, no allocation.  Plans prepared from `params` are stale
    afterwards.  Every argument is checked before anything is launched; a bad one raises LsnfError."""
    lib = _lib.load()
    geo = (int(nz), int(width), int(depth), int(coupling))
    nz, width, depth, coupling = geo
    n = depth * LSNF_PARAMS_PER_BLOCK
    if len(params) != n or len(grads) != n:
        raise LsnfError(f"expected {n} parameter tensors and {n} gradients (None allowed), got {len(params)} and {len(grads)}")
    if state is None:
        raise LsnfError("state is required (new_adam_state())")
    flags = 0
    ema = ema_decay is not None
    if amsgrad or maximize or decoupled_weight_decay or skip_nonfinite or ema:      # (one test on the plain step's path)
        if ema and not 0.0 <= float(ema_decay) < 1.0:
            raise LsnfError(f"ema_decay must lie in [0, 1) or be None (got {ema_decay})")
        flags = (_adam_size_flags(amsgrad, ema) | (ADAM_MAXIMIZE if maximize else 0) | (ADAM_DECOUPLED if decoupled_weight_decay else 0)
                 | (ADAM_SKIP_NONFINITE if skip_nonfinite else 0))
    # the checks and the pointer tables are kept per state buffer, keyed by the tensors' addresses (as backward_params does):
    # a training loop hands over the same storages every step
    key = (geo, state.numel(), tuple(t.data_ptr() for t in params), tuple(0 if g is None else g.data_ptr() for g in grads),
           flags & (ADAM_AMSGRAD | ADAM_EMA))
    tab = _adam_tables.get(state.data_ptr())
    if tab is None or tab[0] != key:
        need = adam_state_bytes(*geo, amsgrad, ema)
        if need == 0:
            raise LsnfError(f"unsupported geometry nz={nz} width={width} depth={depth} coupling={coupling}")
        dev = state.device
        _check_out(state, "state", need // 4, dev, hint=f"from new_adam_state({'amsgrad=True' if amsgrad else ''}{', ' if amsgrad and ema else ''}{'ema=True' if ema else ''})")
        if state.data_ptr() % 16:
            raise LsnfError("state must be 16-byte aligned")
        _check_params(params, nz, width, depth, coupling, dev, "state")
        for i, (t, g) in enumerate(zip(params, grads)):
            _check_in(g, f"grad of param[{i}] ({BLOCK_PARAM_KEYS[i % LSNF_PARAMS_PER_BLOCK]})", t.numel(), dev)
        if len(_adam_tables) >= 16:
            _adam_tables.clear()
        tab = _adam_tables[state.data_ptr()] = (key, (ctypes.c_void_p * n)(*key[2]), (ctypes.c_void_p * n)(*[p or None for p in key[3]]))
    dev = state.device
    if lr_dev is not None:
        _check_out(lr_dev, "lr_dev", 1, dev)
    norm = state[ADAM_NORM_OFFSET // 4] if (max_norm is not None or want_norm or skip_nonfinite) else None
    mn = 0.0 if max_norm is None else float(max_norm)
    if flags == 0:
        _call("lsnf_adam_step", dev, tab[1], tab[2], nz, width, depth, coupling, _ptr(state), float(lr), _ptr(lr_dev),
              float(betas[0]), float(betas[1]), float(eps), float(weight_decay), mn, _ptr(norm))
    else:
        opts = _lib.LsnfAdamOptions(ctypes.sizeof(_lib.LsnfAdamOptions), flags, float(lr), _ptr(lr_dev), float(betas[0]), float(betas[1]),
                                    float(eps), float(weight_decay), mn, float(ema_decay) if ema else 0.0, _ptr(norm))
        _call("lsnf_adam_step_ex", dev, tab[1], tab[2], nz, width, depth, coupling, _ptr(state), ctypes.byref(opts))
    return norm


# ---- Markov-chain extensions (include/lsnf_flow_mcmc.h): defined in mcmc.py on this file's checking path, used as flow.mala_step, flow.reverse_mala_step etc.
from .mcmc import MALA_INIT, MalaState, new_mala_state, mala_step, reverse_mala_step  # noqa: E402,F401
from .mcmc import HMC_INIT, HMC_INNER, HmcState, new_hmc_state, hmc_step, reverse_hmc_step  # noqa: E402,F401
from .mcmc import HMC_ADAPT, HMC_ADAPT_LAST, HmcRowSteps, new_hmc_row_steps, hmc_step_rows, reverse_hmc_step_rows  # noqa: E402,F401
from .mcmc import (HMC_METRIC_CLOSE, HMC_METRIC_FOLD, HmcRowMetric, new_hmc_row_metric, hmc_step_metric,  # noqa: E402,F401
                   reverse_hmc_step_metric)
from .mcmc import HMC_ANNEAL, HmcRowTemper, new_hmc_row_temper, hmc_step_tempered, reverse_hmc_step_tempered  # noqa: E402,F401
from .mcmc import HMC_SWAP, HMC_SWAP_ODD, hmc_step_exchange, reverse_hmc_step_exchange  # noqa: E402,F401
from .mcmc import HMC_RESAMPLE, hmc_step_resample, reverse_hmc_step_resample  # noqa: E402,F401
from .mcmc import HMC_SCHEDULE, hmc_step_schedule, reverse_hmc_step_schedule  # noqa: E402,F401

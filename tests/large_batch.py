"""The batch sizes at which the library leaves its 32-bit-offset kernels: one table for tests/test_large_batch_cpu.py and
tests/test_gpu_large_batch.py (not a test module; the CPU module holds the table to its classes).

Two kernel families address memory through buffer descriptors with 32-bit byte offsets and use the offset 2^31 as an "always
out of range" sentinel for padded column groups, so each may run only while its descriptors' extents stay below 2^31 bytes:
  * the STASH instantiations of lsnf_fwd3q_kernel (csrc/lsnf_fwd3p.hip; rule: lsnf_forward3q_covers) -- the STASH guard
    B * nz * 4 < 2^31 and act per_block * 4 < 2^31 with any part of the stash, the DUMP guard (B + 32) * width * 4 < 2^31 with the
    tiled h dump;
  * lsnf_contract_x3_kernel (csrc/lsnf_params3.hip; rule: lsnf_contract_x3_covers) -- the CONTRACTION guard
    (B + 32) * 128 * 4 < 2^31, which csrc/lsnf_api.hip dump_may_tile follows: from there the forward's h dump is row-major, the
    backward's g arrays are row-major and the contraction is the fp32 LDS kernel.
Everything below is restated in exact Python integers; the kernels' own 32-bit arithmetic is restated in numpy.uint32.

A case is (nz, width, depth, coupling, B), tagged with the guard it is for, the side of it B lies on and the kernels the
default dispatch (LSNF_MATH_BF16X3, automatic small-batch threshold) selects there."""
import numpy as np

from chain_geometries import TILE, pick_tiles

LIMIT = 1 << 31                              # extent of a buffer descriptor (bytes) from which the sentinel offset is in range
SENTINEL = 0x80000000                        # csrc/lsnf_fwd3p.hip stash_row_quad / stash_h_quad, csrc/lsnf_params3.hip x3_task
MAX_B = 1 << 28                              # csrc/lsnf_api.hip Check::batch
X3_MIN_ROWS = 12288                          # csrc/lsnf_layout.h LSNF_X3_MIN_ROWS
DET_MAX_CHUNKS = 128                         # csrc/lsnf_layout.h LSNF_DET_MAX_CHUNKS
SMALL_MAX_AUTO = 16384                       # the automatic small-batch threshold of the bf16x3 family (csrc/lsnf_api.hip)


# ---- layouts: csrc/lsnf_layout.h, documented in include/lsnf_flow.h ----------------------------------------------------
def al4(x):
    """LSNF_AL4"""
    return (x + 3) // 4 * 4


def act_layout(B, HT, WT):
    """lsnf_act_layout: (per_tile, per_block, mask_off) in floats."""
    mask_off = HT * 1024
    per_tile = mask_off + 2 * WT * 64
    return per_tile, per_tile * ((B + 31) // 32), mask_off


def act_saved_floats(geo, B):
    """lsnf_act_saved_floats (csrc/lsnf_api.hip): depth * per_block, independent of the coupling."""
    nz, width, depth = geo[:3]
    HT, WT = pick_tiles(nz // 2, width)
    return depth * act_layout(B, HT, WT)[1]


def dump_layout(B, nz, width):
    """lsnf_dump_layout: offsets of g_v, g_a1, g_a2, g_t, g_p, h1, h2 and the floats per block; rows in whole 32-row tiles."""
    b, half, o, offs = (B + 31) // 32 * 32, nz // 2, 0, {}
    for name, cols in (("gv", nz), ("ga1", width), ("ga2", width), ("gt", half), ("gp", half), ("h1", width), ("h2", width)):
        offs[name] = o
        o = al4(o + b * cols)
    offs["per_block"] = o
    return offs


def fold_per_block(nz, width):
    """lsnf_fold_layout(...).per_block: the folded gradients of one block."""
    half = nz // 2
    return al4(nz * nz + nz + half * width + width + width * width + width + 2 * (width * half + half))


def params_workspace_floats(geo, B):
    """lsnf_backward_params_workspace_floats: 4 (G) + the folds + the dumps + 4 (the tag word)."""
    nz, width, depth = geo[:3]
    return 4 + depth * fold_per_block(nz, width) + depth * dump_layout(B, nz, width)["per_block"] + 4


def det_chunk_rows(B, depth, x3):
    """lsnf_det_chunk_rows.  bf16 contraction: 256 / depth chunks in whole 32-row stages.  fp32 contractions: 128 rows per chunk
    below 16 384 rows, 512 from there, and more rows per chunk (whole 16-row stages) once that would exceed 128 chunks."""
    if x3:
        chunks = max(256 // depth, 1)
        return (-(-B // chunks) + 31) // 32 * 32
    chunk = 512 if B >= 16384 else 128
    if -(-B // chunk) > DET_MAX_CHUNKS:
        chunk = (-(-B // DET_MAX_CHUNKS) + 15) // 16 * 16
    return chunk


MAX_GRID_Y = 65535                           # csrc/lsnf_params.hip lsnf_launch_params_contract kMaxGridY


def contract_chunk_rows(B):
    """csrc/lsnf_params.hip lsnf_launch_params_contract, the fp32 contractions outside the deterministic form: 128 rows per chunk
    below 16 384 rows, 512 from there; the chunks are the grid's y extent, so beyond 65 535 of them the chunk grows in whole
    16-row stages."""
    chunk = 512 if B >= 16384 else 128
    if -(-B // chunk) > MAX_GRID_Y:
        chunk = (-(-B // MAX_GRID_Y) + 15) // 16 * 16
    return chunk


def det_chunks(B, depth, x3):
    """lsnf_det_chunks"""
    return 0 if B < 1 else -(-B // det_chunk_rows(B, depth, x3))


def det_workspace_floats(geo, B):
    """lsnf_backward_params_det_workspace_floats: the default workspace rounded up to 16 bytes, then one image of the folds per
    chunk -- the larger of the two kinds' chunk counts where the bf16 contraction can run at all."""
    nz, width, depth = geo[:3]
    chunks = max(det_chunks(B, depth, 0), det_chunks(B, depth, 1) if B >= X3_MIN_ROWS else 0)
    return al4(params_workspace_floats(geo, B)) + chunks * depth * fold_per_block(nz, width)


def actnorm_init_workspace_bytes(geo, B):
    """lsnf_actnorm_init_workspace_bytes (csrc/lsnf_init.hip): one slab of 2 x 128 doubles per 64 rows, then two (B, nz) and two
    (B, width) float buffers."""
    nz, width = geo[:2]
    return -(-B // 64) * 128 * 2 * 8 + 4 * B * (2 * nz + 2 * width)


def forward_gb(geo, B):
    """Device memory of a stash forward case (bytes): z, z1, the block outputs, the stash, logdet and ll."""
    nz, _, depth = geo[:3]
    return 4 * (B * nz * (1 + depth) + act_saved_floats(geo, B) + 2 * B)


def params_gb(geo, B):
    """Device memory of a parameter-gradient case (bytes): the forward's tensors, g_z1, g_logdet, dL/dz and the deterministic
    workspace (which serves all three paths)."""
    nz = geo[0]
    return forward_gb(geo, B) + 4 * (2 * B * nz + B + det_workspace_floats(geo, B))


# ---- the three guards --------------------------------------------------------------------------------------------------
def stash_covers(geo, B):
    """csrc/lsnf_fwd3p.hip lsnf_forward3q_covers, the part under `stash` (16-byte aligned tensors, vec4 == 4 taken as given)."""
    nz, width = geo[:2]
    HT, WT = pick_tiles(nz // 2, width)
    return (HT, WT) == (2, 2) and B * nz * 4 < LIMIT and act_layout(B, HT, WT)[1] * 4 < LIMIT


def dump_covers(geo, B):
    """csrc/lsnf_fwd3p.hip lsnf_forward3q_covers, the extent of the tiled h dump."""
    return (B + 32) * geo[1] * 4 < LIMIT


def contract_covers(geo, B):
    """csrc/lsnf_params3.hip lsnf_contract_x3_covers (16-byte aligned z tensors, no knob set)."""
    nz, width = geo[:2]
    half = nz // 2
    return B >= X3_MIN_ROWS and nz % 4 == 0 and width % 4 == 0 and half % 4 == 0 and (B + 32) * 128 * 4 < LIMIT


def dump_may_tile(geo, B, small_max=SMALL_MAX_AUTO):
    """csrc/lsnf_api.hip dump_may_tile under LSNF_MATH_BF16X3: csrc/lsnf_layout.h lsnf_dump_can_tile and the contraction's rule."""
    nz, width = geo[:2]
    return B > small_max and nz % 64 == 0 and width % 16 == 0 and contract_covers(geo, B)


def act_first_refused(geo):
    """The first B at which act per_block * 4 reaches 2^31 (the second clause of the stash guard)."""
    HT, WT = pick_tiles(geo[0] // 2, geo[1])
    per_tile = act_layout(32, HT, WT)[0]
    return (-(-LIMIT // (per_tile * 4)) - 1) * 32 + 1


GUARDS = {
    "stash": (stash_covers, lambda geo: min(-(-LIMIT // (geo[0] * 4)), act_first_refused(geo))),
    "dump": (dump_covers, lambda geo: -(-LIMIT // (geo[1] * 4)) - 32),
    "contract": (contract_covers, lambda geo: LIMIT // (128 * 4) - 32),
}


def first_refused(guard, geo):
    """The first B (above LSNF_X3_MIN_ROWS) that `guard` turns away at geometry `geo`."""
    covers, closed_form = GUARDS[guard]
    G = closed_form(geo)
    assert covers(geo, G - 1) and not covers(geo, G), (guard, geo, G)
    return G


# ---- which kernels the default dispatch selects (csrc/lsnf_api.hip select_forward / select_backward / select_contraction) ----
FWD3Q_DUMP, FWD3Q_STASH, FWD3B = "lsnf_fwd3q_kernel<2, 8, 2, 2", "lsnf_fwd3q_kernel<2, 8, 2, 1", "lsnf_fwd3b_kernel"
X3, X3_DET, LDS4, LDS4_DET = ("lsnf_contract_x3_kernel<false>", "lsnf_contract_x3_kernel<true>", "lsnf_tn_gemm_lds_kernel<4, false>",
                              "lsnf_tn_gemm_lds_kernel<4, true>")
BWD3 = "lsnf_bwd3"                           # the throughput backward from the stash (csrc/lsnf_bwd3.hip), any instantiation
BWD_RECOMPUTE = "lsnf_bwd_"                  # the recomputing fp32-MFMA backward of the path without a stash (csrc/lsnf_bwd.hip)


def expected_kernels(geo, B, call):
    """call: "stash" (forward with z_saved + act_saved) or "params" (the fast path: forward with the dump, backward, contraction).
    Returns {"forward": ..., "contraction": ... or None}: name prefixes as a kernel trace prints them."""
    tiled = dump_may_tile(geo, B) and B >= X3_MIN_ROWS
    if call == "stash":
        return {"forward": FWD3Q_STASH if stash_covers(geo, B) else FWD3B, "contraction": None}
    # the dump guard is shadowed: a tiled dump needs the contraction's rule (B < 4 194 272) and the stash's (B * nz * 4 < 2^31, nz = 128)
    q = tiled and geo[1] % 16 == 0 and dump_covers(geo, B) and stash_covers(geo, B)
    return {"forward": FWD3Q_DUMP if q else FWD3B, "contraction": X3 if contract_covers(geo, B) else LDS4}


# ---- the table ---------------------------------------------------------------------------------------------------------
HEADLINE, RAGGED_HALF, RAGGED_WIDTH = (128, 64, 2, 1), (120, 48, 2, 1), (128, 48, 2, 1)
GEOS = {
    HEADLINE: "no padded column group: only a 2^32 wrap-around could hurt it",
    RAGGED_HALF: "half 60 pads the last four-column group of the second half tile: stash_row_quad's sentinel",
    RAGGED_WIDTH: "may tile its dump; width 48 pads the last 16-column half tile of h: stash_h_quad's and x3_segment's sentinel",
}
PAST = 65                                    # G + 65: two whole 32-row tiles and one row past the guard -- a ragged last tile


def past_of(guard, geo):
    """G + 65 -- at the headline geometry, whose two guards are 32 rows apart, the one size past both: the stash guard's G + 65."""
    return first_refused("stash" if geo == HEADLINE else guard, geo) + PAST


def _sides(guard, geo, call):
    G = first_refused(guard, geo)
    return [(geo + (B,), guard, side, call) for B, side in ((G - 1, "below"), (G, "at"), (past_of(guard, geo), "past"))]


# (case, guard, side, call)
TABLE = (_sides("contract", HEADLINE, "params") + _sides("stash", HEADLINE, "stash") + _sides("stash", RAGGED_HALF, "stash")
         + _sides("contract", RAGGED_WIDTH, "params"))
# the headline geometry's two guards are 32 rows apart: its parameter-gradient sizes also stand on both sides of the stash guard
assert first_refused("stash", HEADLINE) - first_refused("contract", HEADLINE) == 32
HEADLINE_SIZES = [4194271, 4194272, 4194303, 4194304, 4194369]
assert sorted({c[4] for c, g, _, _ in TABLE if c[:4] == HEADLINE}) == HEADLINE_SIZES

STASH_CASES = [c for c, g, s, call in TABLE if call == "stash"]
PARAMS_CASES = [c for c, g, s, call in TABLE if call == "params"] + [HEADLINE + (first_refused("stash", HEADLINE),)]
CHAIN_CASE = HEADLINE + (4194369,)           # reverse, sample and the Langevin step
ALL_B = sorted({c[4] for c, _, _, _ in TABLE} | {MAX_B})


# ---- windows -----------------------------------------------------------------------------------------------------------
MAX_WINDOW_ROWS = 4096


def sentinel_row(geo):
    """The row whose bytes hold byte 2^31 of a (B, nz) tensor: where a sentinel store would land behind a descriptor of >= 2^31 bytes."""
    return LIMIT // (4 * geo[0])


def windows(case):
    """[(first row, end row)]: rows 0-63, the 128 rows around B / 2, the last 160 rows with their ragged tile, and the 64 rows
    around the sentinel row where the batch holds it."""
    B = case[4]
    w = [(0, 64), (B // 2 - 64, B // 2 + 64), (B - 160, B)]
    s = sentinel_row(case)
    if s + 32 < B - 160:
        w.insert(2, (s - 32, s + 32))
    elif s < B:                              # inside (or next to) the last window: widen that one
        w[-1] = (min(s - 32, B - 160), B)
    assert sum(b - a for a, b in w) <= MAX_WINDOW_ROWS and all(0 <= a < b <= B for a, b in w)
    return w


def in_windows(case, row):
    return any(a <= row < b for a, b in windows(case))


LIVE_ROWS, LIVE_TAIL = 2048, 700


def live_runs(B):
    """The live rows of a parameter-gradient case: three runs -- from row 0, straddling B / 2, the last 700 rows."""
    n = (LIVE_ROWS - LIVE_TAIL) // 2
    return [(0, n), (B // 2 - n // 2, B // 2 - n // 2 + n), (B - LIVE_TAIL, B)]


# ---- the kernels' 32-bit offset arithmetic, in numpy.uint32 -------------------------------------------------------------------
def _u32(x):
    return np.uint32(int(x) & 0xFFFFFFFF)


def _lands(extent, off):
    """A raw buffer access of 16 bytes at byte offset `off` behind a descriptor of `extent` bytes (uint32 num_records, raw
    addressing): in range iff off + 16 <= extent."""
    return int(off) + 16 <= int(extent)


def stash_padded_accesses(geo, B):
    """Every padded-group store of the STASH forward's row writes (csrc/lsnf_fwd3p.hip stash_row_quad) at batch size B with the
    guard imagined absent: [(row, column)] of the stores that would land in the (B, nz) tensor.  zbytes, the second descriptor
    (base + half * 4, zbytes - half * 4) and the sentinel as the kernel forms them; the store offset is
    sentinel + (32 tt + 16 ft) * 4 behind descriptor hh."""
    nz, half = geo[0], geo[0] // 2
    with np.errstate(over="ignore"):
        zbytes = _u32(B) * _u32(nz) * _u32(4)
        second = _u32(half * 4)
        extents = (zbytes, zbytes - second if zbytes > second else _u32(0))
        hits = []
        for hh in (0, 1):
            for tt in (0, 1):
                for ft in (0, 1):
                    for g in range(4):
                        if 32 * tt + 16 * ft + 4 * g < half:
                            continue                 # a real group: sl.zoff, not the sentinel
                        off = _u32(SENTINEL) + _u32((32 * tt + 16 * ft) * 4)
                        if _lands(extents[hh], off):
                            byte = int(off) + hh * half * 4
                            hits.append((byte // (4 * nz), byte % (4 * nz) // 4))
    return sorted(set(hits))


def stash_zoff_wraps(geo, B):
    """sl0.zoff = ((wbase + n) * nz + 4 g) * 4 in uint32 for the last row a workgroup of the launch can own (grids of 256 rows):
    True if it differs from the exact offset."""
    nz = geo[0]
    row = -(-B // 256) * 256 - 1
    with np.errstate(over="ignore"):
        off = (_u32(row) * _u32(nz) + _u32(12)) * _u32(4) + _u32(16 * nz * 4)
    return int(off) != (row * nz + 12) * 4 + 16 * nz * 4


def x3_padded_accesses(geo, B, ld, ncols, chunk_rows, col0=0):
    """The dead column groups of one operand segment of the bf16 contraction (csrc/lsnf_params3.hip x3_segment / x3_task) at batch
    size B with the guard imagined absent: a segment of `ncols` < 64 live columns, starting at column `col0`, of a row-major
    (B, ld) array -- x3_segment moves the descriptor's base to col0 and takes col0 floats off its extent.  A dead group starts at
    voff = 2^31 and advances by 32 * ld * 4 per stage, eight loads of 16 * ld bytes apart per stage, three stages ahead of the
    chunk's end.  Returns [(row, column)] of the loads that would be in range.  Such a load is harmless in itself: what a dead group
    loads is never written to LDS (`live` gates the split and the write in x3_task).  This is the reading of what the sentinel
    relies on, not evidence that a GPU window would see a missing guard."""
    with np.errstate(over="ignore"):
        extent = _u32((B * ld - col0) * 4)       # (int)(floats * 4) of x3_segment, as the descriptor's uint32 num_records
        hits = []
        if ncols >= 64:
            return hits
        step, jstride = _u32(32 * ld * 4), _u32(16 * ld)
        voff = _u32(SENTINEL)
        for _ in range(-(-chunk_rows // 32) + 3):
            for j in range(8):
                off = voff + _u32(j) * jstride
                if _lands(extent, off):
                    byte = int(off) + col0 * 4
                    hits.append((byte // (4 * ld), byte % (4 * ld) // 4))
            voff = voff + step
    return hits


def x3_voff_exact(B, ld):
    """x3_voff of the last stage of the batch, row-major, for the last thread (rg = 3, col = 60): ((m0 + rg) * ld + col) * 4 in
    numpy.int32 as the kernel computes it, cast to uint32, then the kernel's uint32 additions up to the last load of the third stage
    fetched ahead (voff += step three times, + 7 * jstride).  True if every value equals the exact integer."""
    m0 = (B - 1) // 32 * 32
    with np.errstate(over="ignore"):
        first = (np.int32(m0 + 3) * np.int32(ld) + np.int32(60)) * np.int32(4)
        last = _u32(int(first)) + _u32(3) * _u32(32 * ld * 4) + _u32(7) * _u32(16 * ld)
    exact = ((m0 + 3) * ld + 60) * 4
    return int(first) == exact and int(last) == exact + 3 * 32 * ld * 4 + 7 * 16 * ld

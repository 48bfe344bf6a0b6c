"""CPU: tests/large_batch.py holds what it claims -- every tabled batch size on the side of its guard that its tag says, every
guard with a case on either side, the sentinel row inside a compared window -- and the library's size queries, asked without a
device at every tabled size and at the largest admitted batch (2^28), equal the exact-integer restatement of the layouts of
include/lsnf_flow.h and csrc/lsnf_layout.h.  The 32-bit offset arithmetic of the two buffer-addressed kernel families, restated in
numpy.uint32, shows where a padded-group access would land were a guard absent: the evidence that the windows of
tests/test_gpu_large_batch.py have teeth (no guard mutant is run on a device)."""
import ctypes

import pytest

import large_batch as L
import lsnf_amd


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(lsnf_amd._lib.LIB_PATH)
    for name, n in (("lsnf_act_saved_floats", 4), ("lsnf_backward_params_workspace_floats", 4),
                    ("lsnf_backward_params_det_workspace_floats", 4), ("lsnf_actnorm_init_workspace_bytes", 5)):
        f = getattr(lib, name)
        f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int] * n
    return lib


def test_first_refused_of_every_guard():
    assert L.first_refused("stash", L.HEADLINE) == 4194304 == L.first_refused("stash", L.RAGGED_WIDTH)
    assert L.first_refused("stash", L.RAGGED_HALF) == 4473925
    for geo in L.GEOS:
        assert L.first_refused("contract", geo) == 4194272         # whatever the geometry
        assert L.pick_tiles(geo[0] // 2, geo[1]) == (2, 2) and geo[2:] == (2, 1)
    assert L.first_refused("dump", L.HEADLINE) == 8388576 and L.first_refused("dump", L.RAGGED_WIDTH) == 11184779
    # the act per_block clause is first reached below nz = 74: 2^31 / (4 nz) rows lie above its 7 456 513 from there down
    assert L.act_first_refused(L.HEADLINE) == 7456513
    assert L.first_refused("stash", (72, 64, 2, 1)) == 7456513 < -(-L.LIMIT // (72 * 4))
    assert L.first_refused("stash", (74, 64, 2, 1)) == -(-L.LIMIT // (74 * 4)) < 7456513
    _, per_block, _ = L.act_layout(7456513, 2, 2)
    assert per_block * 4 >= L.LIMIT > L.act_layout(7456512, 2, 2)[1] * 4


def test_every_case_lies_on_the_side_its_tag_claims():
    seen = set()
    for case, guard, side, call in L.TABLE:
        geo, B = case[:4], case[4]
        covers, G = L.GUARDS[guard][0], L.first_refused(guard, geo)
        assert side == {G - 1: "below", G: "at", L.past_of(guard, geo): "past"}[B]
        assert covers(geo, B) == (side == "below"), (case, guard, side)
        assert L.X3_MIN_ROWS < B <= L.MAX_B and (side != "past" or (B % 32 != 0 and B >= G + L.PAST))     # a ragged tile past the guard
        seen.add((guard, geo, side))
    for guard, geo in (("contract", L.HEADLINE), ("stash", L.HEADLINE), ("stash", L.RAGGED_HALF), ("contract", L.RAGGED_WIDTH)):
        assert {(guard, geo, s) for s in ("below", "at", "past")} <= seen       # an edit cannot drop a class
    assert [c[4] for c in L.PARAMS_CASES if c[:4] == L.HEADLINE] == [4194271, 4194272, 4194369, 4194304]
    assert {c[4] for c in L.STASH_CASES if c[:4] == L.HEADLINE} == {4194303, 4194304, 4194369}
    assert L.CHAIN_CASE[4] == 4194369 and len(L.STASH_CASES) == 6 and len(L.PARAMS_CASES) == 7


def test_the_dump_guard_is_shadowed_under_default_dispatch():
    """A tiled dump needs dump_may_tile, hence the contraction's rule: B < 4 194 272, where (B + 32) * width * 4 <= 2^30 for every
    width the <2, 2> kernel takes -- and a dump goes with act_saved, hence the stash guard, which at nz = 128 (the one nz of the
    <2, 2> kernel that may tile) stops at 4 194 304."""
    for width in (16, 32, 48, 64):
        geo = (128, width, 2, 1)
        G = L.first_refused("dump", geo)
        assert G > L.first_refused("contract", geo) and G > L.first_refused("stash", geo)
        assert not L.dump_may_tile(geo, G - 1) and not L.dump_may_tile(geo, L.first_refused("contract", geo))
        assert L.dump_may_tile(geo, L.first_refused("contract", geo) - 1)
        assert (L.first_refused("contract", geo) - 1 + 32) * width * 4 <= 1 << 30


def test_expected_kernels_follow_the_guards():
    want = {("contract", "below"): (L.FWD3Q_DUMP, L.X3), ("contract", "at"): (L.FWD3B, L.LDS4), ("contract", "past"): (L.FWD3B, L.LDS4),
            ("stash", "below"): (L.FWD3Q_STASH, None), ("stash", "at"): (L.FWD3B, None), ("stash", "past"): (L.FWD3B, None)}
    for case, guard, side, call in L.TABLE:
        k = L.expected_kernels(case[:4], case[4], call)
        assert (k["forward"], k["contraction"]) == want[(guard, side)], (case, guard, side)


def test_windows_hold_the_sentinel_row_and_stay_small():
    for case in L.STASH_CASES + [L.CHAIN_CASE]:
        w = L.windows(case)
        B, s = case[4], L.sentinel_row(case)
        assert w[0] == (0, 64) and w[1] == (B // 2 - 64, B // 2 + 64) and w[-1][1] == B and w[-1][0] <= B - 160
        assert sum(b - a for a, b in w) <= L.MAX_WINDOW_ROWS
        assert all(a1 >= b0 for (_, b0), (a1, _) in zip(w, w[1:]))             # disjoint, ascending
        if s < B:
            assert L.in_windows(case, s) and (s + 1 >= B or L.in_windows(case, s + 1))
    past = L.RAGGED_HALF + (L.first_refused("stash", L.RAGGED_HALF) + L.PAST,)
    assert L.sentinel_row(past) == 4473924 < past[4] and L.in_windows(past, 4473924) and L.in_windows(past, 4473925)
    for B in {c[4] for c in L.PARAMS_CASES}:
        runs = L.live_runs(B)
        assert sum(b - a for a, b in runs) == L.LIVE_ROWS and runs[0][0] == 0 and runs[-1] == (B - L.LIVE_TAIL, B)
        assert runs[1][0] < B // 2 < runs[1][1] and runs[0][1] < runs[1][0] and runs[1][1] < runs[2][0]


def test_size_queries_match_the_restated_layouts(lib):
    for geo in L.GEOS:
        nz, width, depth, coupling = geo
        for B in L.ALL_B:
            assert lib.lsnf_act_saved_floats(nz, width, depth, B) == L.act_saved_floats(geo, B), (geo, B)      # the stash size query
            assert lib.lsnf_backward_params_workspace_floats(nz, width, depth, B) == L.params_workspace_floats(geo, B), (geo, B)
            assert lib.lsnf_backward_params_det_workspace_floats(nz, width, depth, B) == L.det_workspace_floats(geo, B), (geo, B)
            assert lib.lsnf_actnorm_init_workspace_bytes(nz, width, depth, coupling, B) == L.actnorm_init_workspace_bytes(geo, B), (geo, B)
    # spelled out once at the headline geometry: 2 304 stash floats per 32-row tile and block; 512 dump floats per row and block
    assert L.act_saved_floats(L.HEADLINE, 4194304) == 2 * 2304 * 131072
    assert L.params_workspace_floats(L.HEADLINE, 4194304) == 4 + 2 * L.fold_per_block(128, 64) + 2 * 512 * 4194304 + 4
    assert L.fold_per_block(128, 64) * 4 * 5 == 663040           # include/lsnf_flow.h: "663 040 bytes per chunk" at depth 5
    # the sizes the GPU module states: ~9 GB a forward case, ~30 GB a parameter-gradient case
    assert 8.5e9 < L.forward_gb(L.HEADLINE, 4194304) < 9.5e9 and 29e9 < L.params_gb(L.HEADLINE, 4194304) < 32e9


def test_deterministic_chunking_follows_the_headers_rule():
    """include/lsnf_flow.h: at most 128 chunks for the fp32-MFMA contractions (128 rows per chunk below 16 384 rows, 512 from there,
    more once that would exceed 128 chunks), 256 / depth chunks for the bf16 contraction."""
    for depth in (1, 2, 5, 16):
        for B in L.ALL_B:
            rows, n = L.det_chunk_rows(B, depth, 0), L.det_chunks(B, depth, 0)
            assert n <= 128 and rows % 16 == 0 and (n - 1) * rows < B <= n * rows
            assert rows > 512 and rows - 16 < -(-B // 128) <= rows          # "more rows per chunk": first applies above 65 536 rows
            rows3, n3 = L.det_chunk_rows(B, depth, 1), L.det_chunks(B, depth, 1)
            assert n3 <= max(256 // depth, 1) and rows3 % 32 == 0 and (n3 - 1) * rows3 < B <= n3 * rows3
    assert L.det_chunk_rows(65536, 2, 0) == 512 and L.det_chunk_rows(65537, 2, 0) == 528
    assert L.det_chunk_rows(4194272, 2, 0) == 32768 and L.det_chunks(4194272, 2, 0) == 128
    assert L.det_chunk_rows(4194271, 2, 1) == 32768 and L.det_chunks(4194271, 2, 1) == 128
    assert L.det_chunks(L.MAX_B, 2, 0) == 128 and L.det_chunk_rows(L.MAX_B, 2, 0) == 1 << 21


def test_fp32_contraction_grid_stays_launchable():
    """The fp32 contraction puts its chunks on the grid's y axis.  With 512-row chunks that axis passed 65 535 above 33.5 M rows, inside
    the admitted 2^28; the chunk now grows there.  At every tabled size the chunk is still 512 rows."""
    for B in L.ALL_B + [33553920, 33553921, 1 << 27]:
        rows = L.contract_chunk_rows(B)
        assert -(-B // rows) <= L.MAX_GRID_Y and rows % 16 == 0
        assert (rows == 512) == (B <= 512 * L.MAX_GRID_Y)
    assert L.contract_chunk_rows(L.MAX_B) == 4112 and -(-L.MAX_B // 4112) == 65281


def test_stash_forward_offsets_in_uint32():
    """csrc/lsnf_fwd3p.hip: zbytes, sl.zoff, the second descriptor and the sentinel.  Below the guard no padded-group store lands
    and no offset wraps; with the guard imagined absent, the padded group of (120, 48) lands on the sentinel row -- a tabled
    window row -- from G on, and the geometries without a padded group of latent columns have nothing to land."""
    for geo in L.GEOS:
        G = L.first_refused("stash", geo)
        assert L.stash_padded_accesses(geo, G - 1) == [] and not L.stash_zoff_wraps(geo, G - 1)
        assert not L.stash_zoff_wraps(geo, G + L.PAST)          # 2^32 lies far above these sizes
    G = L.first_refused("stash", L.RAGGED_HALF)
    # one padded group (columns 60-63 of a half tile) behind each of the two descriptors: bytes 2^31 + 192 (+ 240); at G itself the
    # second descriptor's 16 bytes still end past its extent
    for B, want in ((G, [(4473924, 80)]), (G + L.PAST, [(4473924, 80), (4473925, 20)])):
        hits = L.stash_padded_accesses(L.RAGGED_HALF, B)
        assert hits == want, hits
        assert all(row < B and L.in_windows(L.RAGGED_HALF + (B,), row) for row, _ in hits)
    assert all(L.in_windows(L.RAGGED_HALF + (G + L.PAST,), row) for row, _ in L.stash_padded_accesses(L.RAGGED_HALF, G + L.PAST))
    for geo in (L.HEADLINE, L.RAGGED_WIDTH):                   # half 64: every group of the latent rows is real
        assert L.stash_padded_accesses(geo, L.first_refused("stash", geo) + L.PAST) == []
    # stash_h_quad's padded half tile (width 48) sits behind a descriptor of (B + 31) / 32 * 32 * width * 4 bytes: 0.8 GB at these
    # sizes, so its sentinel stays out of range until the (shadowed) dump guard at 11 184 779 rows
    assert (L.first_refused("stash", L.RAGGED_WIDTH) + L.PAST + 31) // 32 * 32 * 48 * 4 < L.LIMIT // 2


def _x3_segments(geo):
    """(ld, live columns) of every operand segment of the four tasks of lsnf_contract_x3_kernel that has dead column groups, both
    dump forms: a segment spans 64 columns; A segments [0, 64) and [64, K), G segments by source array."""
    nz, width, half = geo[0], geo[1], geo[0] // 2
    segs = []
    for ld, cols in ((nz, nz), (nz, half), (width, width), (half, half)):       # x / g_v; v1 of y; h1, h2, g_a1, g_a2; g_t, g_p, tiled g_v1
        for ncols in (min(cols, 64), cols - 64):
            if 0 < ncols < 64:
                segs.append((ld, ncols))
    return sorted(set(segs))


def test_contraction_offsets_in_uint32():
    """csrc/lsnf_params3.hip x3_segment / x3_voff.  Below the guard no dead column group reads anything and no offset leaves int32.
    With the guard imagined absent the tabled geometries still read nothing at G + 65: their only arrays with dead groups are
    64 or fewer columns wide (extent <= 2^30 bytes there) -- the guard's constant 128 is the widest operand, whatever the
    geometry.  A geometry whose 128-wide operands have dead groups, (120, 48), shows what the sentinel relies on: from 4 473 925
    rows its loads would be in range.  They would be harmless there (a dead group's loads are never written to LDS), so this part
    is the reading of the guard, not evidence that a GPU window has teeth; that evidence is the stash forward's, above."""
    for geo in L.GEOS:
        G = L.first_refused("contract", geo)
        chunk = L.det_chunk_rows(G - 1, geo[2], 1)
        for ld, ncols in _x3_segments(geo):
            for B in (G - 1, G, G + L.PAST):
                assert L.x3_padded_accesses(geo, B, ld, ncols, chunk) == [], (geo, B, ld, ncols)
        assert all(ld <= 64 or geo == L.RAGGED_HALF for ld, _ in _x3_segments(geo))
        assert L.x3_voff_exact(G - 1, 128) and not L.x3_voff_exact(G + L.PAST, 128)      # int32: m0 * 128 * 4 passes 2^31 at 4 194 304 rows
    assert (120, 56) in _x3_segments(L.RAGGED_HALF)
    first = -(-L.LIMIT // (120 * 4))
    assert L.x3_padded_accesses(L.RAGGED_HALF, first - 1, 120, 56, 32768, col0=64) == []
    hits = L.x3_padded_accesses(L.RAGGED_HALF, first + L.PAST, 120, 56, 32768, col0=64)
    assert hits and hits[0][0] == L.sentinel_row(L.RAGGED_HALF) and first > L.first_refused("contract", L.RAGGED_HALF)

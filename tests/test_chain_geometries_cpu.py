"""The geometry table of the chain-step tests (tests/chain_geometries.py), on the CPU: every class of geometry that the output
sections of the four fused chain kernels treat differently is in the table for every instantiation that has it, so that a later
edit of the table cannot drop one silently; and every module that is to run the table runs it."""
import chain_geometries as G


def pick_tiles(half, width):
    """csrc/lsnf_layout.h lsnf_pick_tiles (LSNF_TILE = 32), restated."""
    ht, wt = (half + 31) // 32, (width + 31) // 32
    return next(((h, w) for h, w in ((1, 1), (2, 2), (2, 4)) if ht <= h and wt <= w), None)


def test_the_tags_are_what_lsnf_pick_tiles_selects():
    for geo, cfg, _ in G.TABLE:
        nz, width, depth, coupling = geo
        assert nz % 2 == 0 and 2 <= nz <= 128 and 1 <= width <= 128 and coupling in (0, 1)       # csrc/lsnf_layout.h lsnf_geo_init
        assert 2 <= depth <= 3                                                                    # milliseconds on the device
        assert pick_tiles(nz // 2, width) == cfg == G.pick_tiles(nz // 2, width), geo
    assert len(set(G.GEOS)) == len(G.GEOS)


def test_every_instantiation_has_every_class():
    by_cfg = {}
    for geo, cfg, _ in G.TABLE:
        by_cfg.setdefault(cfg, []).append(geo)
    assert set(by_cfg) == {(1, 1), (2, 2), (2, 4)}
    for cfg, geos in by_cfg.items():
        halves = [nz // 2 for nz, _, _, _ in geos]
        assert any(h % 4 != 0 for h in halves), cfg
        # a draw of four columns f0 .. f0 + 3 (f0 = 0 mod 4) with a real first column and a padding one behind it
        assert any(any(f0 < h < f0 + 4 for f0 in range(0, 32 * cfg[0], 4)) for h in halves), cfg
        assert any(G.draw_straddles(geo) for geo in geos), cfg
        if cfg[0] == 2:
            assert any(nz // 2 <= 32 for nz, _, _, _ in geos), cfg          # the second half-tile holds no real column
            assert any(G.second_half_tile_empty(geo) for geo in geos), cfg
    # an instantiation with a width tile that holds no real column; additive coupling at a ragged half; no padding at all
    assert any(cfg[1] > (w + 31) // 32 for (_, w, _, _), cfg, _ in G.TABLE) and any(G.a_width_tile_empty(geo) for geo in G.GEOS)
    assert any(coupling == 0 and (nz // 2) % 32 != 0 for nz, _, _, coupling in G.GEOS)
    assert any((nz // 2) % 32 == 0 and w % 32 == 0 and cfg == (2, 4) for (nz, w, _, _), cfg, _ in G.TABLE)


def test_batches_and_call_form_subsets():
    assert G.B_SMALL == 33 and G.CASES == [geo + (33,) for geo in G.GEOS]
    assert G.LARGE == [(66, 33, 2, 1, 4100), (10, 40, 2, 1, 8200)]          # 32 and 64 rows per workgroup: single-call cases
    assert all(c[:4] in G.GEOS for c in G.LARGE + G.FORMS) and len(G.FORMS) == 4
    forms = {c[:4] for c in G.FORMS}
    assert any(G.draw_straddles(g) and not G.second_half_tile_empty(g) for g in forms)
    assert any(G.second_half_tile_empty(g) and G.pick_tiles(g[0] // 2, g[1]) == (2, 2) for g in forms)
    assert any(G.second_half_tile_empty(g) and G.pick_tiles(g[0] // 2, g[1]) == (2, 4) for g in forms)


def test_the_four_modules_run_the_table():
    """Importing the GPU test modules needs no device: their case lists hold every entry, and the in-kernel draw is tested at
    every B = 33 entry."""
    import test_gpu_hmc as TH
    import test_gpu_mala as ZM
    import test_gpu_reverse_langevin as RL
    import test_gpu_rmala as RMt
    for T in (ZM, TH, RL):
        assert set(G.CASES + G.LARGE) <= set(T.CASES), T.__name__
    for T in (ZM, RMt, TH, RL):
        assert set(G.CASES + G.LARGE) <= {r[:5] for r in T.RUNS}, T.__name__
        assert set(G.CASES) <= set(T.PHILOX_CASES), T.__name__
    for T in (ZM, RMt, TH):                         # a step for every entry, keyed by the geometry
        assert set(G.GEOS) <= set(T.STEP_GEO), T.__name__


def test_the_row_metric_tempered_and_exchange_lists_run_the_table():
    """Importing the shared GPU check modules needs no device.  The metric and tempered calls run every entry; the replica-exchange
    swap runs every geometry and both large entries, every ladder size at a straddling half, an empty second half-tile in <2, 2> and
    in <2, 4> and additive coupling; the next trajectory and the in-kernel uniform of a swapping call each run a straddling half and
    an empty half-tile."""
    import hmc_exchange_gpu as XG
    import hmc_metric_gpu as MG
    import hmc_tempered_gpu as TG
    assert set(G.CASES + G.LARGE) <= set(MG.COLUMN) and set(G.CASES + G.LARGE) <= set(TG.GENERAL)
    swap_geos = {c[:4] for c in XG.SWAP}
    assert set(G.GEOS) <= swap_geos
    for large in G.LARGE:
        assert any(c[:5] == large for c in XG.SWAP), large
    for R in (2, 4, 8, 16):
        assert any(c[5] == R and G.draw_straddles(c[:4]) for c in XG.SWAP), R
    for tiles in ((2, 2), (2, 4)):
        assert any(G.second_half_tile_empty(c[:4]) and G.pick_tiles(c[0] // 2, c[1]) == tiles for c in XG.SWAP), tiles
    assert any(c[3] == 0 for c in XG.SWAP)
    for cases in (XG.NEXT, XG.UNIFORM):
        assert any(G.draw_straddles(c[:4]) for c in cases) and any(G.second_half_tile_empty(c[:4]) for c in cases)
    for nz, w, depth, coupling, B, R in XG.SWAP + XG.NEXT + XG.UNIFORM + XG.FORMS:
        assert R in (2, 4, 8, 16) and B % R == 0, (nz, w, depth, coupling, B, R)
    assert {c[:4] for c in XG.FORMS} == {c[:4] for c in G.FORMS} and len(set(XG.SWAP)) == len(XG.SWAP)

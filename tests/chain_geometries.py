"""The geometry classes of the four fused chain steps (lsnf_mala_step, lsnf_reverse_mala_step, lsnf_hmc_step,
lsnf_reverse_langevin_step): one table for tests/test_gpu_mala.py, test_gpu_rmala.py, test_gpu_hmc.py and
test_gpu_reverse_langevin.py (not a test module; tests/test_chain_geometries_cpu.py holds the table to its classes).

The output sections of those kernels take row sums over the columns of a row, spread them over four waves of which only 2 HT own
a half-unit, draw noise four columns at a time and have to leave the draw of a padding column out of a sum: all of it depends on
where the half (nz / 2) and the width end inside the 32-column tiles of the instantiation <HT, WT> that csrc/lsnf_layout.h
lsnf_pick_tiles selects.  An entry is (nz, f_width, depth, coupling), tagged with that <HT, WT> and with what it stresses."""

TILE = 32                                    # csrc/lsnf_layout.h LSNF_TILE
DRAW = 4                                     # columns of one in-kernel Philox draw (csrc/lsnf_small3.h chain_xi: f0 .. f0 + 3)


def pick_tiles(half, width):
    """csrc/lsnf_layout.h lsnf_pick_tiles: the smallest of <1, 1>, <2, 2>, <2, 4> that covers (half, width)."""
    ht, wt = -(-half // TILE), -(-width // TILE)
    return (1, 1) if ht <= 1 and wt <= 1 else (2, 2) if ht <= 2 and wt <= 2 else (2, 4) if ht <= 2 and wt <= 4 else None


# (geometry, <HT, WT>, what it stresses)
TABLE = [
    ((62, 31, 2, 1), (1, 1), "one column short of a full tile in both dimensions; half 31: the scalar row access"),
    ((66, 33, 2, 1), (2, 2), "one column into the second tile in both dimensions; half 33"),
    ((124, 63, 3, 1), (2, 2), "ragged at the top end; half 62 = 2 mod 4: a draw straddles the end of the half"),
    ((66, 33, 3, 0), (2, 2), "ragged with additive coupling: the +40-bias packing on padded lanes"),
    ((10, 40, 2, 1), (2, 2), "the second half-tile entirely padding: waves 2 and 3 own half-units without a real column"),
    ((70, 8, 2, 1), (2, 2), "the second width tile entirely padding"),
    ((12, 100, 2, 1), (2, 4), "the second half-tile entirely padding, the width ragged"),
    ((66, 65, 2, 1), (2, 4), "one column into the third width tile; half 33"),
    ((128, 128, 2, 1), (2, 4), "no padding at all"),
]
GEOS = [geo for geo, _, _ in TABLE]
B_SMALL = 33                                 # two full 16-row workgroups and one row: the smallest batch with a partly live workgroup
CASES = [geo + (B_SMALL,) for geo in GEOS]
# the 32- and the 64-row workgroup forms at a ragged half and at an empty half-tile: single calls
LARGE = [(66, 33, 2, 1, 4100), (10, 40, 2, 1, 8200)]
# the call-form tests (in place, 4 bytes off, NULL optionals, the next proposal over the proposal)
FORMS = [geo + (B_SMALL,) for geo in ((66, 33, 2, 1), (124, 63, 3, 1), (10, 40, 2, 1), (12, 100, 2, 1))]


def half_of(geo):
    return geo[0] // 2


def draw_straddles(geo):
    """A four-column draw holds real columns and padding ones: the half is no multiple of DRAW."""
    return half_of(geo) % DRAW != 0


def second_half_tile_empty(geo):
    return pick_tiles(half_of(geo), geo[1])[0] == 2 and half_of(geo) <= TILE


def a_width_tile_empty(geo):
    return pick_tiles(half_of(geo), geo[1])[1] > -(-geo[1] // TILE)

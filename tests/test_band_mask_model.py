"""The slot rule of the band masks (tests/band_mask_model.py) on hand-worked primitives.  Snapped Y is 24.8 fixed point: pixel centre
row p sits at 256 p + 128, and the box of a primitive holds the centres with ymin <= 256 p + 128 <= ymax."""
import numpy as np

import band_mask_model as bm

H = 1216                          # 19 tile rows


def rows(ymin, ymax, h=H):
    py0, py1 = bm.centre_rows(np.array([ymin, ymax, (ymin + ymax) // 2]), h)
    return int(py0), int(py1)


def slots(ymin, ymax, h=H):
    return int(bm.slot_byte(*rows(ymin, ymax, h)))


def test_a_box_whose_last_centre_row_is_63_stays_in_tile_row_0():
    assert rows(60 * 256, 63 * 256 + 128) == (60, 63)        # the centre of row 63 lies on the box's edge: inside
    assert slots(60 * 256, 63 * 256 + 128) == 0b00000001
    assert rows(60 * 256, 63 * 256 + 127) == (60, 62)        # one step short of it
    assert rows(60 * 256, 64 * 256 + 128) == (60, 64)        # ... and the centre of row 64 is the next tile row's
    assert slots(60 * 256, 64 * 256 + 128) == 0b00000011


def test_a_box_whose_first_centre_row_is_64_starts_in_tile_row_1():
    assert rows(64 * 256 + 128, 70 * 256) == (64, 69)
    assert slots(64 * 256 + 128, 70 * 256) == 0b00000010
    assert rows(63 * 256 + 129, 70 * 256) == (64, 69)        # just below the centre of row 63
    assert rows(63 * 256 + 128, 70 * 256) == (63, 69)
    assert slots(63 * 256 + 128, 70 * 256) == 0b00000011


def test_spans_of_8_and_9_tile_rows_are_in_every_slot_and_7_rows_leave_one_out():
    y = lambda p: 256 * p + 128
    assert slots(y(3 * 64 + 5), y(9 * 64 + 7)) == 0b11111000 | 0b00000011      # rows 3 .. 9: seven of them, slot 2 stays empty
    assert slots(y(3 * 64 + 5), y(10 * 64)) == 0xFF                            # rows 3 .. 10: eight
    assert slots(y(3 * 64 + 63), y(11 * 64)) == 0xFF                           # rows 3 .. 11: nine
    assert slots(y(9 * 64), y(10 * 64 + 1)) == 0b00000110                      # rows 9, 10 fold onto slots 1, 2
    assert slots(y(15 * 64 + 1), y(16 * 64 + 1)) == 0b10000001                 # rows 15, 16: the fold wraps inside one primitive


def test_rows_are_clamped_at_0():
    assert rows(-5000, 300) == (0, 0)                        # (300 - 128) >> 8 = 0
    assert slots(-5000, 300) == 0b00000001
    assert rows(-5000, 127) == (0, -1)                       # no centre at all: no slot (the set-up pass never calls such a primitive alive)
    assert slots(-5000, 127) == 0
    assert slots(-70000, 64 * 256 + 128) == 0b00000011


def test_rows_are_clamped_at_the_last_row_of_a_target_that_ends_inside_a_tile_row():
    h = 200                                                  # rows 0 .. 199: tile row 3 is 8 rows high
    assert rows(190 * 256, 400 * 256, h) == (190, 199)
    assert slots(190 * 256, 400 * 256, h) == 0b00001100      # rows 2, 3 -- not rows 2 .. 6, which the unclamped box would reach
    assert slots(193 * 256, 400 * 256, h) == 0b00001000
    assert rows(199 * 256 + 129, 400 * 256, h) == (200, 199)
    assert slots(199 * 256 + 129, 400 * 256, h) == 0


def block(ys):
    """one block's 81 vertices with Y = ys[row] along each vertex row (X does not matter to the rule)"""
    xy = np.zeros((1, 81, 2), np.int32)
    xy[0, :, 1] = np.repeat(np.asarray(ys, np.int32), 9)
    return xy


def test_a_block_puts_each_alive_primitive_into_the_slots_of_its_rows():
    # vertex row j at the centre of pixel row 100 j: cell row lj spans pixel rows 100 lj .. 100 lj + 100, both triangle kinds alike
    xy = block([256 * 100 * j + 128 for j in range(9)])
    even, odd = np.uint64((1 << 0) | (1 << 9) | (1 << 63)), np.uint64((1 << 9) | (1 << 40))
    m = bm.band_masks(xy, np.array([even]), np.array([odd]), H)
    assert m.shape == (1, 8, 2)
    want = np.zeros((8, 2), np.uint64)
    for cell, kind in ((0, 0), (9, 0), (63, 0), (9, 1), (40, 1)):
        lj = cell >> 3
        for r in range((100 * lj) >> 6, ((100 * lj + 100) >> 6) + 1):
            want[r % 8, kind] |= np.uint64(1) << np.uint64(cell)
    assert np.array_equal(m[0], want)
    assert np.bitwise_or.reduce(m[0, :, 0]) == even and np.bitwise_or.reduce(m[0, :, 1]) == odd
    # cell row 7 covers pixel rows 700 .. 800 = tile rows 10 .. 12: they fold onto slots 2, 3, 4 -- where cell row 1 (rows 1 .. 3) is too
    assert int(m[0, 2, 0]) == (1 << 9) | (1 << 63) and int(m[0, 1, 0]) == (1 << 0) | (1 << 9)
    # tile rows reached: 0 .. 3 (cell rows 0, 1), 7 .. 9 (cell row 5), 10 .. 12 (cell row 7)
    assert bm.folded_slots(xy, np.array([even]), np.array([odd]), H)[0].tolist() == [2, 2, 2, 2, 1, 0, 0, 1]


def test_a_block_without_an_alive_primitive_has_empty_slots():
    xy = block([256 * 100 * j + 128 for j in range(9)])
    m = bm.band_masks(xy, np.zeros(1, np.uint64), np.zeros(1, np.uint64), H)
    assert not m.any()
    assert not bm.folded_slots(xy, np.zeros(1, np.uint64), np.zeros(1, np.uint64), H).any()

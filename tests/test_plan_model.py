"""The numpy model of the frame plan's cut rule (tests/plan_model.py) on hand-worked numbers, and the tables and poses the GPU tests
of the injected feedback use (tests/test_gpu_plan_feedback.py): on the CPU, that each reaches what it is named for."""
import numpy as np
import pytest

import plan_model as pm

NO_PIECES = np.zeros(64, np.uint32)


def test_quantum_is_seven_quarter_shares_of_the_sum_over_1024_items():
    assert pm.quantum([585143]) == 1000                      # 7 * 585143 = 4096001
    assert pm.quantum([585142]) == 999                       # 7 * 585142 = 4095994
    assert pm.quantum([292571, 292572]) == 1000              # the sum, not a tile
    assert pm.quantum([1]) == 1 and pm.quantum([585]) == 1 and pm.quantum([586]) == 1 and pm.quantum([1171]) == 2   # never below 1
    assert pm.quantum([0, 0, 0]) == 0 and pm.quantum([]) == 0
    assert pm.quantum(np.full(20, 0xFFFFFFFF, np.uint32)) == 7 * 20 * 0xFFFFFFFF // 4096     # a sum past 32 bits


@pytest.mark.parametrize("q", [1, 7, 1000, 146800639])
def test_every_threshold_at_q_and_one_below(q):
    for mult, lg in ((2, 1), (4, 2), (8, 3), (16, 4)):
        assert pm.strips_log2(mult * q, q) == lg
        assert pm.strips_log2(mult * q - 1, q) == lg - 1
    assert pm.strips_log2(0, q) == 0 and pm.strips_log2(q, q) == 0
    assert pm.strips_log2(16 * q, q, width=63) == 0 and pm.strips_log2(16 * q, q, width=44) == 0      # a narrow tile stays whole
    assert pm.strips_log2(16 * q, 0) == 0                                                             # no quantum, no cut


def test_a_piece_word_lifts_its_tile():
    pieces = NO_PIECES.copy()
    pieces[:5] = [10, 60, 5, 7, 9999]                        # recorded in 4 strips: the fifth word is not the tile's
    assert pm.tile_time(100, 2, pieces, as_one=False) == 240                 # 60 * 4 > 100
    assert pm.tile_time(100, 2, pieces, as_one=True) == 160                  # 240 * 4 // 6
    assert pm.tile_time(300, 2, pieces, as_one=False) == 300                 # the tile's own word is the heavier
    assert pm.tile_time(100, 3, pieces, as_one=False) == 9999 * 8            # recorded in 8: now it is
    assert pm.tile_time(100, 0, pieces, as_one=False) == 100                 # a whole tile has no pieces
    assert pm.tile_time(0, 2, pieces, as_one=False) == 0                     # no time stays no time
    assert pm.tile_time(0, 2, pieces, as_one=True) == 0


def test_the_lift_saturates_at_32_bits():
    pieces = NO_PIECES.copy()
    pieces[3] = 0x20000000                                   # << 4 = 2^33
    assert pm.tile_time(5, 4, pieces, as_one=False) == 0xFFFFFFFF
    assert pm.tile_time(5, 4, pieces, as_one=True) == 0xFFFFFFFF * 4 // 8 == 2147483647
    pieces[3] = 0x0FFFFFFF                                   # << 4 = 0xFFFFFFF0: just fits
    assert pm.tile_time(5, 4, pieces, as_one=False) == 0xFFFFFFF0
    pieces[0] = 0xFFFFFFFF
    assert pm.tile_time(5, 1, pieces, as_one=False) == 0xFFFFFFFF


def test_as_one_scaling_at_every_recorded_cut():
    assert [pm.tile_time(1000, lg, NO_PIECES, as_one=True) for lg in range(5)] == [1000, 800, 666, 571, 500]
    assert [pm.tile_time(1000, lg, NO_PIECES, as_one=False) for lg in range(5)] == [1000] * 5
    assert pm.tile_time(0xFFFFFFFF, 4, NO_PIECES, as_one=True) == 0xFFFFFFFF // 2         # (64-bit product)


GRID = dict(tx=np.tile(np.arange(5), 4), ty=np.repeat(np.arange(4), 5), W=300, ntx=5, nty=4)   # 300 x 200: the last column 44 px wide
ALL = np.ones(20, bool)


def test_an_all_zero_table_cuts_nothing():
    z = np.zeros(20, np.uint32)
    r = pm.request(z, np.full(20, 3), np.full((20, 64), 77, np.uint32), as_one=True, busy=ALL, **GRID)
    assert r["quantum"] == 0 and not r["lg"].any() and r["extra"] == 0 and not r["limited"] and not r["seen"].any()


def test_request_on_a_hand_worked_table():
    words = np.zeros(20, np.uint32)
    words[19] = 585143                                       # the narrow corner tile carries most of the sum
    words[0], words[1], words[6], words[4], words[15] = 2000, 1999, 20000, 50000, 100
    lgs, pieces = np.zeros(20, np.uint8), np.zeros((20, 64), np.uint32)
    lgs[1], pieces[1, 1] = 1, 4000                           # tile 1: max(1999, 4000 * 2) = 8000; as one: 8000 * 4 // 5 = 6400
    q = pm.quantum(words)
    assert q == 7 * (585143 + 2000 + 1999 + 20000 + 50000 + 100) // 4096 == 1126
    r = pm.request(words, lgs, pieces, as_one=True, busy=ALL, **GRID)
    assert r["quantum"] == q
    assert r["seen"][[0, 1, 6, 4]].tolist() == [2000, 6400, 20000, 50000]
    assert r["lg"][[0, 1, 6, 4]].tolist() == [0, 2, 4, 0]                                 # 1, 5, 17 quanta; the narrow tile whole
    assert r["seen"][2] == 50000 and r["lg"][2] == 4                                      # no time: the heaviest within two tiles (tile 4, two columns away)
    assert r["seen"][10] == 20000 and r["seen"][15] == 100                                # ... tile 6 for tile 10; a tile with a time keeps it
    s = pm.request(words, lgs, pieces, as_one=False, busy=ALL, **{**GRID, "ntx": 5, "nty": 4})
    assert s["seen"][[0, 1, 2, 6]].tolist() == [2000, 8000, 0, 20000] and s["lg"][[0, 1, 2, 6]].tolist() == [0, 2, 0, 4]     # shards: face value, no neighbours
    m = pm.request(words, lgs, pieces, as_one=True, busy=ALL, moving=True, **GRID)
    assert m["seen"][0] == 20000 and m["seen"][10] == 20000 and m["seen"][15] == 100      # 3 x 3 for a tile with a time (tile 15 does not reach tile 6), 5 x 5 for one without
    idle = ALL.copy(); idle[6] = False
    assert pm.request(words, lgs, pieces, as_one=True, busy=idle, **GRID)["lg"][6] == 0 # a background tile asks for nothing


def test_tile_2_of_the_hand_worked_table_sees_the_heavier_of_its_neighbours():
    words = np.zeros(20, np.uint32)
    words[19], words[4], words[6] = 585143, 50000, 20000
    r = pm.request(words, np.zeros(20, np.uint8), np.zeros((20, 64), np.uint32), as_one=True, busy=ALL, **GRID)
    assert r["seen"][2] == 50000                             # tile 4 (two columns away) is within reach and heavier than tile 6


def test_item_codes_must_name_every_part_once():
    code = lambda tile, part, lg: tile | part << 20 | lg << 24
    good = [code(3, 0, 0), code(5, 1, 1), code(5, 0, 1)] + [code(7, p, 4) for p in range(16)]
    cuts = pm.items_to_cuts(np.array(good, np.uint32), 9)
    assert cuts.tolist() == [-1, -1, -1, 0, -1, 1, -1, 4, -1]
    for bad in (good + [code(3, 0, 0)], good[:-1], good + [code(5, 0, 0)], good + [code(9, 0, 0)], good + [code(2, 0, 0) | 1 << 27], [code(1, 1, 0)]):
        with pytest.raises(AssertionError):
            pm.items_to_cuts(np.array(bad, np.uint32), 9)
    req = dict(lg=np.array([0, 0, 0, 0, 0, 1, 0, 4, 0]), limited=False)
    assert pm.check_against_request(cuts, req) == 16
    with pytest.raises(AssertionError):
        pm.check_against_request(cuts, dict(lg=np.array([0, 0, 0, 0, 0, 2, 0, 4, 0]), limited=False))      # cut coarser than a request that fits
    assert pm.check_against_request(cuts, dict(lg=np.array([0, 0, 0, 0, 0, 2, 0, 4, 0]), limited=True)) == 16
    with pytest.raises(AssertionError):
        pm.check_against_request(cuts, dict(lg=np.array([0, 0, 0, 0, 0, 0, 0, 4, 0]), limited=True))       # never finer than asked


# ---- the tables and poses of the GPU tests -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(5))
def test_uniform_tables_ask_every_full_width_tile_for_2_to_the_k(k):
    words = pm.uniform_cut_table(k, GRID["tx"], GRID["W"])
    r = pm.request(words, np.zeros(20, np.uint8), np.zeros((20, 64), np.uint32), as_one=True, busy=ALL, **GRID)
    full = GRID["tx"] < 4
    assert (r["lg"][full] == k).all() and not r["lg"][~full].any()
    assert (words[~full] > 16 * r["quantum"]).all()          # the narrow tiles stay whole though their times ask for 16 strips
    assert r["extra"] == 16 * ((1 << k) - 1) and not r["limited"]


def test_random_tables_reach_every_cut_every_special_word_and_an_overflowing_sum():
    cuts, sums = set(), []
    for seed in range(16):
        words, lgs, pieces = pm.random_table(seed, 20)
        assert words.dtype == np.uint32 and lgs.max() <= 4 and pieces.shape == (20, 64)
        assert (words == 0).any() and (pieces == 0xFFFFFFFF).any() and (pieces > words[:, None]).any()
        r = pm.request(words, lgs, pieces, as_one=True, busy=ALL, **GRID)
        cuts |= set(r["lg"][GRID["tx"] < 4].tolist())
        sums.append(int(words.astype(np.uint64).sum()))
        assert not r["limited"]                              # 20 tiles cannot exhaust the budget
    assert cuts == {0, 1, 2, 3, 4}
    assert max(sums) > 1 << 32 and min(sums) < 1 << 32       # some tables' sums pass 32 bits (words of 0xFFFFFFFF), some do not


def test_the_pose_sequence_moves_the_picture_as_the_plan_modes_need(oracle):
    W, H = 300, 200
    u = {name: oracle.look_at_uniforms(1, W, H, *pm.orbit_camera(a)) for name, a in pm.MODE_POSES.items()}
    shift = lambda a, b: pm.camera_shift_px(u[a], u[b], W, H)
    assert 24.0 < shift("rest", "fast") < 0.4 * W                        # the plan's moving mode, within the motion map's reach
    assert shift("fast", "jump") > 0.4 * W and shift("rest", "jump") > 0.4 * W     # a jump cut from either of the two frames before it
    assert 12.0 < shift("jump", "slow") < 24.0                           # weights spread, the plan does not wait
    assert shift("rest", "rest") == 0.0

"""A numpy model of the frame plan's cut rule, written from the rule as k_plan's comments state it (vulkan_forge_amd/csrc/vf_kernels.h),
for the tests that inject the tile times the plan reads (vf_terrain_debug_set_plan_feedback).

The rule.  Every local tile has a time word (10 ns ticks, summed over its strips), the log2 of the strips that time was recorded
with, and 64 piece words (the time of each strip).

  tile_time   a tile cut into strips is as heavy as its heaviest strip makes it: max(word, heaviest piece * strips), saturating at
              2^32 - 1; a zero word stays zero and a whole tile (lg 0) has no pieces.  An unsharded handle then brings the time back
              to "as one item": / (1 + lg / 4), i.e. * 4 // (4 + lg).  Shards keep the face value.
  quantum     max(1, 7 * sum(words) // 4096) of the RAW words of every tile of the state the plan reads; 0 when the sum is 0.
  seen        the tile's own tile_time; on an unsharded handle a tile without a time takes the heaviest tile_time within two tiles'
              distance, and with a moving camera (`moving`) every tile takes the heaviest of its 3 x 3 neighbourhood.  (The lookup
              through the camera motion is not modelled: its landing points are float arithmetic.)
  cut         lg = 4, 3, 2, 1 for seen // quantum >= 16, 8, 4, 2, else 0; no cut without a quantum or for a tile narrower than 64 px.
  budget      the cuts of a frame may add 2048 items; a tile that does not fit falls back to fewer strips.  Which tile loses depends
              on the order of the atomics: the model gives the REQUEST and the invariants (check_against_request), not the loser.
"""
import numpy as np

U32_MAX = 0xFFFFFFFF
TILE = 64
SPLIT_BUDGET = 2048           # extra work items a frame may create by splitting
TARGET_ITEMS = 1024           # the quantum is 7 quarter-shares of sum / TARGET_ITEMS
QUANTUM_X4 = 7


def tile_time(word, lg, pieces, as_one):
    """What the plan takes a tile to have cost.  word: its time; lg: log2 of the strips recorded with it; pieces: its piece words
    (at least 2^lg of them); as_one: an unsharded handle."""
    t, lg = int(word), int(lg)
    if t and lg:
        heaviest = max(int(p) for p in pieces[:1 << lg])
        t = max(t, min(heaviest << lg, U32_MAX))
    return t * 4 // (4 + lg) if as_one else t


def quantum(words):
    """The split quantum of a table of tile words (0: nothing is split)."""
    s = int(np.asarray(words, np.uint64).sum(dtype=np.uint64)) if len(words) else 0
    if s == 0:
        return 0
    q = max(1, QUANTUM_X4 * s // (4 * TARGET_ITEMS))
    assert q <= U32_MAX, "the quantum is a 32-bit word: tables whose 7 * sum / 4096 does not fit are outside the model"
    return q


def strips_log2(seen, q, width=TILE):
    """log2 of the strips the plan asks for a tile of `width` pixels whose time is `seen`, under the quantum q."""
    if q == 0 or width < TILE:
        return 0
    r = int(seen) // int(q)
    return 4 if r >= 16 else 3 if r >= 8 else 2 if r >= 4 else 1 if r >= 2 else 0


def tile_widths(tx, W):
    tx = np.asarray(tx, np.int64)
    return np.minimum(tx * TILE + TILE, W) - tx * TILE


def request(words, lgs, pieces, tx, ty, W, ntx, nty, as_one, busy, moving=False):
    """The cut the plan asks for.  Per local tile k: words[k], lgs[k], pieces[k] (64), its place (tx[k], ty[k]) in the ntx x nty tile
    grid of a frame W pixels wide; busy: the local tiles the frame draws.  Returns dict(quantum, seen (n,), lg (n,; 0 for tiles not
    busy), extra: the items the cuts add, limited: extra > SPLIT_BUDGET)."""
    n = len(words)
    q = quantum(words)
    times = [tile_time(words[k], lgs[k], pieces[k], as_one) for k in range(n)]
    width = tile_widths(tx, W)
    at = {}
    if as_one:                                               # (an unsharded handle's local tiles are the frame's, row-major)
        assert n == ntx * nty
        at = {(int(tx[k]), int(ty[k])): k for k in range(n)}
    seen, lg = np.zeros(n, np.uint64), np.zeros(n, np.int64)
    for k in np.flatnonzero(np.asarray(busy, bool)):
        s = times[k]
        if as_one and q and (s == 0 or moving):
            reach = 1 if s else 2
            for dy in range(-reach, reach + 1):
                for dx in range(-reach, reach + 1):
                    j = at.get((int(tx[k]) + dx, int(ty[k]) + dy))
                    if j is not None:
                        s = max(s, times[j])
        seen[k] = s
        lg[k] = strips_log2(s, q, int(width[k]))
    extra = int(((1 << lg) - 1)[np.asarray(busy, bool)].sum())
    return dict(quantum=q, seen=seen, lg=lg, extra=extra, limited=extra > SPLIT_BUDGET)


def items_to_cuts(codes, ntiles):
    """Item codes of a frame (tile | part << 20 | log2(parts) << 24; the depth-slice fields zero) -> per local tile the log2 of the
    strips it was drawn in, -1 for a tile without an item.  Every tile with an item must appear as exactly the parts 0 .. 2^lg - 1 of
    one lg: none missing, none repeated."""
    codes = np.asarray(codes, np.uint32)
    assert not (codes >> 27).any(), "depth-slice fields are not zero"
    tile, part, lg = (codes & 0xFFFFF).astype(np.int64), ((codes >> 20) & 15).astype(np.int64), ((codes >> 24) & 7).astype(np.int64)
    assert (tile < ntiles).all(), f"an item names tile {int(tile.max())} of {ntiles}"
    assert (lg <= 4).all(), "an item is cut into more than 16 strips"
    cuts = np.full(ntiles, -1, np.int64)
    order = np.lexsort((part, tile))
    tile, part, lg = tile[order], part[order], lg[order]
    first = np.flatnonzero(np.r_[True, tile[1:] != tile[:-1]])
    count = np.diff(np.r_[first, len(tile)])
    for f, c in zip(first, count):
        t, l = int(tile[f]), int(lg[f])
        assert (lg[f:f + c] == l).all(), f"tile {t}: items of different cuts {sorted(set(lg[f:f + c].tolist()))}"
        assert part[f:f + c].tolist() == list(range(1 << l)), f"tile {t} cut in {1 << l}: parts {part[f:f + c].tolist()}"
        cuts[t] = l
    return cuts


def check_against_request(cuts, req):
    """The invariants that hold whatever the order of the budget's atomics: no tile is cut finer than asked, the cuts add at most
    SPLIT_BUDGET items, and a request that fits the budget is granted exactly.  Returns the items the cuts added."""
    busy = cuts >= 0
    got = int(((1 << cuts[busy]) - 1).sum())
    assert got <= SPLIT_BUDGET, f"{got} extra items"
    over = np.flatnonzero(busy & (cuts > req["lg"]))
    assert len(over) == 0, f"tiles {over[:8].tolist()} are cut finer than the rule asks"
    if not req["limited"]:
        bad = np.flatnonzero(busy & (cuts != req["lg"]))
        assert len(bad) == 0, f"tiles {bad[:8].tolist()}: cut {cuts[bad[:8]].tolist()}, the rule asks {req['lg'][bad[:8]].tolist()}"
    return got


def camera_shift_px(ua, ub, W, H):
    """How far the terrain's footprint (the corners of the xz square of half-width 1.5 * spacing at y = 0) moves on the screen between two
    uniform blocks (view u[0:16], proj u[16:32], column-major): the larger of |dx|, |dy| over the corners, in pixels.  The frame plan
    picks its mode by this number (24 px: the plan waits for the previous frame; 12 px: weights spread to the neighbours)."""
    ext = 1.5 * max(float(ua[36]), 1e-8)
    worst = 0.0
    for cx in (-ext, ext):
        for cz in (-ext, ext):
            xy = []
            for u in (ua, ub):
                view = np.asarray(u[0:16], np.float64).reshape(4, 4).T
                proj = np.asarray(u[16:32], np.float64).reshape(4, 4).T
                q = proj @ (view @ np.array([cx, 0.0, cz, 1.0]))
                if not q[3] > 1e-6:
                    return 1e9
                xy.append((q[0] / q[3] * 0.5 * W, q[1] / q[3] * 0.5 * H))
            worst = max(worst, abs(xy[0][0] - xy[1][0]), abs(xy[0][1] - xy[1][1]))
    return worst


# ---- the poses and the tables of the GPU tests (tests/test_gpu_plan_feedback.py) ---------------------------------------------------------------

def orbit_camera(angle, radius=4.2, height=2.0):
    """look_at arguments of a camera on a circle around the terrain"""
    return ((radius * np.cos(angle), height, radius * np.sin(angle)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0)


# orbit angles for a 300 x 200 frame (tests/test_plan_model.py holds their screen shifts to what the names say): from `rest` to `fast`
# the picture moves by more than 24 px, to `jump` by more than 0.4 of the frame from either, from `jump` to `slow` by 12 .. 24 px
MODE_POSES = {"rest": 0.7, "fast": 1.0, "jump": 3.6, "slow": 3.75}


def uniform_cut_table(k, tx, W, q=1000):
    """Tile words that ask every full-width tile for 2^k strips: those tiles get (2^k + 1/2) q ticks, and the narrow tiles of the last
    column carry the rest of the sum that makes the quantum q (heavy, and never cut).  Recorded cuts 0, no piece words."""
    width = tile_widths(tx, W)
    full = width == TILE
    assert (~full).any(), "the table pads the sum with the narrow tiles of the last column"
    words = np.zeros(len(width), np.uint32)
    a = (1 << k) * q + q // 2
    words[full] = a
    total = -(-(q * 4 * TARGET_ITEMS) // QUANTUM_X4) + 64          # 7 * total // 4096 == q
    rest = total - a * int(full.sum())
    assert rest > 0
    words[~full] = rest // int((~full).sum())
    assert quantum(words) == q
    return words


def random_table(seed, n):
    """Seeded random feedback: tile words log-uniform over 1 .. 2^31 with a share of zeros and of 0xFFFFFFFF, recorded cuts 0 .. 4,
    piece words log-uniform with a share above their tile's word and of 0xFFFFFFFF."""
    rng = np.random.default_rng(9000 + seed)
    words = np.exp2(rng.uniform(0.0, 31.0, n)).astype(np.uint64)
    kind = rng.random(n)
    words[kind < 0.15] = 0
    words[kind > 0.93] = U32_MAX
    pick = rng.permutation(n)
    words[pick[0]] = 0                                       # every table has a tile without a time ...
    if seed % 4:
        words[pick[1]] = U32_MAX                             # ... three in four a saturated one (the sum then passes 32 bits) ...
    else:
        words[words == U32_MAX] = 1 << 20                    # ... and one in four none
    lgs = rng.integers(0, 5, n).astype(np.uint8)
    pieces = np.exp2(rng.uniform(0.0, 31.0, (n, 64))).astype(np.uint64)
    pk = rng.random((n, 64))
    pieces[pk < 0.1] = np.minimum(words[:, None] * 3 + 1, U32_MAX).repeat(64, axis=1)[pk < 0.1]     # above the tile's word
    pieces[pk > 0.97] = U32_MAX
    pieces[pk < 0.02] = 0
    return words.astype(np.uint32), lgs, pieces.astype(np.uint32)

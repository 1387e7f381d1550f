"""The slot rule of the per-tile-row alive masks ("band masks"), stated in numpy.

The set-up pass keeps, per block, BAND_SLOTS pairs of 64-bit masks beside the block record.  An alive primitive is set in slot s when
some absolute tile row r (64 pixel rows each) in [py0 >> 6, py1 >> 6] has r % BAND_SLOTS == s, where py0 .. py1 are the pixel-centre rows
inside the primitive's bounding box, clamped to the target:

    py0 = max((ymin + 127) >> 8, 0)        py1 = min((ymax - 128) >> 8, H - 1)         (24.8 snapped Y)

A primitive that spans BAND_SLOTS rows or more is therefore in every slot.  The inputs are what the library's read-out gives: per
block the 81 snapped vertices {X, Y} (9 x 9, row-major) and the record's alive_even / alive_odd.  Cell c = 8 lj + li has the corner
vertices a = 9 lj + li, b = a + 1, c = a + 9, d = a + 10; its even primitive is (a, c, b), its odd one (b, c, d)."""
import numpy as np

BAND_SLOTS = 8
TILE_ROWS = 64
BLOCK_VERTS = 9

_CELL = np.arange(64)
_A = (_CELL >> 3) * BLOCK_VERTS + (_CELL & 7)
EVEN_VERTS = np.stack([_A, _A + BLOCK_VERTS, _A + 1], axis=1)                       # (64, 3)
ODD_VERTS = np.stack([_A + 1, _A + BLOCK_VERTS, _A + BLOCK_VERTS + 1], axis=1)


def centre_rows(y, H):
    """y (..., 3): snapped Y of a primitive's vertices -> (py0, py1), the first and last pixel-centre row of its box on a target H high"""
    y = np.asarray(y, np.int64)
    ymin, ymax = y.min(axis=-1), y.max(axis=-1)
    return np.maximum((ymin + 127) >> 8, 0), np.minimum((ymax - 128) >> 8, H - 1)


def slot_byte(py0, py1):
    """bit s of the result: some tile row r in [py0 >> 6, py1 >> 6] has r % BAND_SLOTS == s (py0 > py1: no row, no bit)"""
    py0, py1 = np.asarray(py0, np.int64), np.asarray(py1, np.int64)
    r0, r1 = py0 >> 6, py1 >> 6
    out = np.zeros(np.broadcast(r0, r1).shape, np.uint8)
    for s in range(BAND_SLOTS):
        hit = (py0 <= py1) & (((s - r0) % BAND_SLOTS) <= (r1 - r0))    # the first row >= r0 that folds onto s lies (s - r0) mod SLOTS behind r0
        out |= (hit.astype(np.uint8) << s).astype(np.uint8)
    return out


def primitive_rows(xy, H):
    """xy (nblocks, 81, 2) int32 -> py0, py1 as (nblocks, 2, 64): [block, 0 even / 1 odd, cell]"""
    y = np.asarray(xy)[..., 1].astype(np.int64)
    e0, e1 = centre_rows(y[:, EVEN_VERTS], H)
    o0, o1 = centre_rows(y[:, ODD_VERTS], H)
    return np.stack([e0, o0], axis=1), np.stack([e1, o1], axis=1)


def mask_bits(m):
    """(n,) uint64 -> (n, 64) bool, bit c first"""
    m = np.asarray(m, np.uint64).reshape(-1, 1)
    return ((m >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def band_masks(xy, alive_even, alive_odd, H):
    """(nblocks, BAND_SLOTS, 2) uint64: [block, slot, 0 even / 1 odd] as the set-up pass writes them"""
    py0, py1 = primitive_rows(xy, H)
    alive = np.stack([mask_bits(alive_even), mask_bits(alive_odd)], axis=1)          # (nblocks, 2, 64)
    slots = slot_byte(py0, py1)
    weight = np.uint64(1) << np.arange(64, dtype=np.uint64)
    out = np.zeros((len(py0), BAND_SLOTS, 2), np.uint64)
    for s in range(BAND_SLOTS):
        inside = alive & (((slots >> s) & 1) != 0)
        out[:, s, :] = (inside * weight).sum(axis=2, dtype=np.uint64)
    return out


def folded_slots(xy, alive_even, alive_odd, H):
    """(nblocks, BAND_SLOTS) int: how many DIFFERENT tile rows the alive primitives of a block put into each slot (2 and more: the slot
    is shared by tile rows BAND_SLOTS apart -- the fold)"""
    py0, py1 = primitive_rows(xy, H)
    alive = np.stack([mask_bits(alive_even), mask_bits(alive_odd)], axis=1)
    r0, r1 = py0 >> 6, py1 >> 6
    nrows = (H + TILE_ROWS - 1) // TILE_ROWS
    out = np.zeros((len(py0), BAND_SLOTS), np.int64)
    for r in range(nrows):
        reached = (alive & (r0 <= r) & (r <= r1)).any(axis=(1, 2))
        out[:, r % BAND_SLOTS] += reached
    return out

"""Band masks: the set-up pass files a block's alive primitives per row of tiles, folded into eight slots, and the tile
kernel classifies the slot of its own tile row instead of the block's whole alive list.

Two referees.  For the MASKS the numpy statement of the slot rule (tests/band_mask_model.py), fed with the library's own read-out of
the snapped vertices and the records' alive masks: the slots must equal it bit for bit.  For the FRAMES the CPU oracle: the masks only
steer which primitives a tile looks at, so colour and visibility stay the oracle's -- EXACT colour 0 LSB, visibility bit for bit, the
FAST frame within RGBA_TOL -- with both line loops, 16 strips per tile, band and tile shards, a last tile row 8 pixels high, and a camera
inside the terrain (generic blocks, the complete tile kernel).

Shapes: 300 x 200 over grid 137 is 5 x 4 tiles with a partial tile in both directions and 17 x 17 blocks (two set-up segments per block
row, partial blocks last).  128 x 1216 over grid 17 is 19 tile rows over 2 x 2 blocks seen from above: a block covers some ten tile
rows, so tile rows eight apart share a slot -- the fold is real, and asserted.

Planted errors (each built once as a library outside the tree and run once against this file, neither kept):
  * the set-up pass files a primitive under the tile row of py0 alone (its last row taken for its first): all 15 tests fail --
    test_masks_equal_the_model on both shapes, and every frame test, because a primitive that crosses into the next tile row is
    missing there;
  * `slot = tile row % 4` in the tile kernel: the masks are right and test_masks_equal_the_model passes; the two
    test_whole_frames_with_both_line_loops[tall-*] cases fail (tile rows 4 and up read the slots of rows 0 .. 3); frames of four
    tile rows or fewer cannot tell, and pass."""
import numpy as np
import pytest

import band_mask_model as bm
import plan_model as pm
from conftest import DEFAULT_CAMERA, FILL_CAMERA, heightmap
from support import cabi  # noqa: F401
from test_gpu_parity import CLIP_CAM, EXACT, FAST, RGBA_TOL

pytestmark = pytest.mark.gpu

SLOPE = dict(W=300, H=200, G=137, cam=DEFAULT_CAMERA, exag=1.0, seed=3)
TALL = dict(W=128, H=1216, G=17, cam=FILL_CAMERA, exag=1.5, seed=4)
SHARDED = dict(W=200, H=320, G=65, cam=DEFAULT_CAMERA, exag=1.0, seed=5)
INSIDE = dict(W=320, H=240, G=32, cam=CLIP_CAM, exag=1.0, seed=6)
STALE = dict(W=320, H=256, G=64)
CAM_B = ((-2.4, 1.1, 2.9), (0.1, 0.0, -0.2), (0.0, 1.0, 0.0), 55.0, 0.1, 100.0)


def uniforms(oracle, W, H, cam, exag=1.0, sun=None):
    u = oracle.look_at_uniforms(1, W, H, *cam)
    u[38] = exag
    if sun is not None:
        u[32:35] = sun
    return u


_ORACLE = {}


def oracle_frame(oracle, luts, u, W, H, G, h):
    """(rgba, vis) of the whole frame, made once per input set"""
    key = (np.asarray(u, np.float32).tobytes(), W, H, G, h.tobytes())
    if key not in _ORACLE:
        _ORACLE[key] = oracle.render_terrain(u, W, H, G, h, luts["viridis"], nthreads=min(8, oracle.max_threads()))
    return _ORACLE[key]


def scene(oracle, luts, cabi, sc):
    """a handle on the scene's inputs, and the oracle's frame for them"""
    h = heightmap(sc["seed"], sc["G"])
    u = uniforms(oracle, sc["W"], sc["H"], sc["cam"], sc["exag"])
    t = cabi.Terrain(sc["W"], sc["H"], sc["G"], luts["viridis"])
    t.set_height(h); t.set_uniforms(u); t.set_shade_precision(EXACT)
    return t, oracle_frame(oracle, luts, u, sc["W"], sc["H"], sc["G"], h)


def hold_to_oracle(t, ref_rgba, ref_vis, what=""):
    """the handle's frame drawn EXACT (colour and stored visibility equal the oracle's) and FAST (within RGBA_TOL); leaves it EXACT"""
    t.set_shade_precision(EXACT)
    t.render()
    rgba = t.read_rgba()
    d = int(np.abs(rgba.astype(np.int16) - ref_rgba.astype(np.int16)).max(initial=0))
    assert d == 0, f"{what}: EXACT colour differs from the oracle by {d} LSB at {int((rgba != ref_rgba).any(axis=-1).sum())} pixels"
    if ref_vis is not None:
        bad = int((t.read_visibility() != ref_vis).sum())
        assert bad == 0, f"{what}: visibility differs at {bad} pixels"
    t.set_shade_precision(FAST)
    t.render()
    d = int(np.abs(t.read_rgba().astype(np.int16) - ref_rgba.astype(np.int16)).max(initial=0))
    t.set_shade_precision(EXACT)
    assert d <= RGBA_TOL, f"{what}: FAST colour differs from the oracle by {d} LSB"


# ---- 1. the masks ----------------------------------------------------------------------------------------------------------------------
def check_masks(r, H):
    """the read-out `r` against the model; returns the blocks the frame set up (count > 0)"""
    model = bm.band_masks(r["xy"], r["alive_even"], r["alive_odd"], H)
    drawn = r["count"] > 0
    assert drawn.any()
    pop = lambda m: bm.mask_bits(m).sum(axis=1)
    assert np.array_equal(r["count"], pop(r["alive_even"]) + pop(r["alive_odd"]))
    wrong = np.flatnonzero(drawn & (r["masks"] != model).any(axis=(1, 2)))
    assert len(wrong) == 0, f"band masks differ from the model in blocks {wrong[:8].tolist()} of {int(drawn.sum())}"
    union = np.bitwise_or.reduce(r["masks"], axis=1)
    assert np.array_equal(union[drawn, 0], r["alive_even"][drawn]) and np.array_equal(union[drawn, 1], r["alive_odd"][drawn])
    return drawn


@pytest.mark.parametrize("name", ["slope", "tall"])
def test_masks_equal_the_model(cabi, oracle, luts, name):
    sc = SLOPE if name == "slope" else TALL
    t, _ = scene(oracle, luts, cabi, sc)
    try:
        for frame in range(2):                               # the two plan states, one after the other
            t.render()
            r = t.band_masks()
            drawn = check_masks(r, sc["H"])
            alive = np.stack([r["alive_even"], r["alive_odd"]], axis=1)[:, None, :]
            filtered = (r["masks"] != alive).any(axis=(1, 2)) & drawn
            print(f"{name} frame {frame}: {int(drawn.sum())} blocks set up, {int(filtered.sum())} with a slot smaller than the alive list")
            assert filtered.any(), "no slot leaves a primitive out: the masks filter nothing here"
            if name == "tall":
                rows = (r["box"][:, 3] >> 6) - (r["box"][:, 1] >> 6) + 1
                folds = bm.folded_slots(r["xy"], r["alive_even"], r["alive_odd"], sc["H"])
                print("tall: tile rows per block", rows[drawn].tolist(), "tile rows per slot", folds[drawn].tolist())
                assert (rows[drawn] > bm.BAND_SLOTS).any(), "no block covers more than eight tile rows"
                assert (folds[drawn] >= 2).any(), "no slot is shared by two tile rows: the fold is not exercised"
    finally:
        t.close()


# ---- 2. the frames ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [0, 1])
@pytest.mark.parametrize("name", ["slope", "tall"])
def test_whole_frames_with_both_line_loops(cabi, oracle, luts, name, groups):
    sc = SLOPE if name == "slope" else TALL
    t, (ref_rgba, ref_vis) = scene(oracle, luts, cabi, sc)
    try:
        t.set_raster_groups(groups)
        hold_to_oracle(t, ref_rgba, ref_vis, f"{name}, line groups {groups}")
        assert t.raster_groups()[0] == groups
    finally:
        t.close()


@pytest.mark.parametrize("groups", [0, 1])
def test_sixteen_strips_per_tile(cabi, oracle, luts, groups):
    """every full-width tile cut into 4-pixel strips by injected tile times: 16 items per tile read the same slot"""
    sc = SLOPE
    t, (ref_rgba, ref_vis) = scene(oracle, luts, cabi, sc)
    try:
        ntx, nty = (sc["W"] + 63) // 64, (sc["H"] + 63) // 64
        tx = np.tile(np.arange(ntx), nty)
        t.set_raster_groups(groups)
        t.enable_timing(True)
        t.render(); t.render()                               # (an injection is refused on a handle's first two frames)
        t.set_plan_feedback(pm.uniform_cut_table(4, tx, sc["W"]))
        t.render()
        cuts = pm.items_to_cuts(t.item_stats()[:, 0], ntx * nty)
        full = pm.tile_widths(tx, sc["W"]) == 64
        assert (cuts[(cuts >= 0) & full] == 4).all() and ((cuts >= 0) & full).sum() >= 4
        rgba = t.read_rgba()
        assert np.array_equal(rgba, ref_rgba), "the frame cut into 16 strips per tile differs from the oracle"
        assert np.array_equal(t.read_visibility(), ref_vis)
    finally:
        t.close()


@pytest.mark.parametrize("name,nranks", [("sharded", 2), ("sharded", 3), ("slope", 2)])
def test_band_shards(cabi, oracle, luts, name, nranks):
    """row bands of 64: a rank's local tile rows are not the frame's; 300 x 200 ends in a band 8 rows high"""
    sc = SHARDED if name == "sharded" else SLOPE
    t, (ref_rgba, ref_vis) = scene(oracle, luts, cabi, sc)
    try:
        for rank in range(nranks):
            t.set_shard(rank, nranks, 64)
            rows = ((np.arange(sc["H"]) // 64) % nranks) == rank
            hold_to_oracle(t, ref_rgba[rows], ref_vis[rows], f"{name}: band shard {rank} of {nranks}")
    finally:
        t.close()


@pytest.mark.parametrize("skew", [0, 3])
def test_tile_shards(cabi, oracle, luts, skew):
    """interleaved tiles, tile-major storage: the slot comes from the tile map's row"""
    sc = SHARDED
    t, (ref_rgba, _) = scene(oracle, luts, cabi, sc)
    try:
        for rank in range(2):
            t.set_tile_shard(rank, 2, skew)
            lay = cabi.tile_layout(sc["W"], sc["H"], rank, 2, skew, lib=t.lib)
            for precision, tol in ((EXACT, 0), (FAST, RGBA_TOL)):
                t.set_shade_precision(precision)
                t.render()
                got = t.read_tiles()
                assert len(got) == len(lay) > 0
                for (tx, ty), tile in zip(lay, got):
                    want = ref_rgba[ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64]
                    d = int(np.abs(tile[:want.shape[0], :want.shape[1]].astype(np.int16) - want.astype(np.int16)).max(initial=0))
                    assert d <= tol, (skew, rank, int(tx), int(ty), precision, d)
    finally:
        t.close()


def test_a_camera_inside_the_terrain(cabi, oracle, luts):
    """near clipping: generic blocks keep the conservative box, their alive primitives follow the slot rule, and the items that met one
    are drawn again by the complete tile kernel -- which reads the same slots"""
    sc = INSIDE
    t, (ref_rgba, ref_vis) = scene(oracle, luts, cabi, sc)
    try:
        hold_to_oracle(t, ref_rgba, ref_vis, "camera inside the terrain")
        t.render()
        r = t.band_masks()
        generic = (r["flags"] & 1) != 0
        assert generic.any(), "no block with a generic primitive: the camera does not clip"
        assert (generic & (r["count"] > 0)).any(), "no generic block with alive primitives"
        bare = generic & (r["count"] == 0)                   # nothing alive, yet a box: a tile that pulls the block reads its slot
        assert not r["masks"][bare].any(), "a generic block without alive primitives has a mask bit set"
        check_masks(r, sc["H"])
    finally:
        t.close()


# ---- 3. staleness ----------------------------------------------------------------------------------------------------------------------
def test_masks_rewritten_every_frame_are_never_read_stale(cabi, oracle, luts):
    """Eight frames with the camera swapped and the heights uploaded again in front of each: both plan states' masks are rewritten with
    other content four times, read through the scalar cache in between.  Then the inputs rest for one frame (the other plan state pays
    its full pass once more), and two frames move the sun alone: both reuse the geometry, masks included.  Every frame is the oracle's."""
    W, H, G = STALE["W"], STALE["H"], STALE["G"]
    cams, hs = (DEFAULT_CAMERA, CAM_B), (heightmap(7, G), heightmap(8, G) * np.float32(1.3))
    t = cabi.Terrain(W, H, G, luts["viridis"])
    try:
        t.set_shade_precision(EXACT)

        def frame(k, u, h, what):
            t.render()
            ref_rgba, _ = oracle_frame(oracle, luts, u, W, H, G, h)
            rgba = t.read_rgba()
            d = int(np.abs(rgba.astype(np.int16) - ref_rgba.astype(np.int16)).max(initial=0))
            assert d == 0, f"frame {k} ({what}): colour differs from the oracle by {d} LSB at {int((rgba != ref_rgba).any(axis=-1).sum())} pixels"

        for k in range(8):
            u, h = uniforms(oracle, W, H, cams[k % 2]), hs[(k // 2) % 2]
            t.set_height(h); t.set_uniforms(u)
            frame(k, u, h, "camera swapped, heights uploaded")
            assert not t.geometry_reused()
        frame(8, u, h, "inputs at rest")
        for k, sun in ((9, (-0.3, 0.9, 0.2)), (10, (0.9, 0.2, -0.1))):
            us = uniforms(oracle, W, H, cams[1], sun=sun)
            t.set_uniforms(us)
            frame(k, us, h, "sun moved")
            assert t.geometry_reused(), f"frame {k}: moving the sun rebuilt the geometry"
        _, ref_vis = oracle_frame(oracle, luts, us, W, H, G, h)
        assert np.array_equal(t.read_visibility(), ref_vis)
    finally:
        t.close()

"""Parity tests proper: the HIP path (called through the C-ABI, include/vf_hip.h) against the CPU oracle on the
same seeded inputs, against the committed golden vectors, and -- at BASELINE.json's full sizes -- through
size-independent properties (determinism, shard-stitch == whole frame).

Bar: visibility (integer work) bit-exact; RGBA of the EXACT precision EQUAL to the oracle's (0 LSB: the arithmetic conventions are
fixed on both sides); RGBA of the FAST precision (the default) within 1 LSB per channel OF THE ORACLE (the tolerance north_star
states) -- both frames are held against the oracle directly, never one against the other."""
import hashlib
import math
import os

import numpy as np
import pytest

from conftest import DEFAULT_CAMERA, FILL_CAMERA, GOLDEN, heightmap
from support import cabi  # noqa: F401

pytestmark = pytest.mark.gpu

RGBA_TOL = 1   # LSB per channel (BASELINE.json north_star: "RGBA within +-1 LSB of reference")
EXACT, FAST = 0, 1   # vf_terrain_set_shade_precision: EXACT reproduces the oracle bit for bit (0 LSB), FAST (default) stays within RGBA_TOL
FAST_DIFF = np.zeros(4, np.int64)   # channel values of the FAST frames seen by hip_frame / compare_both: differing from the oracle by 0, 1, 2, >2 LSB


def note_fast(rgba_fast, ref_rgba):
    """The FAST frame against the ORACLE's: never more than RGBA_TOL apart."""
    d = np.abs(rgba_fast.astype(np.int16) - ref_rgba.astype(np.int16))
    FAST_DIFF[:] += np.bincount(np.minimum(d, 3).ravel(), minlength=4)
    assert int(d.max(initial=0)) <= RGBA_TOL, f"fast fragment path differs from the oracle by {int(d.max())} LSB"


class ExactFrame(np.ndarray):
    """The EXACT frame of hip_frame, carrying the FAST frame of the same handle: assert_parity holds both against the oracle."""
    fast = None


def hip_frame(cabi, u, W, H, G, height, lut, srgb=True, shard=None, shade_mode=0, frames=1):
    """One handle, `frames` frames of the default (FAST) precision -- the last of them planned with the feedback of the ones
    before -- then the same frame with the EXACT arithmetic: returns the EXACT frame (with the FAST one riding on it) and the
    visibility; the caller holds them against the oracle with assert_parity: EXACT equal, FAST within RGBA_TOL."""
    t = cabi.Terrain(W, H, G, lut, lut_is_srgb=srgb)
    try:
        t.set_uniforms(u)
        t.set_shade_mode(shade_mode)
        if height is not None:
            t.set_height(height)
        if shard:
            t.set_shard(*shard)
        for _ in range(frames):
            t.render()
        fast = t.read_rgba()
        vis_fast = t.read_visibility()
        assert np.array_equal(fast, t.read_rgba())      # read_visibility re-renders: the frame must not change
        t.set_shade_precision(EXACT)
        t.render()
        rgba = t.read_rgba()
        vis = t.read_visibility()
        assert np.array_equal(rgba, t.read_rgba())
        assert np.array_equal(vis, vis_fast)            # the precision switch never touches visibility
        rgba = rgba.view(ExactFrame)
        rgba.fast = fast
        return rgba, vis
    finally:
        t.close()


def compare_both(t, ref_rgba, ref_vis):
    """The handle's current frame set-up rendered FAST (as it is) and EXACT against the oracle; leaves the handle FAST."""
    t.render()
    fast = t.read_rgba()
    t.set_shade_precision(EXACT)
    try:
        t.render()
        rgba = t.read_rgba(); vis = t.read_visibility()
    finally:
        t.set_shade_precision(FAST)
    assert_parity(rgba, vis, ref_rgba, ref_vis)
    note_fast(fast, ref_rgba)
    return fast


def assert_parity(rgba, vis, ref_rgba, ref_vis):
    """EXACT frame against the oracle: identical visibility, identical RGBA (0 LSB); the FAST frame riding on a hip_frame result:
    within RGBA_TOL of the oracle."""
    assert vis.shape == ref_vis.shape and rgba.shape == ref_rgba.shape
    bad = int((vis != ref_vis).sum())
    assert bad == 0, f"visibility differs at {bad} pixels"
    d = np.abs(np.asarray(rgba).astype(np.int16) - ref_rgba.astype(np.int16)).max(initial=0)
    assert d == 0, f"EXACT RGBA differs from the oracle by {d} LSB"
    fast = getattr(rgba, "fast", None)
    if fast is not None:
        note_fast(fast, ref_rgba)
    return int(d)


# ---- SPEC_T32 fragment mode: HIP == oracle, bit for bit ------------------------------------------
@pytest.mark.parametrize("W,H,G,tex,cam", [(320, 240, 64, (64, 64), None), (200, 150, 40, (13, 61), None), (160, 120, 32, (1, 1), None),
                                           (256, 256, 128, (128, 128), "fill"), (1920, 1080, 1024, (1024, 1024), None)])
def test_spec_t32_mode_matches_the_oracle(cabi, oracle, luts, W, H, G, tex, cam):
    h = heightmap(G + tex[0], tex[0], tex[1])
    u = oracle.default_uniforms(1, W, H) if cam is None else oracle.look_at_uniforms(1, W, H, *FILL_CAMERA)
    u[38] = 1.7                                                         # exaggeration enters the forward differences
    rgba, vis = hip_frame(cabi, u, W, H, G, h, luts["terrain"], shade_mode=1)
    ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, luts["terrain"], shade_mode=oracle.SHADE_SPEC_T32, nthreads=8)
    assert_parity(rgba, vis, ref_rgba, ref_vis)
    plain, _ = oracle.render_terrain(u, W, H, G, h, luts["terrain"], nthreads=8)
    assert not np.array_equal(plain, ref_rgba)                           # and it is a different image from REFERENCE mode


# ---- committed golden vectors --------------------------------------------------------------------------
Z = np.load(os.path.join(GOLDEN, "frames_oracle.npz"))
GOLD = sorted({k.split("/")[0] for k in Z.files if k.endswith("/meta")})


@pytest.mark.parametrize("name", GOLD)
def test_golden_frames(cabi, oracle, luts, name):
    kind, W, H, G, srgb = (int(v) for v in Z[name + "/meta"])
    cmap = str(Z[name + "/cmap"])
    lut = luts[cmap] if srgb else oracle.lut_to_linear_u8(luts[cmap])
    rgba, vis = hip_frame(cabi, Z[name + "/uniforms"], W, H, G, Z[name + "/height"], lut, bool(srgb))
    assert assert_parity(rgba, vis, Z[name + "/rgba"], Z[name + "/vis"]) == 0


# ---- live parity on seeded inputs, incl. the edge cases ---------------------------------------------------
CLIP_CAM = ((0.2, 0.3, 0.4), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 70.0, 0.1, 100.0)       # camera inside the terrain: near clipping
LOW_CAM = ((0.5, 0.05, 0.5), (0.0, 0.2, 0.0), (0.0, 1.0, 0.0), 90.0, 0.05, 50.0)
CASES = [
    # id, kind, W, H, grid, texture (w,h) or None, camera, colormap, srgb
    ("c2_readme_demo", 0, 800, 600, 128, None, DEFAULT_CAMERA, "viridis", True),          # BASELINE config 2
    ("spike_tiny_grid2", 0, 64, 48, 2, None, None, "viridis", True),                      # two big triangles
    ("spike_grid8_big_tris", 0, 640, 480, 8, None, None, "magma", True),
    ("ragged_frame", 1, 250, 131, 37, (17, 9), None, "terrain", True),                    # W,H not multiples of 64 / 4
    ("one_pixel_rows", 1, 257, 1, 16, (8, 8), None, "viridis", True),
    ("odd_texture_255x3", 1, 320, 200, 64, (255, 3), None, "viridis", True),
    ("texture_larger_than_grid", 1, 200, 150, 16, (128, 96), None, "magma", True),
    ("texture_1x1_nonzero", 1, 160, 120, 24, (1, 1), None, "viridis", True),
    ("fill_camera", 1, 384, 384, 96, (96, 96), FILL_CAMERA, "terrain", True),
    ("near_clip_inside_terrain", 1, 320, 240, 32, (32, 32), CLIP_CAM, "viridis", True),
    ("low_grazing_camera", 0, 320, 240, 16, None, LOW_CAM, "viridis", True),
    ("unorm_lut_fallback", 0, 200, 160, 32, None, None, "terrain", False),
    ("noise_slivers_256", 1, 640, 360, 256, (256, 256), None, "viridis", True),
    ("grid_not_multiple_of_block", 1, 300, 300, 50, (50, 50), None, "magma", True),
    ("wide_frame", 0, 2048, 64, 40, None, None, "viridis", True),
    ("tall_frame", 0, 64, 1100, 40, None, None, "viridis", True),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_live_parity(cabi, oracle, luts, case):
    _, kind, W, H, G, tex, cam, cmap, srgb = case
    h = heightmap(hash(case[0]) % 1000, *tex) if tex else (oracle.SPIKE_DUMMY_HEIGHT if kind == 0 else oracle.SCENE_DUMMY_HEIGHT)
    u = oracle.default_uniforms(kind, W, H) if cam is None else oracle.look_at_uniforms(kind, W, H, *cam)
    lut = luts[cmap] if srgb else oracle.lut_to_linear_u8(luts[cmap])
    ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, lut, lut_is_srgb=srgb, nthreads=8)
    rgba, vis = hip_frame(cabi, u, W, H, G, h if tex or kind else None, lut, srgb)
    assert_parity(rgba, vis, ref_rgba, ref_vis)


@pytest.mark.parametrize("mod", ["exaggeration2", "spacing_half", "h_range_small", "exposure_high", "sun_low", "zero_guards"])
def test_uniform_lanes_drive_the_shader(cabi, oracle, luts, mod):
    """spacing / h_range / exaggeration / exposure / sun have no Python setter on TerrainSpike/Scene, but the UBO
    lanes are live in the shader (terrain.wgsl:46-47,71,83-85): drive them through vf_terrain_set_uniforms."""
    W, H, G = 240, 180, 48
    u = oracle.default_uniforms(1, W, H)
    h = heightmap(21, 48)
    if mod == "exaggeration2": u[38] = 2.0
    if mod == "spacing_half": u[36] = 0.5
    if mod == "h_range_small": u[37] = 0.2
    if mod == "exposure_high": u[35] = 3.5
    if mod == "sun_low": u[32:35] = [0.9, 0.05, -0.3]
    if mod == "zero_guards": u[36] = 0.0; u[37] = 0.0      # max(.,1e-8) guards
    ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, luts["viridis"])
    rgba, vis = hip_frame(cabi, u, W, H, G, h, luts["viridis"])
    assert_parity(rgba, vis, ref_rgba, ref_vis)


@pytest.mark.parametrize("seed", range(32))
def test_random_scenes_fuzz(cabi, oracle, luts, seed):
    """Seeded random frames: odd sizes, eyes above / inside / below / beside the terrain, narrow and wide fields of view,
    near and far planes that cut the terrain, exaggerated heights (slivers many tiles tall).  Bit-exact visibility, <= 1 LSB."""
    rng = np.random.default_rng(1000 + seed)
    W, H = int(rng.integers(1, 400)), int(rng.integers(1, 300))
    G = int(rng.choice([2, 3, 5, 9, 16, 17, 33, 64, 96]))
    tex = (int(rng.integers(1, 80)), int(rng.integers(1, 80)))
    h = (rng.random(tex, dtype=np.float32) - np.float32(0.5)) * np.float32(rng.choice([0.0, 0.2, 1.0, 3.0]))
    r = float(rng.choice([0.05, 0.6, 2.0, 4.5, 9.0]))
    th, ph = rng.uniform(0, 2 * math.pi), rng.uniform(-0.6, 1.4)
    eye = (r * math.cos(th) * math.cos(ph), r * math.sin(ph), r * math.sin(th) * math.cos(ph))
    target = tuple(float(v) for v in rng.uniform(-0.4, 0.4, 3))
    fovy = float(rng.choice([20.0, 45.0, 60.0, 120.0, 170.0]))
    znear = float(rng.choice([1e-3, 0.1, 0.5 * r]))
    zfar = float(rng.choice([r + 0.3, 100.0, 1e4]))                      # r + 0.3: the far plane cuts through the terrain
    u = oracle.look_at_uniforms(1, W, H, eye, target, (0.0, 1.0, 0.0), fovy, znear, zfar)
    u[38] = float(rng.choice([1.0, 1.0, 0.0, 8.0, -2.0]))              # exaggeration
    u[36] = float(rng.choice([1.0, 1.0, 0.3, 2.5]))                     # spacing
    cmap = str(rng.choice(["viridis", "magma", "terrain"]))
    ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, luts[cmap], nthreads=8)
    rgba, vis = hip_frame(cabi, u, W, H, G, h, luts[cmap], frames=4)      # the compared frames are planned with feedback (strips)
    assert_parity(rgba, vis, ref_rgba, ref_vis)


def test_non_finite_heights_do_not_hang_or_fault(cabi, oracle, luts):
    W, H, G = 160, 120, 32
    h = heightmap(3, 32)
    h[5, 7] = np.nan; h[20, 3] = np.inf; h[11, 11] = -np.inf
    u = oracle.default_uniforms(1, W, H)
    ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, luts["viridis"])
    rgba, vis = hip_frame(cabi, u, W, H, G, h, luts["viridis"])
    assert_parity(rgba, vis, ref_rgba, ref_vis)


# ---- BASELINE configs at full size -------------------------------------------------------------------------
def test_c3_scene_1080p_grid1024_full_parity(cabi, oracle, luts):
    W, H, G = 1920, 1080, 1024                                        # BASELINE config 3, SURVEY.md 8(d) C3
    h = heightmap(20250815, G)
    u = oracle.default_uniforms(1, W, H)
    ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, luts["viridis"], nthreads=min(16, oracle.max_threads()))
    rgba, vis = hip_frame(cabi, u, W, H, G, h, luts["viridis"])
    assert_parity(rgba, vis, ref_rgba, ref_vis)
    assert 0.05 < (vis > 0).mean() < 0.15


@pytest.fixture(scope="module")
def c4(cabi, oracle, luts):
    W = H = G = 4096                                                  # BASELINE config 4, SURVEY.md 8(d) C4
    h = heightmap(20250816, G)
    t = cabi.Terrain(W, H, G, luts["viridis"])
    t.set_height(h)
    yield t, h, W, H, G
    t.close()


@pytest.mark.parametrize("cam", [None, FILL_CAMERA], ids=["default_camera", "fill_camera"])
def test_c4_full_size_properties(c4, oracle, cam):
    t, h, W, H, G = c4
    u = oracle.default_uniforms(1, W, H) if cam is None else oracle.look_at_uniforms(1, W, H, *cam)
    t.set_shard(0, 1, 64)
    t.set_uniforms(u)
    t.render(); a = t.read_rgba()
    t.render(); b = t.read_rgba()
    assert a.shape == (H, W, 4)
    assert hashlib.sha256(a.tobytes()).hexdigest() == hashlib.sha256(b.tobytes()).hexdigest()     # idempotent / deterministic
    assert (a[..., 3] == 255).all()
    bg = (a == np.array([39, 39, 48, 255], np.uint8)).all(axis=2).mean()
    # analytic-surface coverage is 10.7 % / ~73 %; the +-0.25 noise heights widen the silhouette
    assert (0.70 < bg < 0.93) if cam is None else (0.10 < bg < 0.35), bg
    # screen-band shards rendered one after another on this GPU stitch to the whole frame, byte for byte
    for nranks, band in ((2, 64), (8, 64), (4, 256)):
        out = np.empty_like(a)
        for r in range(nranks):
            t.set_shard(r, nranks, band)
            t.render()
            loc = t.read_rgba()
            rows = np.flatnonzero(((np.arange(H) // band) % nranks) == r)
            assert loc.shape[0] == rows.size
            out[rows] = loc
        assert np.array_equal(out, a), (nranks, band)
    # interleaved-tile shards (the bench's N > 1 layout): every rank's tile-major slab, placed by vf_tile_layout
    from vulkan_forge_amd import cabi as _cabi
    # skew 0 (column stripes) is the bench's N > 1 layout: single tile columns for 8 ranks, stripes of 2 tiles for 4, of 4 tiles for 2
    # ... and load-balanced deals of the same stripes (round 5): the stripes' measured times -> vf_balance_stripes -> a registered map
    t.set_shard(0, 1, 64); t.render()
    col_ms = t.tile_times().reshape(H // 64, W // 64).sum(axis=0)
    maps = []
    for nranks, sl2 in ((2, 2), (4, 1), (8, 0)):
        stripe_ms = col_ms.reshape(-1, 1 << sl2).sum(axis=1)
        owner = _cabi.balance_stripes(stripe_ms, nranks, lib=t.lib)
        assert np.bincount(owner, minlength=nranks).tolist() == [len(owner) // nranks] * nranks
        loads = np.bincount(owner, weights=stripe_ms, minlength=nranks)
        naive = np.bincount(np.arange(len(owner)) % nranks, weights=stripe_ms, minlength=nranks)
        assert loads.max() <= naive.max() * 1.0001, (nranks, loads, naive)       # never worse than the round-robin deal on measured times
        maps.append((nranks, _cabi.register_stripe_map(owner, sl2, nranks, lib=t.lib)))
    for nranks, skew in [(2, 1), (8, 3), (3, 5), (2, 0), (4, 0), (8, 0), (2, 2 << 16), (4, 1 << 16), (3, (1 << 16) | 2)] + maps:
        out = np.zeros_like(a)
        for r in range(nranks):
            t.set_tile_shard(r, nranks, skew)
            t.render()
            tiles = t.read_tiles()
            lay = _cabi.tile_layout(W, H, r, nranks, skew, lib=t.lib)
            assert tiles.shape[0] == len(lay) == t.local_tiles()
            for k, (tx, ty) in enumerate(lay):
                out[ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64] = tiles[k]
        assert np.array_equal(out, a), (nranks, skew)
    t.set_shard(0, 1, 64)


def test_c4_rank_frames_while_the_plan_settles(c4, oracle, luts):
    """One rank of eight (column stripes) at C4: its few far-field tiles are cut into up to 16 strips -- and, in a library built with
    tools/experiments/r06_kernel_laboratory.patch + -DVF_SLICES=1, into depth slices (parts of the tile's descending block-row list, drawn by different workgroups and merged by
    atomic max).  Every frame on the way from the cold plan to the settled one (whole tiles, then strips by tile time, then strips
    ordered by their own times) equals the whole frame's tiles -- itself compared with the oracle in the next test."""
    from vulkan_forge_amd import cabi as _cabi
    t, h, W, H, G = c4
    u = oracle.default_uniforms(1, W, H)
    t.set_shard(0, 1, 64); t.set_uniforms(u); t.render()
    whole = t.read_rgba()
    sliced_items = cut_items = 0
    try:
        for r in (2, 5):
            t.set_tile_shard(r, 8, 0)
            lay = _cabi.tile_layout(W, H, r, 8, 0, lib=t.lib)
            t.enable_timing(True)
            for frame in range(7):
                t.render()
                tiles = t.read_tiles()
                codes = t.item_stats()[:, 0]
                sliced_items += int(((codes >> 29) & 3).astype(bool).sum())
                cut_items += int(((codes >> 24) & 7).astype(bool).sum())
                for k, (tx, ty) in enumerate(lay):
                    assert np.array_equal(tiles[k], whole[ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64]), (r, frame, tx, ty)
            t.enable_timing(False)
        assert cut_items > 0                                          # (sliced_items > 0 only with the depth slices patched back in)
    finally:
        t.enable_timing(False)
        t.set_shard(0, 1, 64)


def test_c4_default_camera_full_oracle_parity(c4, oracle, luts):
    t, h, W, H, G = c4
    u = oracle.default_uniforms(1, W, H)
    t.set_shard(0, 1, 64)
    t.set_uniforms(u)
    ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, luts["viridis"], nthreads=min(16, oracle.max_threads()))
    compare_both(t, ref_rgba, ref_vis)


def test_c4_one_shot_frame_is_planned(c4, cabi, oracle, luts):
    """The reference's usage is one-shot -- construct, render once (src/terrain/mod.rs:410-491).  A fresh handle has no tile times:
    its first frame is planned from the static estimate (k_plan_estimate), must already cut the heavy far-field tiles into strips,
    and must of course be the same picture (EXACT precision: the oracle's, byte for byte)."""
    _, h, W, H, G = c4
    u = oracle.default_uniforms(1, W, H)
    ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, luts["viridis"], nthreads=min(16, oracle.max_threads()))
    t = cabi.Terrain(W, H, G, luts["viridis"])
    try:
        t.set_height(h); t.set_uniforms(u); t.set_shade_precision(EXACT)
        t.enable_timing(True)
        t.render()                                                      # the ONE frame
        rgba = t.read_rgba()
        codes = t.item_stats()[:, 0]
        t.enable_timing(False)
        assert int(((codes >> 24) & 7).astype(bool).sum()) > 0, "the first frame was not cut into strips"
        assert np.array_equal(rgba, ref_rgba)
        assert np.array_equal(t.read_visibility(), ref_vis)
    finally:
        t.close()


def test_c4_fill_camera_full_oracle_parity(c4, oracle, luts):
    """The bench's other_camera (top-down, 73 % coverage) at full size against the oracle -- rendered a
    few times first so that the compared frame is planned with scheduling feedback, as the timed frames are."""
    t, h, W, H, G = c4
    u = oracle.look_at_uniforms(1, W, H, *FILL_CAMERA)
    t.set_shard(0, 1, 64)
    t.set_uniforms(u)
    for _ in range(4):
        t.render()
    ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, luts["viridis"], nthreads=min(16, oracle.max_threads()))
    compare_both(t, ref_rgba, ref_vis)


def test_fragment_stage_diagnostics_reproduce_the_frame(c4, oracle):
    """vf_terrain_debug_fragment_stage: the resolve-only launch (visibility -> RGBA8) must give the tile kernel's frame byte for
    byte, must not disturb the handle's output, and reports a time and the covered pixels (both C4 cameras)."""
    t, h, W, H, G = c4
    t.set_shard(0, 1, 64)
    for cam, lo, hi in ((None, 0.07, 0.30), (FILL_CAMERA, 0.65, 0.90)):
        u = oracle.default_uniforms(1, W, H) if cam is None else oracle.look_at_uniforms(1, W, H, *cam)
        t.set_uniforms(u)
        t.render(); a = t.read_rgba()
        ft = t.fragment_stage(repeats=3)
        assert ft["equal_to_frame"] == 1 and ft["repeats"] == 3 and ft["resolve_ms"] > 0.0
        assert lo < ft["covered_pixels"] / float(W * H) < hi, ft
        assert ft["covered_pixels"] >= int((a != np.array([39, 39, 48, 255], np.uint8)).any(axis=2).sum())   # (a covered pixel may shade to the clear colour, never the reverse)
        assert ft["covered_pixels"] == int((t.read_visibility() != 0).sum())
        assert np.array_equal(t.read_rgba(), a)                         # the caller's frame is untouched


def test_visibility_and_fragment_diagnostics_without_a_rendered_frame(cabi, oracle, luts):
    """vf_terrain_read_visibility / vf_terrain_debug_fragment_stage re-draw a frame into scratch buffers: the frame
    vf_terrain_render drew last, or -- before any render on this shard layout -- the CURRENT uniforms (never stale or
    uninitialised ones), any number of times in a row."""
    W, H, G = 300, 200, 48
    h = heightmap(31, G)
    u1 = oracle.default_uniforms(1, W, H)
    u2 = oracle.look_at_uniforms(1, W, H, (2.0, 2.5, -3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0, 0.1, 100.0)
    (_, v1), (_, v2) = (oracle.render_terrain(u, W, H, G, h, luts["viridis"]) for u in (u1, u2))
    assert not np.array_equal(v1, v2)
    t = cabi.Terrain(W, H, G, luts["viridis"])
    try:
        t.set_height(h); t.set_uniforms(u1)
        assert np.array_equal(t.read_visibility(), v1)
        assert np.array_equal(t.read_visibility(), v1)                   # twice, no vf_terrain_render in between
        t.set_uniforms(u2)
        assert np.array_equal(t.read_visibility(), v2)                   # still no frame: the current uniforms
        ft = t.fragment_stage(repeats=1)
        assert ft["equal_to_frame"] == 1 and ft["covered_pixels"] == int((v2 != 0).sum())
        with pytest.raises(cabi.VfError):
            t.read_rgba()                                                # the diagnostics did not count as a rendered frame
        t.render(); a = t.read_rgba()
        t.set_uniforms(u1)
        assert np.array_equal(t.read_visibility(), v2)                   # the frame drawn last, whatever was set since
        assert np.array_equal(t.read_rgba(), a)
        t.set_shard(0, 1, 64)                                            # new layout: that frame is forgotten
        assert np.array_equal(t.read_visibility(), v1)
    finally:
        t.close()


def test_feedback_scheduling_never_changes_the_frame(cabi, oracle, luts):
    """The frame plan is feedback-driven (last frame's per-tile time orders the work and cuts heavy tiles into column
    strips).  Jump between two unrelated cameras on one handle: every frame must equal the oracle's, whatever plan the
    previous camera left behind -- and the strip path must actually have been exercised."""
    W = H = 1536
    G = 1536
    h = heightmap(77, G)
    cams = [DEFAULT_CAMERA, ((0.3, 0.9, 2.6), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0, 0.1, 100.0)]
    us = [oracle.look_at_uniforms(1, W, H, *c) for c in cams]
    refs = [oracle.render_terrain(u, W, H, G, h, luts["viridis"], nthreads=min(16, oracle.max_threads())) for u in us]
    t = cabi.Terrain(W, H, G, luts["viridis"])
    try:
        t.set_height(h)
        t.set_shade_precision(EXACT)                                    # compared byte for byte with the oracle below
        t.enable_timing(True)
        strips_seen = 0
        for k in (0, 0, 0, 1, 0, 1, 1, 1, 0):
            t.set_uniforms(us[k]); t.render()
            rgba = t.read_rgba()
            strips_seen += int((t.item_stats()[:, 0] >> 24).astype(bool).sum())
            assert np.array_equal(rgba, refs[k][0]), k
        assert strips_seen > 0
        t.enable_timing(False)
        vis = t.read_visibility()
        assert np.array_equal(vis, refs[0][1])
    finally:
        t.close()


@pytest.mark.parametrize("plan_streams", [False, True])
def test_plan_queued_ahead_is_used_only_for_the_inputs_it_was_made_for(cabi, oracle, luts, plan_streams):
    """Round 5: a caller that waits for every frame of a camera at rest gets the NEXT frame's plan queued behind each frame
    (vf_hip.hip::render_impl).  Whatever changes between two frames -- camera, heights, exaggeration, shade mode, shard, timing -- the plan
    made ahead is for other inputs and must be thrown away: every frame below equals the oracle's.
    Round 6: a handle whose caller has always waited has no plan streams -- its plan made ahead goes out behind the next READ-BACK's
    copy, on the caller's stream (plan_streams False: every settle frame is read back); two frames in flight once make the streams."""
    W, H, G = 640, 400, 192
    h0, h1 = heightmap(41, G), heightmap(42, G)
    cams = [DEFAULT_CAMERA, ((2.5, 1.6, -2.8), (0.1, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0, 0.1, 100.0), FILL_CAMERA]
    t = cabi.Terrain(W, H, G, luts["viridis"])
    try:
        t.set_shade_precision(0)
        t.set_height(h0)
        if plan_streams:
            t.set_uniforms(oracle.look_at_uniforms(1, W, H, *cams[0]))
            t.render(); t.render(); t.sync()                     # a frame arriving while another is in flight: the handle takes the plan streams

        def settle_and_check(u, h, what, **kw):
            for _ in range(5):                                   # synchronous frames of one set of inputs: from the fourth on the plan comes from the call before
                t.render()
                if plan_streams: t.sync()
                else: t.read_rgba()                              # (the read-back is what sends a waiting caller's next plan on its way)
            ref, ref_vis = oracle.render_terrain(u, W, H, G, h, luts["viridis"], nthreads=8, **kw)
            assert np.array_equal(t.read_rgba(), ref), what
            return ref_vis

        u = oracle.look_at_uniforms(1, W, H, *cams[0]); t.set_uniforms(u)
        settle_and_check(u, h0, "at rest")
        u = oracle.look_at_uniforms(1, W, H, *cams[1]); t.set_uniforms(u)                # a plan for camera 0 is waiting: not this frame's
        t.render(); t.sync()
        ref, _ = oracle.render_terrain(u, W, H, G, h0, luts["viridis"], nthreads=8, want_vis=False)
        assert np.array_equal(t.read_rgba(), ref), "first frame of another camera"
        settle_and_check(u, h0, "other camera at rest")
        t.set_height(h1)                                           # other heights under a waiting plan
        vis = settle_and_check(u, h1, "other heights")
        assert np.array_equal(t.read_visibility(), vis)           # (a diagnostic re-render in between)
        u2 = u.copy(); u2[38] = np.float32(1.7); t.set_uniforms(u2)                     # exaggeration: same camera matrices, other geometry
        settle_and_check(u2, h1, "exaggeration")
        t.enable_timing(True); t.render(); t.sync(); assert t.timings()["frames"] >= 1; t.enable_timing(False)     # timing switched on over a waiting plan
        ref, _ = oracle.render_terrain(u2, W, H, G, h1, luts["viridis"], nthreads=8, want_vis=False)
        assert np.array_equal(t.read_rgba(), ref), "timed frame"
        t.set_shard(1, 2, 64)                                      # a shard under a waiting plan
        for _ in range(4):
            t.render(); t.sync()
        rows = np.flatnonzero(((np.arange(H) // 64) % 2) == 1)
        assert np.array_equal(t.read_rgba(), ref[rows]), "band shard"
        t.set_shard(0, 1, 64)
        u3 = oracle.look_at_uniforms(1, W, H, *cams[2]); t.set_uniforms(u3)
        settle_and_check(u3, h1, "top-down camera")
    finally:
        t.close()


@pytest.mark.parametrize("plan_streams", [True, False])
def test_a_plan_thrown_away_while_its_set_up_pass_still_runs(cabi, oracle, luts, plan_streams):
    """Round 6 (advisor): vf_terrain_render is asynchronous.  A caller that rests on one view (a plan for the next frame is queued
    behind every frame) and then calls render, set_uniforms, render WITHOUT a sync throws a plan away whose set-up pass -- on its own
    stream -- may still be writing the records the new plan's block boxes rewrite.  A large grid keeps that pass busy; the second
    view shows a corner only, so whole 16-block segments the stale pass works on are not needed (and never rewritten) in the new one."""
    W, H, G = 768, 768, 2048
    h = heightmap(47, G)
    corner = ((2.1, 0.9, 2.2), (1.25, -0.1, 1.2), (0.0, 1.0, 0.0), 18.0, 0.1, 100.0)
    t = cabi.Terrain(W, H, G, luts["magma"])
    try:
        t.set_shade_precision(0)
        t.set_height(h)
        ua, ub = oracle.look_at_uniforms(1, W, H, *DEFAULT_CAMERA), oracle.look_at_uniforms(1, W, H, *corner)
        refs = {k: oracle.render_terrain(u, W, H, G, h, luts["magma"], nthreads=8, want_vis=False)[0] for k, u in (("a", ua), ("b", ub))}
        if plan_streams:
            t.set_uniforms(ua)
            t.render(); t.render(); t.sync()                    # two frames in flight: the handle takes the context's plan streams
        for rnd in range(3):
            for first, second, want in ((ua, ub, "b"), (ub, ua, "a")):
                t.set_uniforms(first)
                for _ in range(5):
                    t.render()                                  # at rest: the last call queued the next frame's plan (plan streams) ...
                    if plan_streams: t.sync()
                    else: t.read_rgba()                         # ... or its read-back did, behind the copy (none: a waiting caller)
                t.render()                                      # takes that plan, queues another one behind this frame ...
                if not plan_streams: t.read_rgba()
                t.set_uniforms(second)
                t.render()                                      # ... which is not this frame's: dropped while it may still run
                t.sync()
                assert np.array_equal(t.read_rgba(), refs[want]), (rnd, want)
    finally:
        t.close()


def test_orbiting_camera_back_to_back(cabi, oracle, luts):
    """A camera that moves the picture by more than a tile per frame makes the plan wait for the previous frame's feedback
    instead of overlapping it (vf_hip.hip: kFreshFeedbackPx); slow motion keeps the overlap.  Frames are queued back to back
    without a read in between; the last one of each run must equal the oracle's."""
    import math
    W, H, G = 1280, 720, 512
    h = heightmap(5, G)
    t = cabi.Terrain(W, H, G, luts["viridis"])
    try:
        t.set_height(h)
        t.set_shade_precision(EXACT)
        for nposes, frames in ((48, 9), (720, 12)):                       # 7.5 degrees per frame, then 0.5
            eyes = [(4.2 * math.cos(2 * math.pi * k / nposes), 2.0, 4.2 * math.sin(2 * math.pi * k / nposes)) for k in range(frames)]
            us = [oracle.look_at_uniforms(1, W, H, e, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0) for e in eyes]
            for u in us:
                t.set_uniforms(u); t.render()
            rgba = t.read_rgba()
            ref_rgba, ref_vis = oracle.render_terrain(us[-1], W, H, G, h, luts["viridis"], nthreads=min(16, oracle.max_threads()))
            assert np.array_equal(rgba, ref_rgba), nposes
            assert np.array_equal(t.read_visibility(), ref_vis), nposes
    finally:
        t.close()


def test_maximum_grid_8192(cabi, oracle, luts):
    """Largest grid the C-ABI accepts (8192: 1024 x 1024 blocks, the limit of the tile kernel's 10-bit block indices):
    oracle parity at 2048 x 1536, and interleaved-tile shards that reassemble to the same frame."""
    W, H, G = 2048, 1536, 8192
    h = heightmap(1, G)
    u = oracle.default_uniforms(1, W, H)
    t = cabi.Terrain(W, H, G, luts["viridis"])
    try:
        t.set_height(h); t.set_uniforms(u)
        t.render(); fast = t.read_rgba()
        t.set_shade_precision(EXACT)
        t.render(); a = t.read_rgba()
        ref, _ = oracle.render_terrain(u, W, H, G, h, luts["viridis"], nthreads=min(16, oracle.max_threads()), want_vis=False)
        assert np.array_equal(a, ref)
        note_fast(fast, ref)
        out = np.zeros_like(a)
        for r in range(3):
            t.set_tile_shard(r, 3, 5); t.render()
            tiles = t.read_tiles()
            for k, (tx, ty) in enumerate(cabi.tile_layout(W, H, r, 3, 5, lib=t.lib)):
                out[ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64] = tiles[k]
        assert np.array_equal(out, a)
    finally:
        t.close()


def test_c5_pose_batch_subset(cabi, oracle, luts):
    """BASELINE config 5: 64 look-ats on the default camera's orbit over one terrain;
    8 of the 64 poses at a quarter-size frame against the oracle, one terrain object reused for all poses."""
    W, H, G = 480, 270, 256
    h = heightmap(20250817, G)
    t = cabi.Terrain(W, H, G, luts["viridis"])
    try:
        t.set_height(h)
        for k in range(0, 64, 8):
            th = 2 * math.pi * k / 64
            cam = ((3 * math.sqrt(2) * math.cos(th), 2.0, 3 * math.sqrt(2) * math.sin(th)), (0, 0, 0), (0, 1, 0), 45.0, 0.1, 100.0)
            u = oracle.look_at_uniforms(1, W, H, *cam)
            t.set_uniforms(u)
            ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, luts["viridis"], nthreads=8)
            compare_both(t, ref_rgba, ref_vis)
    finally:
        t.close()


# ---- height re-upload, borrowed device texture, stitch kernel ------------------------------------------------
def test_height_reupload_and_resize(cabi, oracle, luts):
    W, H, G = 200, 150, 40
    u = oracle.default_uniforms(1, W, H)
    t = cabi.Terrain(W, H, G, luts["magma"])
    try:
        t.set_uniforms(u)
        for shape in ((2, 2), (40, 40), (40, 40), (13, 61), (1, 1)):
            h = heightmap(sum(shape), shape[0], shape[1])
            t.set_height(h)
            ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, luts["magma"])
            compare_both(t, ref_rgba, ref_vis)
    finally:
        t.close()


@pytest.mark.parametrize("case", ["noise_640x360_g256", "fill_900x700_g384", "c3_1080p_g1024", "strips_rank_of_8"])
def test_both_line_loops_of_the_raster_draw_the_same_frame(cabi, oracle, luts, case):
    """The raster stage's line loop exists with and without the group pass (vf_terrain_set_raster_groups; left alone, a handle times both
    and keeps the faster per view).  Forced either way, and left to choose over enough frames to have probed both, a handle must
    give the same bytes -- FAST and EXACT, visibility included -- and the EXACT ones are the oracle's."""
    W, H, G, cam, shard = {"noise_640x360_g256": (640, 360, 256, DEFAULT_CAMERA, None), "fill_900x700_g384": (900, 700, 384, FILL_CAMERA, None),
                           "c3_1080p_g1024": (1920, 1080, 1024, DEFAULT_CAMERA, None), "strips_rank_of_8": (2048, 2048, 2048, DEFAULT_CAMERA, (3, 8))}[case]
    h = heightmap(len(case), G)
    u = oracle.look_at_uniforms(1, W, H, *cam)
    t = cabi.Terrain(W, H, G, luts["viridis"])
    try:
        t.set_height(h); t.set_uniforms(u)
        frames = {}
        for mode in (0, 1, -1):
            t.set_raster_groups(mode)
            if shard: t.set_tile_shard(shard[0], shard[1], 0)
            else: t.set_shard(0, 1, 64)
            for _ in range(20 if mode < 0 else 4):                  # (-1: past the probe window)
                t.render()
            fast = t.read_tiles() if shard else t.read_rgba()
            if mode >= 0:
                assert t.raster_groups()[0] == mode
            t.set_shade_precision(EXACT); t.render()
            exact = t.read_tiles() if shard else t.read_rgba()
            t.set_shade_precision(FAST)
            frames[mode] = (fast, exact)
        assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1], frames[1][1])
        assert np.array_equal(frames[-1][0], frames[0][0]) and np.array_equal(frames[-1][1], frames[0][1])
        if not shard:
            ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, luts["viridis"], nthreads=min(16, oracle.max_threads()))
            assert np.array_equal(frames[0][1], ref_rgba)
            note_fast(frames[0][0], ref_rgba)
            for mode in (0, 1):
                t.set_raster_groups(mode)
                assert np.array_equal(t.read_visibility(), ref_vis), mode
    finally:
        t.close()


def test_records_rewritten_every_frame_are_never_read_stale(cabi, oracle, luts):
    """k_tile reads a block's record through the SCALAR cache (constant-address-space load, vf_kernels.h "scalar-cache coherence")
    although k_block_setup wrote it with vector stores, on another stream, a frame earlier in the same buffer: that relies on the
    invalidate at the kernel boundary.  One handle, 20 frames, heights re-uploaded and the camera swapped before every one of them
    (both plan states are rewritten with different records again and again, nothing settles): every frame must be the oracle's."""
    W, H, G = 640, 360, 256
    cams = [DEFAULT_CAMERA, ((-2.4, 1.1, 2.9), (0.1, 0.0, -0.2), (0.0, 1.0, 0.0), 55.0, 0.1, 100.0)]
    us = [oracle.look_at_uniforms(1, W, H, *c) for c in cams]
    t = cabi.Terrain(W, H, G, luts["viridis"])
    try:
        for f in range(20):
            h = heightmap(900 + f % 5, G) * np.float32(1.0 + 0.5 * (f % 3))
            k = f & 1 if f < 12 else (f // 3) & 1                       # strictly alternating, then in runs: both plan-state parities see both cameras
            t.set_height(h); t.set_uniforms(us[k])
            ref_rgba, ref_vis = oracle.render_terrain(us[k], W, H, G, h, luts["viridis"], nthreads=8)
            t.set_shade_precision(FAST); t.render(); fast = t.read_rgba()
            note_fast(fast, ref_rgba)
            t.set_shade_precision(EXACT); t.render()
            assert np.array_equal(t.read_rgba(), ref_rgba), f
            if f % 5 == 4:
                assert np.array_equal(t.read_visibility(), ref_vis), f
    finally:
        t.close()


@pytest.mark.parametrize("seed", [3, 4, 5, 6])
def test_fast_precision_shards_equal_the_whole_frame(cabi, oracle, luts, seed):
    """The DEFAULT (FAST) fragment arithmetic must give the same bytes from every kernel instantiation and every cut of the frame:
    every fused multiply-add is written by hand under -ffp-contract=off, across the k_tile variants, strips and k_resolve(4).
    Random mid-size scenes, FAST throughout: whole frame (after feedback frames: strips) == 2..8 band shards == tile shards of
    several skews, each shard rendered three times so that its own plan has feedback; and the resolve-only launch equals the frame."""
    rng = np.random.default_rng(seed)
    W, H, G = int(rng.integers(500, 1300)), int(rng.integers(400, 900)), int(rng.choice([192, 256, 384, 512]))
    h = heightmap(seed, G)
    cam = (DEFAULT_CAMERA, FILL_CAMERA, ((0.4, 1.0, 2.7), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0, 0.1, 100.0))[seed % 3]
    u = oracle.look_at_uniforms(1, W, H, *cam)
    t = cabi.Terrain(W, H, G, luts["magma"])
    try:
        t.set_height(h); t.set_uniforms(u)
        t.enable_timing(True)
        for _ in range(4):
            t.render()
        whole = t.read_rgba()
        strips = int((t.item_stats()[:, 0] >> 24).astype(bool).sum())
        t.enable_timing(False)
        ft = t.fragment_stage(repeats=1)
        assert ft["equal_to_frame"] == 1
        ref_rgba, _ = oracle.render_terrain(u, W, H, G, h, luts["magma"], nthreads=8, want_vis=False)
        note_fast(whole, ref_rgba)
        for n, band in ((2, 64), (5, 64), (3, 128)):
            out = np.zeros_like(whole)
            for r in range(n):
                t.set_shard(r, n, band)
                for _ in range(3):
                    t.render()
                out[np.flatnonzero(((np.arange(H) // band) % n) == r)] = t.read_rgba()
            assert np.array_equal(out, whole), (n, band)
        ncols = (W + 63) // 64
        balanced2 = cabi.register_stripe_map(cabi.balance_stripes(rng.random(ncols // 2 * 2), 2)[:ncols // 2 * 2].tolist() + [0] * (ncols % 2), 0, 2)
        for n, skew in ((2, 0), (4, 0), (8, 0), (3, 5), (2, 2 << 16), (4, 1 << 16), (2, balanced2)):
            out = np.zeros_like(whole)
            for r in range(n):
                t.set_tile_shard(r, n, skew)
                for _ in range(3):
                    t.render()
                tiles = t.read_tiles()
                for k, (tx, ty) in enumerate(cabi.tile_layout(W, H, r, n, skew, lib=t.lib)):
                    hh, ww = min(64, H - ty * 64), min(64, W - tx * 64)
                    out[ty * 64:ty * 64 + hh, tx * 64:tx * 64 + ww] = tiles[k][:hh, :ww]
            assert np.array_equal(out, whole), (n, skew)
        assert strips >= 0
    finally:
        t.close()


_TORCH_INTEROP = r"""
import ctypes as C, os, sys
import numpy as np
import torch                      # first: the process then shares ONE HIP runtime (torch's) with libvf_hip.so
sys.path.insert(0, os.environ["VF_ROOT"])
import oracle
from vulkan_forge_amd import cabi
assert torch.cuda.is_available()
W, H, G, nr, band = 256, 512, 64, 4, 64
lut = np.load(os.path.join(os.environ["VF_ROOT"], "tests", "golden", "colormaps_rgba8.npz"))["viridis"]
u = oracle.default_uniforms(1, W, H)
h = np.random.default_rng(9).random((64, 64), dtype=np.float32) * np.float32(0.5) - np.float32(0.25)
d_h = torch.from_numpy(h).cuda()
gathered = torch.zeros((nr, H // nr, W, 4), dtype=torch.uint8, device="cuda")
t = cabi.Terrain(W, H, G, lut)
t.set_uniforms(u); t.set_shade_precision(0)                 # EXACT: compared byte for byte with the oracle
t.set_height_device(d_h.data_ptr(), 64, 64)                 # borrowed texture already in HBM
stream = torch.cuda.current_stream().cuda_stream
for r in range(nr):
    t.set_shard(r, nr, band)
    t.set_output_device(gathered[r].data_ptr())             # render straight into the caller's buffer
    t.render(stream)
t.sync()
image = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
rc = t.lib.vf_stitch_bands_device(t.ctx, C.c_void_p(gathered.data_ptr()), C.c_void_p(image.data_ptr()), W, H, nr, band, C.c_void_p(stream))
assert rc == 0
torch.cuda.synchronize()
ref, _ = oracle.render_terrain(u, W, H, G, h, lut)
assert np.array_equal(image.cpu().numpy(), ref)
t.close()
# tile shards on a frame whose edges cut tiles (200 x 150): slabs rendered into a caller-owned gather buffer + stitch kernel
W, H, G = 200, 150, 48
u = oracle.default_uniforms(1, W, H)
ref, _ = oracle.render_terrain(u, W, H, G, h, lut)
maps = [(2, cabi.register_stripe_map([1, 0, 0, 1], 0, 2)), (3, cabi.register_stripe_map([2, 0, 1, 1], 0, 3)), (2, cabi.register_stripe_map([1, 0], 1, 2))]   # registered stripe maps (owner per column stripe; 200 px = 4 tile columns)
for nr, skew in [(3, 5), (2, 1), (5, 3), (2, 1 << 16), (3, (1 << 16) | 1), (2, 2 << 16)] + maps:     # (stripes of 2 / 4 tiles: the layout word skew | stripe_log2 << 16)
    t = cabi.Terrain(W, H, G, lut)
    t.set_uniforms(u); t.set_height_device(d_h.data_ptr(), 64, 64); t.set_shade_precision(0)
    stride = max(len(cabi.tile_layout(W, H, r, nr, skew, lib=t.lib)) for r in range(nr)) + 1     # a stride larger than needed is fine
    gathered = torch.zeros((nr, stride * 4096), dtype=torch.int32, device="cuda")
    for r in range(nr):
        t.set_tile_shard(r, nr, skew)
        t.set_output_device(gathered[r].data_ptr())
        t.render(stream)
    image = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    t.stitch_tiles(gathered.data_ptr(), image.data_ptr(), nr, skew, stride, stream)
    torch.cuda.synchronize()
    assert np.array_equal(image.cpu().numpy(), ref), (nr, skew)
    try:
        t.read_rgba()
        raise SystemExit("read_rgba must refuse a tile-sharded handle")
    except cabi.VfError:
        pass
    t.close()
print("INTEROP_OK")
"""


def test_torch_device_buffers_streams_and_stitch_kernel():
    """Caller-owned HBM buffers (torch tensors), the caller's stream, virtual ranks and the de-interleave kernel.
    Runs in a child process that imports torch BEFORE the C-ABI library so both use one HIP runtime."""
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, VF_ROOT=ROOT)
    r = subprocess.run([sys.executable, "-c", _TORCH_INTEROP], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "INTEROP_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- grid_generate (bit-exact) and the triangle path --------------------------------------------------------
@pytest.mark.parametrize("nx,nz,sp", [(4, 3, (2.0, 1.0)), (2, 2, (1.0, 1.0)), (3, 3, (2.0, 2.0)), (256, 256, (1.0, 1.0)),
                                      (257, 129, (0.37, 1.9)), (1000, 7, (1e-3, 1e3)), (4096, 4096, (1.0, 1.0))])
def test_grid_generate_bit_exact(cabi, oracle, nx, nz, sp):
    import vulkan_forge as vf
    xy, uv, idx = vf.grid_generate(nx, nz, spacing=sp)
    oxy, ouv, oidx = oracle.grid_generate(nx, nz, sp)
    assert xy.dtype == np.float32 and uv.dtype == np.float32 and idx.dtype == np.uint32
    assert xy.shape == (nx * nz, 2) and uv.shape == (nx * nz, 2) and idx.shape == (6 * (nx - 1) * (nz - 1),)
    assert np.array_equal(xy.view(np.uint32), oxy.view(np.uint32))
    assert np.array_equal(uv.view(np.uint32), ouv.view(np.uint32))
    assert np.array_equal(idx, oidx)


@pytest.mark.parametrize("W,H", [(256, 256), (64, 64), (33, 21), (1, 1), (1920, 1080), (16, 16), (32, 24)])
def test_triangle_path(oracle, W, H):
    import vulkan_forge as vf
    a = vf.render_triangle_rgba(W, H)                                # BASELINE config 1 at (256, 256)
    assert a.shape == (H, W, 4) and a.dtype == np.uint8 and a.flags.c_contiguous
    assert np.array_equal(a, oracle.render_triangle(W, H))
    if (W, H) == (33, 21):
        assert np.array_equal(a, Z["triangle_33x21/rgba"])


def test_zz_fast_precision_histogram():
    """Runs last in this module: what the default (FAST) fragment path did across every frame the tests above rendered with both
    precisions -- never more than 1 LSB from the EXACT one (asserted per frame), and equal nearly everywhere."""
    total = int(FAST_DIFF.sum())
    assert total > 0
    print(f"\nFAST vs EXACT over {total} channel values: 0 LSB {FAST_DIFF[0]}, 1 LSB {FAST_DIFF[1]} ({100.0 * FAST_DIFF[1] / total:.4f} %), 2 LSB {FAST_DIFF[2]}, more {FAST_DIFF[3]}")
    assert FAST_DIFF[2] == 0 and FAST_DIFF[3] == 0
    assert FAST_DIFF[1] <= 0.01 * total

"""The mip-pyramid CPU model (tests/drape_mip_model) against what mipmapping must do: the pyramid equals an
independent numpy restatement bit for bit, a constant image gives the unmipped frame (and the oracle's) at any bias, a magnified
image gives the unmipped frame, the level of detail is the footprint on the surface, the bias shifts it, the nearest filter picks
the level stated, and the cases the GPU tests draw reach every branch of the sampler."""

import numpy as np
import pytest

import support  # noqa: F401  (the repository root and the model directories on sys.path)
import drape_mip_model as dmm
from test_drape_model import VIRIDIS, constant_lut, plain
from overlay_scenes import GRID, heights

drm = dmm.drm
import gbuffer_model as gbm

f32 = np.float32
PYRAMID_SIZES = [(37, 53), (1, 1), (2, 3), (5, 1), (211, 157), (16384, 2), (2, 16384)]


def numpy_pyramid(img):
    """the pyramid restated: float32 sums in the written order, times 1 / count, astype(float16) (round to nearest even)"""
    import oracle
    decode = oracle.srgb_tables()[0].astype(f32)
    a = img[..., 3].astype(f32) / f32(255.0)
    cur = np.concatenate([decode[img[..., :3]] * a[..., None], a[..., None]], axis=2).astype(f32)
    levels = [None]
    while cur.shape[:2] != (1, 1):
        h, w = cur.shape[:2]
        hk, wk = max(1, (h + 1) >> 1), max(1, (w + 1) >> 1)
        pad = np.zeros((2 * hk, 2 * wk, 4), f32)
        pad[:h, :w] = cur
        there = np.zeros((2 * hk, 2 * wk), bool)
        there[:h, :w] = True
        total = pad[0::2, 0::2].copy()                        # (2i, 2j) always exists
        count = np.ones((hk, wk), np.int64)
        for dy, dx in ((0, 1), (1, 0), (1, 1)):               # then (2i + 1, 2j), (2i, 2j + 1), (2i + 1, 2j + 1)
            m = there[dy::2, dx::2]
            total = np.where(m[..., None], total + pad[dy::2, dx::2], total).astype(f32)
            count += m
        assert set(np.unique(count).tolist()) <= {1, 2, 4}
        level = (total * (f32(1.0) / count.astype(f32))[..., None]).astype(f32).astype(np.float16)
        levels.append(level)
        cur = level.astype(f32)                               # the next level is formed from the stored values
    return levels


def test_the_binary16_conversion_is_round_to_nearest_even():
    L = dmm.lib()
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.random(4000, dtype=f32), rng.random(2000, dtype=f32) * f32(1e-4), rng.random(2000, dtype=f32) * f32(2e-7),
                           np.array([0.0, 1.0, 65504.0, 65519.9, 65520.0, 1e9, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -14, 0.999999, -0.3], f32)])
    # ties: halfway between two neighbouring binary16 values
    h = np.arange(0, 0x7BFF, 37, dtype=np.uint16)
    lo, hi = h.view(np.float16).astype(np.float64), (h + 1).astype(np.uint16).view(np.float16).astype(np.float64)
    vals = np.concatenate([vals, ((lo + hi) / 2).astype(f32)])
    with np.errstate(over="ignore"):
        want = vals.astype(np.float16).view(np.uint16)
    got = np.array([L.dmm_half_bits(float(v)) for v in vals], np.uint16)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    back = np.array([L.dmm_half_value(int(b)) for b in range(0, 0x7C01, 13)], f32)
    assert np.array_equal(back, np.arange(0, 0x7C01, 13, dtype=np.uint16).view(np.float16).astype(f32))


@pytest.mark.parametrize("size", PYRAMID_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_pyramid_equals_a_numpy_restatement(size):
    iw, ih = size
    img = drm.image(seed=iw * 7 + ih, size=size)
    got, want = dmm.pyramid(img), numpy_pyramid(img)
    sz = dmm.sizes(iw, ih)
    assert len(got) == len(want) == len(sz)
    assert len(sz) == {(37, 53): 7, (1, 1): 1, (16384, 2): 15, (2, 16384): 15, (2, 3): 3, (5, 1): 4, (211, 157): 9}[size]
    for k in range(1, len(sz)):
        w, h = sz[k]
        assert (w, h) == (max(1, (sz[k - 1][0] + 1) >> 1), max(1, (sz[k - 1][1] + 1) >> 1))
        assert got[k].shape == want[k].shape == (h, w, 4), k
        assert np.array_equal(got[k].view(np.uint16), want[k].view(np.uint16)), (k, int((got[k].view(np.uint16) != want[k].view(np.uint16)).sum()))
    assert sz[-1] == (1, 1)
    from vulkan_forge_amd._drape import mip_sizes
    assert mip_sizes(iw, ih) == sz


def test_the_level_count_at_the_size_limit():
    assert len(dmm.sizes(16384, 16384)) == 15 and len(dmm.sizes(37, 53)) == 7 and len(dmm.sizes(1, 1)) == 1
    assert sum(w * h for w, h in dmm.sizes(16384, 16384)[1:]) * 8 == 715827880          # the 716 MB of include/vf_hip.h


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cam", ["default", "near"])
def test_a_constant_image_gives_the_unmipped_frame_and_the_oracles(cam, mode):
    """premultiplied values 0 and 1 are exact in binary16, so every level holds the image's colour and every blend returns it"""
    W, H = 96, 64
    colour = (255, 0, 255)
    lut = constant_lut(colour)
    u, rgba, vis = plain(W, H, cam, lut, mode)
    u2, rgba2, vis2 = plain(W, H, cam, VIRIDIS, mode)
    for size in ((1, 1), (37, 53), (300, 7)):
        img = np.zeros((size[1], size[0], 4), np.uint8)
        img[:] = (*colour, 255)
        for filt in ("linear", "nearest"):
            flat, flat_again = drm.frame(rgba2, vis2, u2, heights(), GRID, VIRIDIS, img, extent=drm.EXTENT, filter=filt, shade_mode=mode)
            for bias in (-16.0, -1.0, 0.0, 1.5, 16.0):
                frame, again = dmm.frame(rgba, vis, u, heights(), GRID, lut, img, filter=filt, bias=bias, shade_mode=mode)
                assert np.array_equal(again, vis != 0) and np.array_equal(frame, rgba), (size, filt, bias)       # the oracle's frame
                frame, again = dmm.frame(rgba2, vis2, u2, heights(), GRID, VIRIDIS, img, extent=drm.EXTENT, filter=filt, bias=bias, shade_mode=mode)
                assert np.array_equal(again, flat_again) and np.array_equal(frame, flat), (size, filt, bias)     # the unmipped model's
    assert (vis != 0).mean() > 0.03


@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_a_magnified_image_gives_the_unmipped_frame(cam):
    W, H = 257, 131
    u, rgba, vis = plain(W, H, cam)
    img = drm.image()
    for filt in ("linear", "nearest"):
        flat, flat_again = drm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, extent=drm.EXTENT, filter=filt)
        frame, again, s = dmm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, extent=drm.EXTENT, filter=filt, bias=0.0, want_sample=True)
        mag = again & ~(s[..., 6] > 0)
        print(f"{cam} {filt}: {mag.sum()} of {again.sum()} rewritten pixels magnified")
        assert mag.sum() > 0.5 * again.sum()                  # 37 x 53 texels under 257 x 131 pixels: mostly magnified
        assert np.array_equal(frame[mag], flat[mag]) and np.array_equal(again[mag], flat_again[mag])
        assert np.array_equal(frame[~again], rgba[~again])
        frame, again = dmm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, extent=drm.EXTENT, filter=filt, bias=-16.0)
        assert np.array_equal(again, flat_again) and np.array_equal(frame, flat)


@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_the_footprint_is_the_surfaces(cam):
    """lod - bias against 0.5 log2(rho2) in binary64 from the geometry-buffer model's world positions of the pixel, its right and its
    lower neighbour, where the three carry the same visibility id: the piecewise-linear logarithm lies at most 0.0431 below, never
    above; the rest of [-0.06, +0.02] is binary32 rounding of positions and differences."""
    import oracle
    from support import uniforms
    W, H, grid = 257, 131, 24                                 # (a coarse grid: at the scenes' 1024 no primitive spans two pixels)
    u = uniforms(W, H, cam)
    assert u[36] == 1.0
    rgba, vis = oracle.render_terrain(u, W, H, grid, heights(), VIRIDIS, want_vis=True, nthreads=8, shade_mode=oracle.SHADE_REFERENCE)
    rgba = rgba.reshape(H, W, 4)
    iw, ih = dmm.CASE_SIZE
    ext = np.array(dmm.CASE_EXTENT[cam], f32)
    bias = 0.75
    _, again, s = dmm.frame(rgba, vis, u, heights(), grid, VIRIDIS, dmm.case_image(), extent=ext, bias=bias, want_sample=True)
    _, pos, _ = gbm.planes(vis, u, heights(), grid)
    x, z = pos[..., 0].astype(np.float64) / float(u[36]), pos[..., 2].astype(np.float64) / float(u[36])
    same = np.zeros((H, W), bool)
    same[:-1, :-1] = (vis[:-1, :-1] == vis[:-1, 1:]) & (vis[:-1, :-1] == vis[1:, :-1])
    pick = same & again & np.isfinite(s[..., 6])
    assert pick.sum() > 0.3 * again.sum()
    sx, sz = float(f32(iw) / (ext[2] - ext[0])), float(f32(ih) / (ext[3] - ext[1]))
    ax = ((x[:-1, 1:] - x[:-1, :-1]) * sx) ** 2 + ((z[:-1, 1:] - z[:-1, :-1]) * sz) ** 2
    ay = ((x[1:, :-1] - x[:-1, :-1]) * sx) ** 2 + ((z[1:, :-1] - z[:-1, :-1]) * sz) ** 2
    want = np.full((H, W), np.nan)
    with np.errstate(divide="ignore"):
        want[:-1, :-1] = 0.5 * np.log2(np.maximum(ax, ay))
    d = (s[..., 6].astype(np.float64) - bias)[pick] - want[pick]
    print(f"{cam}: lod - 0.5 log2(rho2) in [{d.min():+.4f}, {d.max():+.4f}] over {pick.sum()} pixels")
    assert d.min() >= -0.06 and d.max() <= 0.02


def shares(s, again, levels):
    lod = s[..., 6][again]
    n = len(lod)
    top = float(levels - 1)
    ends = ((~(lod > 0)) | (lod >= top)).sum() / n
    between = (lod > 0) & (lod < top)
    t = lod[between] - np.floor(lod[between])
    blends = (t > 0).sum() / n
    fl, cnt = np.unique(np.floor(lod[between]), return_counts=True)
    return ends, blends, {int(k): c / n for k, c in zip(fl, cnt)}


@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_the_gpu_tests_case_reaches_the_code(cam):
    W, H = 257, 131
    u, rgba, vis = plain(W, H, cam)
    img = dmm.case_image()
    assert img.shape == (769, 1021, 4) and (img[..., 3] == 0).any() and (img[..., 3] == 255).any() and ((img[..., 3] > 0) & (img[..., 3] < 255)).any()
    levels = len(dmm.sizes(*dmm.CASE_SIZE))
    frame, again, s = dmm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, extent=dmm.CASE_EXTENT[cam], bias=0.0, want_sample=True)
    ends, blends, floors = shares(s, again, levels)
    print(f"{cam}: {again.sum()} rewritten; lod <= 0 or top {ends:.3f}; 0 < t < 1 {blends:.3f}; floor(lod) shares {floors}")
    assert again.sum() > 0.1 * (vis != 0).sum()
    assert ends >= 0.05
    assert sum(1 for v in floors.values() if v >= 0.02) >= 3
    assert blends >= 0.25
    flat, _ = drm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, extent=dmm.CASE_EXTENT[cam])
    assert (frame != flat).any()                              # mipmapping shows
    cut = dmm.clipped_pixels(vis, u, heights(), GRID)
    print(f"{cam}: {cut} covered pixels show a primitive cut by the near or far plane")
    assert (cut > 0) == (cam == "near")                       # the `near` camera is the one through the clipper


def test_bias_moves_the_level_of_detail():
    W, H = 257, 131
    u, rgba, vis = plain(W, H, "default")
    img = dmm.case_image()
    kw = dict(extent=dmm.CASE_EXTENT["default"], want_sample=True)
    _, again0, s0 = dmm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, bias=0.0, **kw)
    for bias in (1.5, -1.0):
        _, again, s = dmm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, bias=bias, **kw)
        both = again & again0 & np.isfinite(s0[..., 6])
        assert both.sum() > 0.5 * again0.sum()
        assert np.array_equal(s[..., 6][both], s0[..., 6][both] + f32(bias))      # (multiples of 2^-24 below 16: the sum is exact)


def test_the_nearest_filter_picks_the_level_stated():
    """an image whose level k is the constant k / 16 names the level a sample came from: impossible with real means, so the model's
    sampler is given such a pyramid through its own cache"""
    W, H = 257, 131
    u, rgba, vis = plain(W, H, "default")
    iw, ih = 64, 64
    img = np.zeros((ih, iw, 4), np.uint8)
    img[..., 3] = 255
    buf, sz = dmm._flat(img)
    saved = buf.copy()
    try:
        o = 0
        for k, (w, h) in enumerate(sz[1:], 1):
            buf[o:o + 4 * w * h] = np.float16(k / 16.0).view(np.uint16)
            o += 4 * w * h
        ext = (-1.4, -1.4, -0.2, 0.1)                          # 64 texels over a part of the grid: minified at this frame size
        _, again, s = dmm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, extent=ext, filter="nearest", bias=2.0, want_sample=True)
        lod = s[..., 6][again]
        want = np.where(lod + f32(0.5) >= len(sz) - 1, len(sz) - 1, np.floor(np.maximum(lod, 0) + f32(0.5))).astype(np.int64)
        want[~(lod > 0)] = 0
        got = s[..., 0][again]
        expect = np.where(want == 0, f32(0.0), (want / 16.0).astype(f32))
        assert np.array_equal(got, expect)
        assert len(set(want.tolist())) >= 3
    finally:
        buf[:] = saved

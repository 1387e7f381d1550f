"""The draped-image CPU model (tests/drape_model) against what a drape must do: an image of the colormap's own colour
gives the oracle's frame bit for bit, a transparent one writes nothing, the nearest filter takes the texel the geometry-buffer
position falls in, filtering is premultiplied, the fragment arithmetic with shadows and ambient occlusion equals a numpy restatement,
and the scenes the GPU tests draw are partly draped."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
import support
import drape_model as drm
import gbuffer_model as gbm
from overlay_scenes import GRID, heights

abm, shm = drm.abm, drm.shm
f32 = np.float32
VIRIDIS = np.load(os.path.join(HERE, "golden", "colormaps_rgba8.npz"))["viridis"]


_plain = {}


def plain(W, H, cam, lut=VIRIDIS, mode=0, h=None, sun=None):
    """the oracle's exact frame and its visibility, computed once per case"""
    import oracle
    key = (W, H, cam, lut.tobytes(), mode, None if h is None else h.tobytes(), None if sun is None else tuple(sun))
    if key not in _plain:
        u = support.uniforms(W, H, cam, sun=sun)
        rgba, vis = oracle.render_terrain(u, W, H, GRID, heights() if h is None else h, lut, want_vis=True, nthreads=8,
                                          shade_mode=oracle.SHADE_SPEC_T32 if mode else oracle.SHADE_REFERENCE)
        _plain[key] = (u, rgba.reshape(H, W, 4), vis)
    return _plain[key]


def constant_lut(colour):
    lut = np.zeros((256, 4), np.uint8)
    lut[:] = (*colour, 255)
    return lut.reshape(1024)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cam", ["default", "near"])
def test_an_image_of_the_colormaps_colour_gives_the_oracles_frame(cam, mode):
    W, H = 96, 64
    colour = (200, 90, 33)
    lut = constant_lut(colour)
    u, rgba, vis = plain(W, H, cam, lut, mode)
    for size, filt in (((1, 1), "linear"), ((4, 2), "linear"), ((4, 2), "nearest")):
        img = np.zeros((size[1], size[0], 4), np.uint8)
        img[:] = (*colour, 255)
        frame, again = drm.frame(rgba, vis, u, heights(), GRID, lut, img, filter=filt, shade_mode=mode)
        assert np.array_equal(again, vis != 0), (size, filt, int((again != (vis != 0)).sum()))
        assert np.array_equal(frame, rgba), (size, filt, int((frame != rgba).any(axis=2).sum()))
    assert (vis != 0).mean() > 0.03


def test_a_transparent_image_or_opacity_zero_writes_nothing():
    W, H = 96, 64
    u, rgba, vis = plain(W, H, "default")
    clear = drm.image()
    clear[..., 3] = 0
    for img, opacity in ((clear, 1.0), (drm.image(), 0.0)):
        for filt in ("linear", "nearest"):
            frame, again = drm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, extent=drm.EXTENT, opacity=opacity, filter=filt)
            assert not again.any() and np.array_equal(frame, rgba)
    _, again = drm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, drm.image(), extent=drm.EXTENT)
    assert again.any()


def test_the_nearest_filter_takes_the_texel_the_position_falls_in():
    import oracle
    W, H = 257, 131
    iw, ih = 37, 53
    ext = np.array((-0.7, -0.5, 0.9, 0.8), f32)               # its edges lie inside the frame of the top-down camera
    u, rgba, vis = plain(W, H, "fill")
    assert u[36] == 1.0                                       # (spacing 1: the geometry buffers' position is (x, h exag, z) itself)
    iy, ix = np.meshgrid(np.arange(ih), np.arange(iw), indexing="ij")
    img = np.stack([ix, iy, (ix * 7 + iy * 3) % 256, np.full_like(ix, 255)], axis=2).astype(np.uint8)   # every texel distinct, opaque
    frame, again, sample = drm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, extent=ext, filter="nearest", want_sample=True)
    _, pos, _ = gbm.planes(vis, u, heights(), GRID)
    x, z = pos[..., 0], pos[..., 2]
    sx, sz = f32(iw) / (ext[2] - ext[0]), f32(ih) / (ext[3] - ext[1])
    fu, fv = (x - ext[0]) * sx, (z - ext[1]) * sz
    inside = (vis != 0) & (fu >= 0) & (fu <= f32(iw)) & (fv >= 0) & (fv <= f32(ih))
    assert np.array_equal(again, inside)
    cx = np.minimum(np.floor(fu[inside]).astype(np.int64), iw - 1)
    cy = np.minimum(np.floor(fv[inside]).astype(np.int64), ih - 1)
    decode = oracle.srgb_tables()[0]
    assert len(np.unique(decode)) == 256                      # (a sample names its texel)
    got = sample[inside]
    assert np.array_equal(got[:, 0], decode[cx]) and np.array_equal(got[:, 1], decode[cy]) and (got[:, 3] == 1.0).all()
    assert np.array_equal(got[:, 2], decode[(cx * 7 + cy * 3) % 256])
    # every row and column is met, the first and the last ones too, and the frame shows the extent's edges
    assert set(cx.tolist()) == set(range(iw)) and set(cy.tolist()) == set(range(ih))
    covered = vis != 0
    assert (covered & ~inside & (fu < 0)).any() and (covered & ~inside & (fu > iw)).any()
    assert (covered & ~inside & (fv < 0)).any() and (covered & ~inside & (fv > ih)).any()
    assert np.array_equal(frame[~again], rgba[~again]) and (frame[again] != rgba[again]).any()


@pytest.mark.parametrize("spacing", [2.0, 0.25])
def test_the_extent_is_in_grid_coordinates_whatever_the_spacing(spacing):
    """The twin of the test above at a spacing that is not 1 (a power of two: position.x / spacing is exact) and exaggeration -2.
    include/vf_hip.h: the extent is in the plane in which the grid's vertices lie at -1.5 ... 1.5 and is not multiplied by the
    spacing, unlike overlay coordinates -- the texel is the one that position / spacing falls in."""
    import oracle
    W, H = 257, 131
    iw, ih = 7, 5
    ext = np.array((-0.7, -0.5, 0.9, 0.8), f32)
    h = heights()
    # the top-down camera on its own line of sight, further out with the terrain's width and lifted over the exaggerated relief
    k = spacing + 1.0
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, (0.0, 2.2 * k, 0.01 * k), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 0.1, 100.0), f32).reshape(44)
    u[36], u[38] = spacing, -2.0
    rgba, vis = oracle.render_terrain(u, W, H, GRID, h, VIRIDIS, want_vis=True, nthreads=8, shade_mode=oracle.SHADE_REFERENCE)
    rgba = rgba.reshape(H, W, 4)
    iy, ix = np.meshgrid(np.arange(ih), np.arange(iw), indexing="ij")
    img = np.stack([ix, iy, (ix * 7 + iy * 3) % 256, np.full_like(ix, 255)], axis=2).astype(np.uint8)
    frame, again, sample = drm.frame(rgba, vis, u, h, GRID, VIRIDIS, img, extent=ext, filter="nearest", want_sample=True)
    _, pos, _ = gbm.planes(vis, u, h, GRID)
    x, z = pos[..., 0] / f32(spacing), pos[..., 2] / f32(spacing)              # exact: back in the grid's plane
    sx, sz = f32(iw) / (ext[2] - ext[0]), f32(ih) / (ext[3] - ext[1])
    fu, fv = (x - ext[0]) * sx, (z - ext[1]) * sz
    inside = (vis != 0) & (fu >= 0) & (fu <= f32(iw)) & (fv >= 0) & (fv <= f32(ih))
    assert np.array_equal(again, inside)
    cx = np.minimum(np.floor(fu[inside]).astype(np.int64), iw - 1)
    cy = np.minimum(np.floor(fv[inside]).astype(np.int64), ih - 1)
    decode = oracle.srgb_tables()[0]
    got = sample[inside]
    assert np.array_equal(got[:, 0], decode[cx]) and np.array_equal(got[:, 1], decode[cy]) and (got[:, 3] == 1.0).all()
    assert set(cx.tolist()) == set(range(iw)) and set(cy.tolist()) == set(range(ih))
    # the frame shows the extent's four edges; read in the spaced world, the same box would lie elsewhere
    covered = vis != 0
    assert (covered & ~inside & (fu < 0)).any() and (covered & ~inside & (fu > iw)).any()
    assert (covered & ~inside & (fv < 0)).any() and (covered & ~inside & (fv > ih)).any()
    wu, wv = (pos[..., 0] - ext[0]) * sx, (pos[..., 2] - ext[1]) * sz
    spaced = covered & (wu >= 0) & (wu <= f32(iw)) & (wv >= 0) & (wv <= f32(ih))
    assert (spaced != inside).sum() > 0.2 * inside.sum()
    assert np.array_equal(frame[~again], rgba[~again]) and (frame[again] != rgba[again]).any()


def test_filtering_is_premultiplied():
    W, H = 96, 64
    u, rgba, vis = plain(W, H, "fill")
    img = np.array([[(255, 0, 0, 255), (0, 255, 0, 0)]], np.uint8)            # opaque red beside transparent green
    frame, again, sample = drm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, filter="linear", want_sample=True)
    s = sample[again]
    assert again.any() and (s[:, 1] == 0).all() and (s[:, 2] == 0).all()      # no green bleeds into the blend
    mixed = (s[:, 3] > 0) & (s[:, 3] < 1)
    assert mixed.any() and np.array_equal(s[:, 0], s[:, 3])                   # red is its own coverage: decode[255] = 1


def fma(a, b, c):
    """fmaf through binary64: the product is exact there; the sum rounds twice only in a double-rounding case (2^-29 per operation)"""
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(f32)


def restate(u, attr, lit, amb, val, opacity, lut):
    """fs_main + the sRGB store of DESIGN.md 4 (reference shade mode) with lambert * lit, shade * amb and the mixed albedo, in numpy
    binary32: abm_frame's arithmetic with the albedo replaced"""
    import oracle
    one, zero = f32(1.0), f32(0.0)
    h, x, z = attr
    decode = oracle.srgb_tables()[0]
    h_range = max(u[37], f32(1e-8))
    t = f32(0.5) + h / (f32(2.0) * h_range)
    t = np.minimum(np.maximum(t, zero), one)
    c = t * f32(256.0) - f32(0.5)
    i0f = np.floor(c)
    f = c - i0f
    i0 = np.clip(i0f.astype(np.int64), 0, 255)
    i1 = np.clip(i0f.astype(np.int64) + 1, 0, 255)
    _, cosx = oracle.sincos(x * f32(1.3))
    sinz, _ = oracle.sincos(z * f32(1.1))
    dhdx = f32(1.3) * cosx * f32(0.25)
    dhdz = f32(-1.1) * sinz * f32(0.25)
    d = fma(dhdz, dhdz, fma(dhdx, dhdx, one))
    inv = one / np.sqrt(d)
    nx, ny, nz = -dhdx * inv, inv, -dhdz * inv
    sx, sy, sz = u[32], u[33], u[34]
    linv = one / np.sqrt(fma(sz, sz, fma(sy, sy, sx * sx)))
    Lx, Ly, Lz = sx * linv, sy * linv, sz * linv
    ndl = fma(nz, Lz, fma(ny, Ly, nx * Lx))
    lambert = np.minimum(np.maximum(ndl, zero), one) * lit
    shade = (f32(0.15) * (one - lambert) + lambert) * amb
    Aop = val[:, 3] * f32(opacity)
    out = np.empty((len(h), 4), np.uint8)
    out[:, 3] = 255
    lin = decode[np.asarray(lut, np.uint8).reshape(256, 4)[:, :3]]
    for ch in range(3):
        l0, l1 = lin[i0, ch], lin[i1, ch]
        lc = fma(f, l1 - l0, l0)
        alb = fma(f32(opacity), val[:, ch], (one - Aop) * lc)
        out[:, ch] = oracle.srgb_encode(alb * u[35] * shade)
    return out


@pytest.mark.parametrize("cam", ["default", "fill"])
def test_with_shadows_and_ambient_occlusion(cam):
    W, H = 96, 64
    h = abm.scene_heights()
    sun = shm.sun_vector(*abm.SCENE_SUN_DEG)
    u, rgba, vis = plain(W, H, cam, h=h, sun=sun)
    sky = abm.field(u, h, GRID, abm.scene_directions(), abm.SCENE_PARAMS["reach"])
    lit = shm.field(u, h, GRID, **abm.SCENE_SHADOWS)
    strength = abm.SCENE_PARAMS["strength"]
    # 1. lit and amb are the ambient model's: under an opaque image of one colour at opacity 1 the albedo is that colour whatever
    #    the colormap, and the frame is the ambient model's frame of a colormap of that colour
    colour = (180, 140, 60)
    img = np.zeros((3, 5, 4), np.uint8)
    img[:] = (*colour, 255)
    flat = constant_lut(colour)
    _, flat_rgba, flat_vis = plain(W, H, cam, flat, h=h, sun=sun)
    assert np.array_equal(flat_vis, vis)
    for use_lit, use_sky in ((True, True), (True, False), (False, True)):
        want, _ = abm.frame(flat_rgba, vis, u, h, GRID, flat, sky if use_sky else np.ones_like(sky), strength, lit=lit if use_lit else None)
        got, again = drm.frame(rgba, vis, u, h, GRID, VIRIDIS, img, lit=lit if use_lit else None, sky=sky if use_sky else None, strength=strength)
        assert np.array_equal(again, vis != 0) and np.array_equal(got, want), (use_lit, use_sky)
        assert (want != flat_rgba).any()
    # 2. the fragment arithmetic with the tests' image, restated in numpy for a sample of the rewritten pixels
    _, pos, _ = gbm.planes(vis, u, h, GRID)
    assert u[36] == 1.0 and u[38] == 1.0                      # (position = (x, h, z))
    for opacity, filt in ((1.0, "linear"), (0.37, "nearest")):
        frame, again, sample = drm.frame(rgba, vis, u, h, GRID, VIRIDIS, drm.image(), extent=drm.SCENE_EXTENT[cam], opacity=opacity, filter=filt,
                                         lit=lit, sky=sky, strength=strength, want_sample=True)
        pick = np.argwhere(again)[::2]
        assert len(pick) > 100
        py, px = pick[:, 0], pick[:, 1]
        s = sample[py, px]
        assert (s[:, 4] < 1).any() and (s[:, 5] < 1).any() and (s[:, 4] <= 1).all() and (s[:, 5] <= 1).all()
        p = pos[py, px]
        want = restate(u, (p[:, 1], p[:, 0], p[:, 2]), s[:, 4], s[:, 5], s[:, :4], opacity, VIRIDIS)
        assert np.array_equal(frame[py, px], want), int((frame[py, px] != want).any(axis=1).sum())
        assert np.array_equal(frame[~again], rgba[~again])


@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_the_gpu_tests_scenes_are_partly_draped(cam):
    W, H = 257, 131
    u, rgba, vis = plain(W, H, cam)
    covered = int((vis != 0).sum())
    for filt in ("linear", "nearest"):
        frame, again = drm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, drm.image(), extent=drm.SCENE_EXTENT[cam], filter=filt)
        frac = again.sum() / covered
        assert covered > 0 and 0.1 <= frac <= 0.9, (cam, filt, frac)
        assert not again[vis == 0].any() and np.array_equal(frame[~again], rgba[~again]) and (frame[again] != rgba[again]).any()
    assert drm.image().shape == (53, 37, 4) and drm.EXTENT == (-1.1, -0.9, 1.3, 1.6)
    img = drm.image()
    iy, ix = np.meshgrid(np.arange(53), np.arange(37), indexing="ij")
    hole = (ix // 6 + iy // 6) % 3 == 0
    assert (img[hole, 3] == 0).all() and (img[~hole, 3] >= 1).all()

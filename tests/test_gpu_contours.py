"""Contour layers extracted on the GPU equal the CPU model (tests/contour_model) drawn by the occlusion model's
composite, bit for bit and with no pixel left out: cameras, joins, widths, translucent colours, occlusion, lift, layer order, a NaN
texel, vertices and plateaus exactly on a level, grids 100 and 257; the counts and the height bounds equal the model's; the layer is
a snapshot that follows the exaggeration; over-budget requests and sharded handles are refused with nothing changed."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import contour_model as cm
from overlay_scenes import CAMERAS, GRID, heights, scene
from support import vf  # noqa: F401

ocm = cm.ocm


def oracle_vis(u, W, H, h, grid):
    import oracle
    return oracle.render_terrain(u, W, H, grid, h, np.zeros(1024, np.uint8), want_vis=True, nthreads=8)[1]


def model_frame(base, u, h, grid, L):
    """the model's frame: the layers over `base`; the oracle's visibility only where a record occludes"""
    H, W = base.shape[:2]
    occluding = bool((L.array()["flags"] & ocm.OCCLUDE).any())
    vis = oracle_vis(u, W, H, h, grid) if occluding else np.zeros((H, W), np.uint32)
    return ocm.composite(base, vis, u, h, grid, L)


def same(got, want):
    diff = (got != want).any(axis=2)
    assert not diff.any(), f"{int(diff.sum())} pixels differ from the model, first at {np.argwhere(diff)[:4].tolist()}"


def add_contours(s, L, h, grid, u, levels, **kw):
    """the same contour layer on the scene and on the model's layers -> layer id"""
    lid = s.add_contours(np.asarray(levels, np.float32), **kw)
    L.contours(h, grid, u, levels, **kw)
    assert s.layer_primitive_count(lid) == len(L.recs[-1]) == L.nsegments * (2 if kw.get("join", "round") == "round" else 1)
    return lid


LEVELS = np.arange(-0.6, 0.9, 0.1).astype(np.float32)


@pytest.mark.parametrize("cam,size", [("default", (1920, 1080)), ("default", (1280, 720)), ("fill", (1280, 720)), ("near", (1280, 720))])
def test_frames_equal_the_model(vf, cam, size):
    """a point layer, contours (round, 1 px, opaque), contours (no joins, 5 px, translucent, occluding, lifted), a polygon layer,
    contours (round, 5 px, translucent): every kind of contour layer, in layer order between other layers"""
    W, H = size
    h = heights()
    s = scene(vf, W, H, h, cam)
    base = s.render_rgba()
    u = s.debug_uniforms_f32()
    rng = np.random.default_rng(5)
    pts = np.column_stack([rng.uniform(-1.5, 1.5, 500), np.full(500, 0.02), rng.uniform(-1.5, 1.5, 500)]).astype(np.float32)
    poly = [np.array([[-0.8, 0.05, -0.7], [0.9, 0.05, -0.5], [0.2, 0.05, 0.9]], np.float32)]
    L = cm.Layers()
    s.add_points(pts, size_px=9.0, rgba=(255, 40, 40, 200), drape=True, occlude=True)
    L.points(pts, size_px=9.0, rgba=(255, 40, 40, 200), drape=True, occlude=True)
    add_contours(s, L, h, GRID, u, LEVELS[::3], width_px=1.0, rgba=(0, 0, 0, 255))
    add_contours(s, L, h, GRID, u, LEVELS[1::3], width_px=5.0, rgba=(255, 255, 0, 120), lift=0.02, join="none", occlude=True, depth_bias=0.02)
    s.add_polygons(poly, fill_rgba=(0, 90, 255, 140), line_rgba=(255, 255, 255, 255), line_width_px=2.0, drape=True)
    L.polygons(poly, fill_rgba=(0, 90, 255, 140), line_rgba=(255, 255, 255, 255), line_width_px=2.0, drape=True)
    add_contours(s, L, h, GRID, u, LEVELS[2::6], width_px=5.0, rgba=(20, 200, 80, 150))
    got = s.render_rgba()
    assert (got != base).any(axis=2).sum() > W * H // 50
    same(got, model_frame(base, u, h, GRID, L))
    assert np.array_equal(s.render_rgba(), got)


@pytest.mark.parametrize("occlude", [False, True])
@pytest.mark.parametrize("width", [1.0, 5.0])
@pytest.mark.parametrize("join", ["round", "none"])
def test_joins_widths_and_occlusion(vf, join, width, occlude):
    W, H = 640, 360
    h = heights(9)
    s = scene(vf, W, H, h)
    base = s.render_rgba()
    u = s.debug_uniforms_f32()
    L = cm.Layers()
    add_contours(s, L, h, GRID, u, LEVELS[::2], width_px=width, rgba=(200, 30, 30, 140), join=join, occlude=occlude, lift=0.01 if occlude else 0.0)
    same(s.render_rgba(), model_frame(base, u, h, GRID, L))
    if occlude:                                               # set_layer_occlusion works on a contour layer like on a line layer
        s.set_layer_occlusion(0, False)
        L.set_occlusion(0, False)
        same(s.render_rgba(), model_frame(base, u, h, GRID, L))


@pytest.mark.parametrize("grid", [100, 257])
def test_small_grids_a_nan_texel_and_levels_through_vertices(vf, grid):
    """grid 100: 99 cells, border blocks are masked; a NaN texel: its triangles emit nothing and the bounds leave it out; three levels
    are vertex heights, so contours pass exactly through vertices"""
    W, H = 800, 450
    h = heights(6, (64, 80))
    h[20, 30] = np.nan
    s = vf.Scene(W, H, grid=grid)
    s.set_height_from_r32f(h)
    s.set_camera_look_at(*CAMERAS["default"])
    base = s.render_rgba()
    u = s.debug_uniforms_f32()
    surf = cm.surface(h, grid)
    assert np.isnan(surf).any()
    assert s.height_bounds() == cm.bounds(surf)
    through = [surf[grid // 2, grid // 3], surf[3, grid - 2], surf[grid - 1, 0]]
    levels = np.unique(np.concatenate([LEVELS[::2], np.asarray(through, np.float32)]))
    L = cm.Layers()
    add_contours(s, L, h, grid, u, levels, width_px=3.0, rgba=(0, 0, 0, 160))
    add_contours(s, L, h, grid, u, levels[::2], width_px=1.0, rgba=(255, 255, 255, 255), join="none", lift=0.05)
    same(s.render_rgba(), model_frame(base, u, h, grid, L))


def terrain(W, H, grid, h, u):
    from vulkan_forge_amd import cabi
    lut = np.load(os.path.join(support.HERE, "golden", "colormaps_rgba8.npz"))["viridis"]
    t = cabi.Terrain(W, H, grid, lut)
    t.set_height(h)
    t.set_uniforms(u)
    return t


def frame(t, u=None):
    if u is not None:
        t.set_uniforms(u)
    t.render()
    return t.read_rgba()


def test_plateaus_on_a_level_exaggeration_and_snapshot(vf):
    """Heights near 2^20, where binary32 has a step of 1/8: the surface is made of plateaus, and every level is a multiple of 1/8 that
    whole groups of vertices lie on exactly.  The layer follows a change of exaggeration; a height upload leaves its records as
    they are (they drape on the new surface)."""
    W, H, grid = 960, 540, 257
    rng = np.random.default_rng(12)
    big = np.float32(2.0 ** 20)
    h = (big + np.float32(0.125) * rng.integers(0, 24, (40, 40))).astype(np.float32)
    s = vf.Scene(W, H, grid=grid)
    s.set_camera_look_at((3.0, 3.0, 3.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0)
    u = s.debug_uniforms_f32().copy()
    u[38] = 2.0 ** -20                                        # world y = h * exaggeration: about 1
    surf = cm.surface(h, grid)
    levels = (big + np.float32([0.5, 1.0, 1.5, 2.0, 2.5])).astype(np.float32)
    assert sum(int((surf == v).sum()) for v in levels) > 1000 and (surf[:, 1:] == surf[:, :-1]).mean() > 0.3
    plain, t = terrain(W, H, grid, h, u), terrain(W, H, grid, h, u)
    assert t.height_bounds() == cm.bounds(surf)
    L = cm.Layers()
    lid, nseg = t.add_contours(levels, width_px=3.0, rgba=(255, 255, 255, 170), join=0)
    L.contours(h, grid, u, levels, width_px=3.0, rgba=(255, 255, 255, 170))
    assert nseg == L.nsegments > 1000 and t.layer_primitive_count(lid) == 2 * nseg
    base = frame(plain)
    got = frame(t)
    assert (got != base).any(axis=2).sum() > 2000
    same(got, ocm.composite(base, np.zeros((H, W), np.uint32), u, h, grid, L))
    u2 = u.copy()
    u2[38] = 1.5 * 2.0 ** -20                                 # exaggeration changed after the add
    base2 = frame(plain, u2)
    assert not np.array_equal(base2, base)
    same(frame(t, u2), ocm.composite(base2, np.zeros((H, W), np.uint32), u2, h, grid, L))
    h3 = (big + np.float32(0.125) * rng.integers(0, 24, (40, 40))).astype(np.float32)
    plain.set_height(h3)
    t.set_height(h3)                                          # snapshot: the records stay, draped on the new surface
    assert t.layer_primitive_count(lid) == 2 * nseg
    same(frame(t), ocm.composite(frame(plain), np.zeros((H, W), np.uint32), u2, h3, grid, L))
    t.close()
    plain.close()


def test_interval_levels_and_terrain_spike(vf):
    from vulkan_forge_amd import _overlays as ov
    W, H = 640, 360
    h = heights(3)
    s = scene(vf, W, H, h)
    base = s.render_rgba()
    u = s.debug_uniforms_f32()
    lo, hi = s.height_bounds()
    assert (lo, hi) == cm.bounds(cm.surface(h, GRID))
    levels = ov.contour_args(None, 0.2, 0.05, 1.0, (0, 0, 0, 255), 0.0, "round", (lo, hi))[0]
    assert len(levels) >= 5 and levels[0] >= lo and levels[-1] <= hi and levels[0] - np.float32(0.2) < lo
    L = cm.Layers()
    lid = s.add_contours(interval=0.2, base=0.05)
    L.contours(h, GRID, u, levels)
    assert s.layer_primitive_count(lid) == 2 * L.nsegments
    same(s.render_rgba(), model_frame(base, u, h, GRID, L))
    with pytest.raises(ValueError, match="exactly one"):
        s.add_contours()
    with pytest.raises(ValueError, match="65536"):
        s.add_contours(interval=1e-6)
    spike = vf.TerrainSpike(160, 120, grid=48)
    blo, bhi = spike.height_bounds()
    assert blo < bhi
    lid = spike.add_contours(interval=0.1)
    assert spike.layer_primitive_count(lid) > 0
    plain = vf.TerrainSpike(160, 120, grid=48).render_rgba()
    assert not np.array_equal(spike.render_rgba(), plain)


def test_empty_layer_and_clear_overlays(vf):
    W, H = 320, 200
    h = heights(4)
    plain = scene(vf, W, H, h).render_rgba()
    s = scene(vf, W, H, h)
    assert s.add_contours(np.float32([50.0])) == 0            # no segment: an empty layer with its id
    assert s.layer_primitive_count(0) == 0
    assert np.array_equal(s.render_rgba(), plain)
    assert s.add_contours(LEVELS, width_px=2.0, occlude=True) == 1
    assert not np.array_equal(s.render_rgba(), plain)
    s.clear_overlays()
    assert np.array_equal(s.render_rgba(), plain)
    assert np.array_equal(s.render_rgba(), plain)
    with pytest.raises(RuntimeError, match="no overlay layer"):
        s.layer_primitive_count(0)


def test_over_budget_is_refused_and_changes_nothing(vf):
    W, H = 640, 360
    h = heights(2)
    s = scene(vf, W, H, h)
    s.add_contours(LEVELS[::4], width_px=2.0, rgba=(255, 0, 0, 255))
    before = s.render_rgba()
    n0 = s.layer_primitive_count(0)
    dense = np.linspace(-0.7, 0.9, 40000).astype(np.float32)  # random heights on grid 1024: every triangle crosses thousands of these
    with pytest.raises(RuntimeError, match=r"contours: \d+ segments .* 2\^24"):
        s.add_contours(dense, join="none")
    assert s.layer_primitive_count(0) == n0
    with pytest.raises(RuntimeError, match="no overlay layer"):
        s.layer_primitive_count(1)
    assert np.array_equal(s.render_rgba(), before)
    assert s.add_contours(LEVELS[1::4]) == 1                  # and the handle still takes layers
    assert not np.array_equal(s.render_rgba(), before)


def test_bad_arguments_and_a_sharded_handle_refuse(vf):
    from vulkan_forge_amd import cabi
    lib = cabi.load()
    t = cabi.Terrain(64, 128, 32, np.zeros(1024, np.uint8))
    t.set_uniforms(vf.Scene(64, 128, grid=32).debug_uniforms_f32())
    col = ctypes.cast((ctypes.c_uint8 * 4)(0, 0, 0, 255), ctypes.c_void_p)
    lv = np.float32([0.0, 0.1])

    def call(levels, n=None, width=1.0, lift=0.0, join=0, occlude=0, bias=0.01):
        levels = np.asarray(levels, np.float32)
        return lib.vf_terrain_add_contours(t.t, levels.ctypes.data, len(levels) if n is None else n, width, col, lift, join, occlude, bias, None, None)

    assert call([0.1, 0.0]) == cabi.VF_ERR_INVALID            # not ascending
    assert call([0.0, 0.0]) == cabi.VF_ERR_INVALID
    assert call([0.0, np.nan]) == cabi.VF_ERR_INVALID
    assert call(lv, n=0) == cabi.VF_ERR_INVALID
    assert call(lv, n=65537) == cabi.VF_ERR_INVALID
    assert call(lv, width=np.inf) == cabi.VF_ERR_INVALID
    assert call(lv, lift=np.nan) == cabi.VF_ERR_INVALID
    assert call(lv, join=2) == cabi.VF_ERR_INVALID
    assert call(lv, occlude=1, bias=-1.0) == cabi.VF_ERR_INVALID
    with pytest.raises(cabi.VfError, match="no overlay layer"):
        t.layer_primitive_count(0)                            # nothing was committed
    assert call(lv) == cabi.VF_OK
    t.clear_overlays()
    t.set_shard(1, 2, 64)
    assert call(lv) == cabi.VF_ERR_INVALID
    assert "whole-frame" in lib.vf_last_error().decode()
    t.close()

"""The far end of every size range the C ABI accepts (include/vf_hip.h), rendered and held to the oracle and the CPU models with the
comparisons of the rest of the suite: EXACT colour equal, FAST colour within RGBA_TOL (1 LSB), visibility equal, feature passes
equal to their models bit for bit.  No tolerance of its own.

  frames        16384 pixels a side: 256 tile columns or rows, 1024 overlay bins, int16 pixel boxes; extreme aspects over the whole
                frame, the full 16384 x 16384 frame over its first, middle and last bands, 256 registered stripes and 256 bands
  read-back     the triangle path at 16384 x 8 and 8 x 16384; render_png at 16384 x 16 (tests/test_gpu_api.py: the PNG scanlines)
  textures      32768 texels a side
  ambient       reach 1024 on a grid that does not clip it (16 earlier tiles in the scan's table), 64 directions
  contours      65536 levels, millions of segments in one block

tests/limit_cases.py describes the cases; tests/test_limit_cases.py shows on the CPU that each reaches the edge it is named for.
One handle at a time: a 16384 x 16384 handle holds more than 1 GiB of device memory."""

import numpy as np
import pytest

import limit_cases as lc
from support import cabi  # noqa: F401
from test_gpu_parity import EXACT, assert_parity, hip_frame, note_fast

pytestmark = pytest.mark.gpu


def threads(oracle):
    return min(16, oracle.max_threads())


# ---- 1a. extreme aspects ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.ASPECT_CASES, ids=[c["name"] for c in lc.ASPECT_CASES])
def test_extreme_aspects_equal_the_oracle(cabi, oracle, luts, case):
    W, H, G = case["W"], case["H"], case["grid"]
    u, h, lut = lc.uniforms(case, oracle), lc.heights(case), luts[case["cmap"]]
    ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, lut, nthreads=threads(oracle))
    rgba, vis = hip_frame(cabi, u, W, H, G, h, lut, frames=case["frames"])
    assert_parity(rgba, vis, ref_rgba, ref_vis)


# ---- 1b. the full frame ----------------------------------------------------------------------------------------------
def read_rows(t, y0, rows):
    out = np.empty((rows, t.W, 4), np.uint8)
    t._check(t.lib.vf_terrain_read_rgba(t.t, out.ctypes.data, y0, rows))
    return out


def test_the_full_16384_frame_equals_the_oracle_on_its_first_middle_and_last_bands(cabi, oracle, luts):
    c = lc.FULL
    W, H, G = c["W"], c["H"], c["grid"]
    u, h, lut = lc.uniforms(c, oracle), lc.heights(c), luts[c["cmap"]]
    t = cabi.Terrain(W, H, G, lut)
    try:
        t.set_height(h); t.set_uniforms(u); t.set_shade_precision(EXACT)
        t.enable_timing(True)
        for _ in range(c["frames"]):                                   # the second frame is planned from the first one's feedback
            t.render()
        items = len(t.item_stats())
        t.enable_timing(False)
        assert items > 4096, items                                      # k_plan_sort orders more than one 4096-item run
        for rank in lc.FULL_RANKS:
            ref, _ = oracle.render_terrain(u, W, H, G, h, lut, rank=rank, nranks=lc.FULL_NRANKS, band_h=lc.FULL_BAND, want_vis=False, nthreads=threads(oracle))
            rows = lc.rows_of(rank, lc.FULL_NRANKS, lc.FULL_BAND, H)
            for y0 in rows[::lc.FULL_BAND]:                             # (the oracle touches the rank's rows only)
                got = read_rows(t, int(y0), lc.FULL_BAND)
                d = (got != ref[y0:y0 + lc.FULL_BAND]).any(axis=2)
                assert not d.any(), f"rank {rank} rows from {y0}: {int(d.sum())} pixels differ, first at {np.argwhere(d)[:4].tolist()}"
    finally:
        t.close()


# ---- 1c. shards at the limit -----------------------------------------------------------------------------------------
def test_256_stripes_and_interleaved_tile_shards_equal_the_whole_frame(cabi, oracle, luts):
    c = lc.SHARD_WIDE
    W, H, G = c["W"], c["H"], c["grid"]
    u, h, lut = lc.uniforms(c, oracle), lc.heights(c), luts[c["cmap"]]
    owner = lc.stripe_owners()
    assert len(owner) == lc.MAX_STRIPES == (W + 63) // 64
    uneven = cabi.register_stripe_map(owner, 0, lc.SHARD_RANKS)
    with pytest.raises(cabi.VfError, match="256 stripes"):
        cabi.register_stripe_map(np.zeros(lc.MAX_STRIPES + 1, np.uint8), 0, lc.SHARD_RANKS)
    t = cabi.Terrain(W, H, G, lut)
    try:
        t.set_height(h); t.set_uniforms(u)
        for _ in range(3):
            t.render()
        whole = t.read_rgba()
        ref_rgba, _ = oracle.render_terrain(u, W, H, G, h, lut, want_vis=False, nthreads=threads(oracle))
        note_fast(whole, ref_rgba)
        for skew in (0, uneven):
            out = np.zeros_like(whole)
            seen = 0
            for r in range(lc.SHARD_RANKS):
                t.set_tile_shard(r, lc.SHARD_RANKS, skew)
                for _ in range(3):
                    t.render()
                tiles = t.read_tiles()
                lay = cabi.tile_layout(W, H, r, lc.SHARD_RANKS, skew, lib=t.lib)
                assert tiles.shape[0] == len(lay) == t.local_tiles()
                if skew:
                    assert sorted(set(lay[:, 0].tolist())) == np.flatnonzero(owner == r).tolist()
                for k, (tx, ty) in enumerate(lay):
                    out[ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64] = tiles[k]
                seen += len(lay)
            assert seen == (W // 64) * (H // 64)
            assert np.array_equal(out, whole), skew
    finally:
        t.close()


def test_256_bands_for_8_ranks_equal_the_whole_frame(cabi, oracle, luts):
    c = lc.SHARD_TALL
    W, H, G = c["W"], c["H"], c["grid"]
    u, h, lut = lc.uniforms(c, oracle), lc.heights(c), luts[c["cmap"]]
    t = cabi.Terrain(W, H, G, lut)
    try:
        t.set_height(h); t.set_uniforms(u)
        for _ in range(3):
            t.render()
        whole = t.read_rgba()
        ref_rgba, _ = oracle.render_terrain(u, W, H, G, h, lut, want_vis=False, nthreads=threads(oracle))
        note_fast(whole, ref_rgba)
        out = np.zeros_like(whole)
        for r in range(lc.SHARD_RANKS):
            t.set_shard(r, lc.SHARD_RANKS, 64)
            for _ in range(3):
                t.render()
            out[lc.rows_of(r, lc.SHARD_RANKS, 64, H)] = t.read_rgba()
        assert np.array_equal(out, whole)
    finally:
        t.close()


# ---- 1d. read-back ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(lc.MAX_FRAME, 8), (8, lc.MAX_FRAME)])
def test_triangle_path_at_the_frame_limit(oracle, W, H):
    """(the Renderer class: the shim function render_triangle_rgba keeps the reference's guard rail of 8192 pixels, _validate.py)"""
    import vulkan_forge as vf
    a = vf.Renderer(W, H).render_triangle_rgba()
    ref = oracle.render_triangle(W, H)
    assert a.shape == (H, W, 4) and a.dtype == np.uint8
    assert np.array_equal(a, ref)
    assert len(np.unique(ref.reshape(-1, 4), axis=0)) > 2               # (the triangle shows)
    with pytest.raises(ValueError, match="8192"):
        vf.render_triangle_rgba(W, H)


def test_render_png_round_trips_at_16384_columns(tmp_path):
    import vulkan_forge as vf
    from PIL import Image
    W, H = lc.MAX_FRAME, 16
    s = vf.Scene(W, H, grid=257)
    s.set_height_from_r32f(lc.noise(7400, (40, 257)))
    s.set_camera_look_at(*lc.top_down(W, H))
    out = tmp_path / "wide.png"
    s.render_png(str(out))
    png = np.asarray(Image.open(out).convert("RGBA"))
    rgba = s.render_rgba()
    assert png.shape == (H, W, 4) and np.array_equal(png, rgba)
    assert len(np.unique(rgba.reshape(-1, 4), axis=0)) > 100            # (a picture, not the clear colour)


# ---- 3. ambient occlusion at reach 1024 and at 64 directions ---------------------------------------------------------
def _field_cases():
    import ambient_model as abm
    return abm.LIMIT_FIELD_CASES


@pytest.mark.parametrize("grid,exag,reach,D", _field_cases())
def test_sky_view_field_at_the_reach_and_direction_limits(cabi, oracle, grid, exag, reach, D):
    import ambient_model as abm
    from overlay_scenes import CAMERAS
    from support import assert_field
    h = abm.limit_heights()
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, 64, 64, *CAMERAS["default"]), np.float32).reshape(44)
    u[38] = exag
    dirs = abm.case_directions(D)
    assert reach == lc.MAX_REACH and grid > reach or len(dirs) == lc.MAX_DIRECTIONS
    want = abm.field(u, h, grid, dirs, reach)
    t = cabi.Terrain(64, 64, grid, np.zeros(1024, np.uint8))
    try:
        t.set_height(h); t.set_uniforms(u)
        t.set_ambient_occlusion(False, reach=reach, directions=dirs)
        got = t.sky_view_field()
    finally:
        t.close()
    assert got.shape == (grid, grid) and got.dtype == np.float32
    assert_field(got, want, f"grid {grid} reach {reach} directions {len(dirs)}")
    assert ((want > 0.1) & (want < 0.9)).mean() > 0.1


# ---- 4. height textures of 32768 texels a side -----------------------------------------------------------------------
@pytest.mark.parametrize("shape", lc.TEXTURE_SHAPES, ids=["x".join(map(str, s)) for s in lc.TEXTURE_SHAPES])
def test_height_textures_of_32768_texels(cabi, oracle, luts, shape):
    W, H, G = lc.TEXTURE_FRAME
    h = lc.big_texture(shape)
    u = oracle.default_uniforms(1, W, H)
    for mode in (oracle.SHADE_REFERENCE, oracle.SHADE_SPEC_T32):         # SPEC_T32 takes its normals from the texture with tw-scaled indices
        ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, luts["terrain"], shade_mode=mode, nthreads=8)
        rgba, vis = hip_frame(cabi, u, W, H, G, h, luts["terrain"], shade_mode=mode)
        assert_parity(rgba, vis, ref_rgba, ref_vis)


def test_a_texture_of_32769_texels_is_refused_and_the_handle_keeps_its_texture(cabi, oracle, luts):
    W, H, G = lc.TEXTURE_FRAME
    h = lc.big_texture(lc.TEXTURE_SHAPES[0])
    u = oracle.default_uniforms(1, W, H)
    ref_rgba, ref_vis = oracle.render_terrain(u, W, H, G, h, luts["terrain"], nthreads=8)
    t = cabi.Terrain(W, H, G, luts["terrain"])
    try:
        t.set_uniforms(u); t.set_height(h); t.set_shade_precision(EXACT)
        t.render()
        for shape in ((1, lc.MAX_TEXTURE + 1), (lc.MAX_TEXTURE + 1, 1)):
            with pytest.raises(cabi.VfError, match="1..32768"):
                t.set_height(np.ones(shape, np.float32))
        t.render()
        assert_parity(t.read_rgba(), t.read_visibility(), ref_rgba, ref_vis)
    finally:
        t.close()


# ---- 5. contours at 65536 levels -------------------------------------------------------------------------------------
def test_contours_at_65536_levels_equal_the_model(cabi, oracle, luts):
    """The frame compared is the one of the full 65536-level layer (join none): the model's composite of its 2.2 million segments takes
    about 3 s on the CPU."""
    import contour_model as cm
    c = lc.CONTOURS
    W, H, G = c["W"], c["H"], c["grid"]
    h, u = lc.heights(c), lc.uniforms(c, oracle)
    surf = cm.surface(h, G)
    t = cabi.Terrain(W, H, G, luts["viridis"])
    try:
        t.set_height(h); t.set_uniforms(u); t.set_shade_precision(EXACT)
        assert t.height_bounds() == cm.bounds(surf)
        levels = lc.contour_levels(t.height_bounds())
        assert len(levels) == lc.MAX_LEVELS and (np.diff(levels) > 0).all()
        t.render()
        base = t.read_rgba()
        kw = dict(width_px=1.0, rgba=(0, 0, 0, 255))
        L = cm.Layers()
        L.contours(h, G, u, levels, join="none", **kw)
        lid, nseg = t.add_contours(levels, join=1, **kw)
        assert nseg == L.nsegments > 2000000 and t.layer_primitive_count(lid) == len(L.recs[-1]) == nseg
        t.render()
        got = t.read_rgba()
        want = cm.ocm.composite(base, np.zeros((H, W), np.uint32), u, h, G, L)
        d = (got != want).any(axis=2)
        assert not d.any(), f"{int(d.sum())} pixels differ from the model, first at {np.argwhere(d)[:4].tolist()}"
        assert (got != base).any(axis=2).mean() > 0.05
        t.clear_overlays()
        R = cm.Layers()
        R.contours(h, G, u, levels, join="round", **kw)
        lid, nseg = t.add_contours(levels, join=0, **kw)                 # round joins: two records a segment, within the 2^24 budget
        assert nseg == R.nsegments and t.layer_primitive_count(lid) == len(R.recs[-1]) == 2 * nseg
    finally:
        t.close()


def test_contours_over_the_record_budget_at_65536_levels_are_refused(cabi, oracle, luts):
    c = lc.CONTOURS
    W, H, G = c["W"], c["H"], lc.CONTOURS_REFUSED_GRID
    h, u = lc.heights(c), lc.uniforms(c, oracle)
    t = cabi.Terrain(W, H, G, luts["viridis"])
    try:
        t.set_height(h); t.set_uniforms(u)
        lid, _ = t.add_contours(np.float32([0.0, 0.1]), width_px=2.0, rgba=(255, 0, 0, 255))
        t.render()
        before, n0 = t.read_rgba(), t.layer_primitive_count(lid)
        with pytest.raises(cabi.VfError, match=r"2\^24"):
            t.add_contours(lc.contour_levels(t.height_bounds()), join=0)
        assert t.layer_primitive_count(lid) == n0
        with pytest.raises(cabi.VfError, match="no overlay layer"):
            t.layer_primitive_count(lid + 1)
        t.render()
        assert np.array_equal(t.read_rgba(), before)
    finally:
        t.close()

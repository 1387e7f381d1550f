"""What the flood and the spill share on the host and the list of the passes behind
the tile kernel, pinned from outside: clear_* leaves the scan counter and the forced group settings and nothing else; with two
features on, render_batch, render_batch_host, set_tile_shard and set_shard refuse with the message of the feature they test first,
which is not the order the passes are drawn in.  One handle of grid 65 (two tiles a side in both fills) and a frame of 64 x 64."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import spill_model as spm
from overlay_scenes import heights
from support import bits

fdm, cm = spm.fdm, spm.cm
W = H = 64
GRID = 65
TINT = dict(shallow_rgba=(0, 255, 255, 200), deep_rgba=(20, 20, 20, 90), depth_full=0.3)


def uniforms():
    return support.uniforms(W, H, exag=0.6)


def terrain(supersample=None):
    from vulkan_forge_amd import cabi
    lut = np.load(os.path.join(support.HERE, "golden", "colormaps_rgba8.npz"))["viridis"]
    t = cabi.Terrain(W, H, GRID, lut, supersample=supersample)
    t.set_height(heights(**fdm.FIELD_TEXTURE))
    t.set_uniforms(uniforms())
    return t


def frame(t):
    t.render()
    return t.read_rgba().copy()


# ---- the reset ----

def test_clear_flood_keeps_the_scan_counter_and_the_forced_group_and_nothing_else():
    h = cm.surface(heights(**fdm.FIELD_TEXTURE), GRID)
    level = fdm.field_level(h, 0.5)
    _, several = fdm.field_seed_lists(h, level, GRID)
    t = terrain()
    plain = frame(t)
    never = t.flood_info()
    assert never["scans"] == 0 and never["group"] == 16 and never["vertices"] is None
    t.flood_group(4)
    t.set_flood(level, several, **TINT)
    first = t.flood_field()
    assert (first > 0).any()
    t.set_flood(fdm.field_level(h, 0.6), "edges", **TINT)     # a changed input: the field is computed again
    assert (bits(t.flood_field()) != bits(first)).any()
    assert (frame(t) != plain).any()
    info = t.flood_info()
    assert (info["scans"], info["group"], info["enabled"], info["depth_full"]) == (2, 4, True, pytest.approx(0.3))
    assert info["flooded_vertices"] > 0 and info["passes"] > 0
    t.clear_flood()
    assert t.flood_scans() == 2
    assert t.flood_info() == {**never, "scans": 2, "group": 4}
    assert np.array_equal(frame(t), plain)
    with pytest.raises(RuntimeError, match="no flood set"):
        t.flood_field()
    t.set_flood(level, several, **TINT)
    assert np.array_equal(bits(t.flood_field()), bits(first))
    info = t.flood_info()
    assert (info["scans"], info["group"]) == (3, 4)
    t.close()


def test_clear_spill_keeps_the_scan_counter_and_the_forced_group_settings_and_nothing_else():
    h = cm.surface(heights(**fdm.FIELD_TEXTURE), GRID)
    _, several = spm.field_seed_lists(h, GRID)
    t = terrain()
    plain = frame(t)
    never = t.spill_info()
    assert never["scans"] == 0 and never["group"] == 16 and never["vertices"] is None
    t.spill_group(4, flags=False)
    t.set_spill(several, **TINT)
    first, first_sink = t.spill_field(), t.sink_depth_field()
    t.set_spill("edges", **TINT)                              # a changed input: the field is computed again
    assert (bits(t.spill_field()) != bits(first)).any()
    assert (frame(t) != plain).any()
    info = t.spill_info()
    assert (info["scans"], info["group"], info["enabled"], info["depth_full"]) == (2, 4, True, pytest.approx(0.3))
    assert info["reached_vertices"] > 0 and info["passes"] > 0 and info["tile_runs"] > 0
    t.clear_spill()
    assert t.spill_scans() == 2
    assert t.spill_info() == {**never, "scans": 2, "group": 4}
    assert np.array_equal(frame(t), plain)
    with pytest.raises(RuntimeError, match="no spill set"):
        t.spill_field()
    t.set_spill(several, **TINT)
    assert np.array_equal(bits(t.spill_field()), bits(first)) and np.array_equal(bits(t.sink_depth_field()), bits(first_sink))
    info = t.spill_info()
    assert (info["scans"], info["group"]) == (3, 4)
    queued = -(-info["passes"] // 4) * 4                      # (the passes of the last group behind the fixpoint run too)
    assert info["tile_runs"] == queued * spm.n_tiles(GRID)    # the activity flags are still ignored: every tile in every pass
    t.close()


# ---- the order of the refusals ----

# feature -> (enable, disable, what render_batch says, what the shard calls say); in the order the calls test them
FEATURES = {
    "shadows": (lambda t: t.set_shadows(True), lambda t: t.set_shadows(False),
                "render_batch on a handle with shadows enabled is not supported: a sun per pose would need a shadow field per pose",
                "the handle has shadows enabled: shadows need a whole-frame handle"),
    "ambient": (lambda t: t.set_ambient_occlusion(True), lambda t: t.set_ambient_occlusion(False),
                "render_batch on a handle with ambient occlusion enabled is not supported",
                "the handle has ambient occlusion enabled: it needs a whole-frame handle"),
    "viewshed": (lambda t: t.set_viewshed((0.1, 0.2)), lambda t: t.clear_viewshed(),
                 "render_batch on a handle with a viewshed enabled is not supported",
                 "the handle has a viewshed enabled: it needs a whole-frame handle"),
    "cumulative": (lambda t: t.set_cumulative_viewshed([(0.1, 0.2), (-0.4, 0.3)]), lambda t: t.clear_cumulative_viewshed(),
                   "render_batch on a handle with a cumulative viewshed enabled is not supported",
                   "the handle has a cumulative viewshed enabled: it needs a whole-frame handle"),
    "exposure": (lambda t: t.set_sun_exposure([(0.3, 0.8, -0.5), (-0.2, 0.6, 0.4)]), lambda t: t.clear_sun_exposure(),
                 "render_batch on a handle with sun exposure enabled is not supported",
                 "the handle has sun exposure enabled: it needs a whole-frame handle"),
    "haze": (lambda t: t.set_haze(0.5), lambda t: t.clear_haze(),
             "render_batch on a handle with haze enabled is not supported",
             "the handle has haze enabled: it needs a whole-frame handle"),
    "flood": (lambda t: t.set_flood(0.1), lambda t: t.clear_flood(),
              "render_batch on a handle with a flood enabled is not supported",
              "the handle has a flood enabled: it needs a whole-frame handle"),
    "spill": (lambda t: t.set_spill(), lambda t: t.clear_spill(),
              "render_batch on a handle with the spill enabled is not supported",
              "the handle has the spill enabled: it needs a whole-frame handle"),
}
ORDER = list(FEATURES)
SUPERSAMPLED = ("render_batch on a supersampled handle is not supported: render the poses one by one (vf_terrain_render)",
                "the handle is supersampled: the resolve needs a whole-frame handle")
# (the last four are drawn in the other order: exposure, cumulative, viewshed; flood before haze)
PAIRS = (("shadows", "flood"), ("flood", "spill"), ("viewshed", "haze"), ("cumulative", "spill"), ("shadows", "ambient"),
         ("cumulative", "exposure"), ("viewshed", "cumulative"), ("haze", "flood"), ("ambient", "spill"))


def refusals(t):
    """the messages of (render_batch, render_batch_host, set_tile_shard, set_shard)"""
    from vulkan_forge_amd import cabi
    u = uniforms().reshape(1, 44)
    said = []
    for call in (lambda: t.render_batch(u), lambda: t.render_batch_host(u), lambda: t.set_tile_shard(0, 2), lambda: t.set_shard(0, 2, 64)):
        with pytest.raises(cabi.VfError) as e:
            call()
        said.append(str(e.value))
    return said


def test_two_features_on_are_refused_with_the_message_of_the_one_tested_first():
    t = terrain()
    for a, b in PAIRS:
        assert ORDER.index(a) < ORDER.index(b)
        for first, second in ((a, b), (b, a)):                # (the order of enabling does not matter)
            FEATURES[first][0](t)
            FEATURES[second][0](t)
            _, _, batch, shard = FEATURES[a]
            assert refusals(t) == [batch, batch, shard, shard], (a, b)
            FEATURES[a][1](t)
            _, _, batch, shard = FEATURES[b]
            assert refusals(t) == [batch, batch, shard, shard], (b, "alone")
            FEATURES[b][1](t)
    t.render_batch(uniforms().reshape(1, 44))                 # everything is off again: nothing is refused
    t.set_tile_shard(0, 1)
    t.close()


def test_the_place_of_the_supersampling_refusal_among_the_features():
    t = terrain(supersample=2)
    assert refusals(t) == [SUPERSAMPLED[0], SUPERSAMPLED[0], SUPERSAMPLED[1], SUPERSAMPLED[1]]
    # render_batch: behind every feature; set_tile_shard: behind the viewshed; set_shard: behind sun exposure
    for name, tile_shard_first, shard_first in (("viewshed", True, True), ("cumulative", False, True), ("exposure", False, True),
                                                ("haze", False, False), ("spill", False, False)):
        on, off, batch, shard = FEATURES[name]
        on(t)
        assert refusals(t) == [batch, batch, shard if tile_shard_first else SUPERSAMPLED[1], shard if shard_first else SUPERSAMPLED[1]], name
        off(t)
    t.close()

"""The GPU feature soak's slice (tests/test_gpu_feature_soak.py) is not vacuous: the reference alone (soak_features.case / expected,
no GPU), over exactly the corners and seeds that module runs, covers pixels, rewrites part of them, draws overlays, meets every
mutation, and is deterministic."""
import collections

import numpy as np
import pytest

import soak_features as sf
from test_gpu_feature_soak import BLOCKS, FIRST_SEED, PER_BLOCK

SEEDS = range(FIRST_SEED, FIRST_SEED + BLOCKS * PER_BLOCK)


@pytest.fixture(scope="module")
def slice_shares(oracle):
    """shares() of every seed of the slice (None for a degenerate camera) and of every corner, computed once"""
    seeds = {}
    for seed in SEEDS:
        try:
            seeds[seed] = sf.shares(sf.case(seed))
        except RuntimeError:
            seeds[seed] = None
    return seeds, {c["name"]: sf.shares(c) for c in sf.CORNERS}


def test_no_seed_of_the_slice_is_skipped(slice_shares):
    seeds, _ = slice_shares
    assert [s for s, v in seeds.items() if v is None] == []


def test_the_slice_covers_rewrites_and_draws(slice_shares):
    seeds, corners = slice_shares
    stat = [v for v in seeds.values() if v is not None] + list(corners.values())
    print("\n" + sf.describe(stat))
    assert sum(s["covered"] > 0.05 for s in stat) >= 0.4 * len(stat)
    shaded = [s["rewritten"] for s in stat if s["rewritten"] is not None]     # (a shade feature is on in every case)
    partial = sum(0.1 < r < 0.9 for r in shaded)
    # (measured 29 % against the bound of 25 %; a change to the draw in soak_features._make moves it, and the draw, not the bound, is what to tune then)
    assert partial >= 0.25 * len(shaded), (partial, len(shaded))
    assert sum(s["overlays_show"] for s in stat) >= 0.8 * len(stat)


def test_every_mutation_occurs_and_every_corner_runs_the_chain(oracle):
    kinds = collections.Counter(sf.case(seed)["mutation"] for seed in SEEDS)
    assert all(kinds[k] >= 3 for k in sf.MUTATIONS), kinds
    for c in sf.CORNERS:
        state = sf.featured(c, sf.initial_state(c), overlays=True)
        e = sf.expected(c, state)
        assert e["frame"].shape == (c["H"], c["W"], 4) and e["layers"] is not None
        sf.planes(c, state, e["vis"])
        assert sf.expected(c, sf.mutated(c, state))["frame"].shape == (c["H"], c["W"], 4)
    names = [c["name"] for c in sf.CORNERS]
    assert len(set(names)) == len(names)


def test_the_corners_hold_the_edges_they_are_named_for(oracle):
    by = {c["name"]: c for c in sf.CORNERS}
    assert {c["grid"] for c in sf.CORNERS} >= {2, 3, 9, 10, 63, 64, 65, 129}
    assert {(c["W"], c["H"]) for c in sf.CORNERS} >= {(1, 1), (15, 17), (16, 16), (17, 15), (64, 64), (65, 63), (16384, 24), (24, 16384)}
    assert {len(c["ambient"]["directions"]) for c in sf.CORNERS} >= {1, 64}
    assert {(c["grid"], c["ambient"]["reach"]) for c in sf.CORNERS} >= {(5, 1.0), (5, 1024.0)}
    assert {c["exaggeration"] for c in sf.CORNERS} >= {0.0, -2.0} and {c["spacing"] for c in sf.CORNERS} >= {0.3, 2.5}
    assert by["texture1x1"]["heights"].shape == (1, 1) and int(np.isnan(by["one_nan_texel"]["heights"]).sum()) == 1
    # an all-NaN texture: no bounds, no contour segment, fields of 1
    c = by["all_nan_texture"]
    state = sf.featured(c, sf.initial_state(c), overlays=True)
    assert sf.cm.bounds(sf.cm.surface(c["heights"], c["grid"])) == (float("inf"), float("-inf"))
    assert list(sf.layers(c, state).segments.values()) == [0]
    P = state["ambient_params"]
    assert (sf.shm.field(state["u"], c["heights"], c["grid"], **state["shadow_params"]) == 1).all()
    assert (sf.abm.field(state["u"], c["heights"], c["grid"], P["directions"], P["reach"]) == 1).all()
    # the plateau: the contour layer has segments, and one of its levels is the height of many vertices
    c = by["constant_texture_level_on_the_plateau"]
    surf = sf.cm.surface(c["heights"], c["grid"])
    assert any(k == "contours" and max(int((surf == v).sum()) for v in kw["levels"]) > 20 for k, kw in c["overlays"])
    assert list(sf.layers(c, sf.featured(c, sf.initial_state(c), overlays=True)).segments.values())[0] > 0


@pytest.mark.parametrize("name", ["grid3_frame15x17_sun_on_horizon", "grid10_frame17x15_sun_on_axis", "grid64_frame65x63"])
def test_the_odd_frames_draw_overlays_in_their_partial_last_bins(oracle, name):
    """what gives the GPU comparison its hold on the overlay bin count: in a frame whose width or height is no multiple of 16 the
    reference's overlays change pixels in the columns from 16 (W // 16) on and the rows from 16 (H // 16) on, so a pass that drops
    the partial last bin column or row differs from it there"""
    c = sf.CORNERS.named(name)
    e = sf.expected(c, sf.featured(c, sf.initial_state(c), overlays=True))
    drawn = (e["frame"] != e["shaded"]).any(axis=2)
    W, H = c["W"], c["H"]
    assert W % 16 and H % 16
    assert drawn[:, 16 * (W // 16):].any() and drawn[16 * (H // 16):, :].any()


@pytest.mark.parametrize("name", ["frame16384x24", "frame24x16384"])
def test_the_frame_limit_corners_reach_the_last_bin_and_both_outer_tiles(oracle, name):
    """the corners at the C ABI's frame limit, from the models alone: the terrain covers the first and the last tile column (wide) or
    row (tall), the overlays change pixels in the last 16-pixel bin column or row, and the shade pass writes part of the covered
    pixels again, not all and not none; everything is on, and pick asks for the pixels at the four corners (soak_features.run_case)"""
    c = sf.CORNERS.named(name)
    W, H = c["W"], c["H"]
    assert max(W, H) == 16384 and c["grid"] >= 129 and c["features"] == "both" and len(c["ambient"]["directions"]) == len(sf._FAN)
    assert {k for k, _ in c["overlays"]} == {"points", "lines", "polygons", "contours"}
    e = sf.expected(c, sf.featured(c, sf.initial_state(c), overlays=True))
    covered = e["vis"] != 0
    drawn = (e["frame"] != e["shaded"]).any(axis=2)
    if W > H:
        covered, drawn = covered.T, drawn.T                   # (the long side first)
    assert covered[:64].any() and covered[-64:].any()
    assert drawn[-16:].any()
    assert 0.1 < e["mask"].sum() / covered.sum() < 0.9


def test_expected_is_deterministic(oracle):
    for c in [sf.case(FIRST_SEED + 3), sf.CORNERS[5]]:
        state = sf.mutated(c, sf.featured(c, sf.initial_state(c), overlays=True))
        a, b = sf.expected(c, state), sf.expected(sf.case(FIRST_SEED + 3) if c["name"].startswith("seed") else c, state)
        for k in ("rgba", "vis", "shaded", "mask", "frame"):
            assert a[k].tobytes() == b[k].tobytes(), k


def test_fresh_seeds_skip_few_cameras(oracle):
    """the script's seeds: at most 10 % may be skipped for a degenerate camera"""
    skipped = 0
    for seed in range(31000, 31100):
        try:
            sf.uniforms(sf.case(seed))
        except RuntimeError:
            skipped += 1
    print(f"\n{skipped} of 100 fresh seeds skipped")
    assert skipped <= 10


def test_the_reduced_fill_corner_has_its_edge_between_the_frame_and_the_bins_edge(oracle):
    """the finding kept as a corner: an edge of the fill lies wholly right of the 17-pixel frame and left of x = 32, on rows where
    the frame's last column is inside the fill"""
    pm = sf.ocm.pm
    c = {k["name"]: k for k in sf.CORNERS}["fill_edge_beyond_the_frame_inside_its_last_bin"]
    assert c["overlays"][-1][1]["polygons"][0][0] is sf.GAP_RING and c["W"] == 17
    u = sf.uniforms(c)
    edges = pm.ring_edges(c["W"], c["H"], u, c["heights"], c["grid"], sf.GAP_RING)
    gap = [e for e in edges if e[6] > c["W"] + 1 and e[7] < 32]
    assert len(gap) == 1
    cov = pm.fill_coverage(c["W"], c["H"], u, c["heights"], c["grid"], [sf.GAP_RING])
    inside = [r for r in np.flatnonzero(cov[:, 16] == 1.0) if gap[0][8] <= r + 0.5 < gap[0][9]]     # (rows whose parity needs that crossing)
    assert len(inside) >= 3

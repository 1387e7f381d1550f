"""The GPU feature soak's slice (tests/test_gpu_feature_soak.py) is not vacuous: the reference alone (soak_features.case / expected,
no GPU), over exactly the corners and seeds that module runs, covers pixels, rewrites part of them, drapes an image over part of
them, draws overlays, meets every mutation, and is deterministic; the draped image's corners hold the edges they are named for."""
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


def test_the_slice_drapes_part_of_what_it_covers(slice_shares):
    """conditions on the reference alone; the draw (soak_features._drape) is what to tune when one fails, not the bound"""
    seeds, corners = slice_shares
    cases = {seed: sf.case(seed) for seed in SEEDS}
    with_drape = [seed for seed in SEEDS if cases[seed]["drape"] is not None]
    assert len(with_drape) >= 0.7 * len(SEEDS) and len(SEEDS) - len(with_drape) >= 4, len(with_drape)
    assert all(c["drape"] is not None for c in sf.CORNERS)
    stat = [seeds[seed] for seed in with_drape if seeds[seed] is not None] + list(corners.values())
    draped = [s for s in stat if s["draped"] is not None]     # (a drape and a covered pixel)
    partial = sum(0.1 < s["draped"] < 0.9 for s in draped)
    cross = sum(s["masks_cross"] for s in draped)
    print(f"\n{len(draped)} draped cases with a covered pixel: the drape rewrites 10-90 % of the covered pixels in {partial}, its mask and the shade pass's cross in {cross}")
    assert len(draped) >= 40
    assert partial >= 0.5 * len(draped), (partial, len(draped))
    assert cross >= len(draped) / 3.0, (cross, len(draped))
    # every size class, both channel counts, every extent kind, every opacity and both filters, among the seeds alone
    D = [cases[seed]["drape"] for seed in with_drape]
    D += [d["replace"] for d in D]
    shapes = [d["image"].shape for d in D]
    assert any(ih * iw == 1 for ih, iw, _ in shapes) and any(ih == 1 and iw > 1 for ih, iw, _ in shapes) and any(iw == 1 and ih > 1 for ih, iw, _ in shapes)
    assert any(ih * iw >= 256 and (ih * iw) % 256 == 0 for ih, iw, _ in shapes) and any(ih * iw >= 256 and (ih * iw) % 256 for ih, iw, _ in shapes)
    assert {ch for _, _, ch in shapes} == {3, 4}
    assert {d["extent_kind"] for d in D} == set(sf.DRAPE_EXTENTS) and {d["opacity"] for d in D} == {1.0, 0.37, 0.0}
    assert {d["filter"] for d in D} == set(sf.DRAPE_FILTERS)
    for seed in with_drape:                                   # drape_replace: another size, the other channel count, another extent, the other filter
        d = cases[seed]["drape"]
        r = d["replace"]
        assert r["image"].shape[:2] != d["image"].shape[:2] and r["image"].shape[2] + d["image"].shape[2] == 7
        assert r["extent"] != d["extent"] and r["filter"] != d["filter"]
    for d in D:                                               # the extent is in the grid's own plane, whatever the spacing
        assert d["extent"] is None or (d["extent"][2] > d["extent"][0] and d["extent"][3] > d["extent"][1] and max(abs(v) for v in d["extent"]) < 6.0)


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
    drawn = (e["frame"] != e["draped"]).any(axis=2)
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
    drawn = (e["frame"] != e["draped"]).any(axis=2)
    if W > H:
        covered, drawn = covered.T, drawn.T                   # (the long side first)
    assert covered[:64].any() and covered[-64:].any()
    assert drawn[-16:].any()
    assert 0.1 < e["mask"].sum() / covered.sum() < 0.9


def test_expected_is_deterministic(oracle):
    for c in [sf.case(FIRST_SEED + 3), sf.case(FIRST_SEED + 7), sf.CORNERS[5]]:
        assert c["drape"] is not None
        for state in (sf.featured(c, sf.initial_state(c), overlays=True), sf.mutated(c, sf.featured(c, sf.initial_state(c), overlays=True))):
            a, b = sf.expected(c, state), sf.expected(sf.case(int(c["name"][4:])) if c["name"].startswith("seed") else c, state)
            for k in ("rgba", "vis", "shaded", "mask", "draped", "drape_mask", "frame"):
                assert a[k].tobytes() == b[k].tobytes(), k
    # a cached entry made without the drape is never returned for a state with it
    c, cache = sf.case(FIRST_SEED + 7), {}
    state = sf.featured(c, sf.initial_state(c))
    bare = sf.expected(c, dict(state, drape=None), cache)
    with_it = sf.expected(c, state, cache)
    assert not bare["drape_mask"].any() and with_it["drape_mask"].any() and (with_it["frame"] != bare["frame"]).any()
    assert with_it["frame"].tobytes() == sf.expected(c, state)["frame"].tobytes()


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


# ---- the draped image's corners ----------------------------------------------------------------------------------------

def draped(name):
    """a corner's state with everything on but the overlays, its reference, and drape_model's sample of the drape pass"""
    c = sf.CORNERS.named(name)
    state = sf.featured(c, sf.initial_state(c))
    e = sf.expected(c, state)
    u, h, G, D, A = state["u"], state["heights"], c["grid"], state["drape"], state["ambient_params"]
    lit = sf.shm.field(u, h, G, **state["shadow_params"]) if state["shadows"] else None
    sky = sf.abm.field(u, h, G, A["directions"], A["reach"]) if state["ambient"] else None
    frame, mask, sample = sf.drm.frame(e["shaded"], e["vis"], u, h, G, sf.lut(c["cmap"]), D["image"], extent=D["extent"], opacity=D["opacity"],
                                       filter=D["filter"], lit=lit, sky=sky, strength=A["strength"], shade_mode=c["mode"], want_sample=True)
    assert np.array_equal(frame, e["draped"]) and np.array_equal(mask, e["drape_mask"])
    return c, state, e, sample


def texel_sample(image, ix, iy):
    """the premultiplied linear (r, g, b, a) of one texel, as drape_model.c forms it"""
    import oracle
    decode = oracle.srgb_tables()[0]
    a = np.float32(image[iy, ix, 3]) / np.float32(255.0)
    return np.array([decode[image[iy, ix, ch]] * a for ch in range(3)] + [a], np.float32)


def grid_position(c, state, vis):
    """the geometry-buffer position of every pixel in the grid's own plane: world x and z over the spacing"""
    _, pos, _ = sf.gbm.planes(vis, state["u"], state["heights"], c["grid"])
    return pos[..., 0] / np.float32(c["spacing"]), pos[..., 2] / np.float32(c["spacing"])


def test_one_texel_under_the_linear_filter(oracle):
    c, state, e, sample = draped("drape_1x1_linear_full_extent")
    D = state["drape"]
    assert D["image"].shape == (1, 1, 4) and D["filter"] == "linear" and D["extent"] is None and c["mutation"] == "drape_opacity_zero"
    covered, m = e["vis"] != 0, e["drape_mask"]
    assert m.any() and not m[~covered].any() and m.sum() >= 0.9 * covered.sum()
    # all four taps are the one texel: fma(f, q - q, q) = q
    assert (sample[m][:, :4] == texel_sample(D["image"], 0, 0)).all()
    # what is covered and not written lies on the grid's border (its interpolated x or z rounds beyond +-1.5)
    x, z = grid_position(c, state, e["vis"])
    rest = covered & ~m
    assert (np.maximum(np.abs(x[rest]), np.abs(z[rest])) > 1.49).all()


def test_an_extent_whose_width_overflows_takes_texel_0_0(oracle):
    c, state, e, sample = draped("drape_extent_overflows")
    D = state["drape"]
    ext = np.array(D["extent"], np.float32)
    with np.errstate(over="ignore"):
        assert np.isfinite(ext).all() and np.isinf(ext[2] - ext[0]) and np.isinf(ext[3] - ext[1])
        assert np.float32(D["image"].shape[1]) / (ext[2] - ext[0]) == 0.0
    assert len({tuple(t) for t in D["image"].reshape(-1, 4)[:, :3].tolist()}) == D["image"].shape[0] * D["image"].shape[1]    # (a wrong texel shows)
    m = e["drape_mask"]
    assert m.any() and np.array_equal(m, e["vis"] != 0)
    assert (sample[m][:, :4] == texel_sample(D["image"], 0, 0)).all()
    assert (e["draped"][m] != e["shaded"][m]).any()


@pytest.mark.parametrize("name", ["drape_extent_off_the_grid", "drape_transparent_image"])
def test_the_corners_that_rewrite_nothing(oracle, name):
    c, state, e, _ = draped(name)
    assert (e["vis"] != 0).sum() > 100 and not e["drape_mask"].any() and np.array_equal(e["draped"], e["shaded"])
    bare = sf.expected(c, dict(state, drape=None))
    assert np.array_equal(e["frame"], bare["frame"])
    if name == "drape_transparent_image":
        assert not state["drape"]["image"][..., 3].any() and state["drape"]["image"][..., :3].any() and c["mutation"] == "drape_replace"
        after = sf.expected(c, sf.mutated(c, state))
        assert c["drape"]["replace"]["image"].shape[2] == 3 and after["drape_mask"].sum() > 100
    else:
        assert state["drape"]["image"][..., 3].all() and state["drape"]["extent"][0] > 1.5


def near_plane_straddlers(c, u):
    """per primitive id - 1: the triangle has vertices on both sides of the near plane (clip z < 0 is out), from the
    uniforms' view and projection (column-major, u[0:16] and u[16:32]) and the surface"""
    G = max(c["grid"], 2)
    surf = sf.cm.surface(c["heights"], c["grid"]).astype(np.float64)
    g = -1.5 + np.arange(G) * (3.0 / (G - 1))
    X, Z = np.meshgrid(g, g)
    world = np.stack([X * u[36], surf * u[38], Z * u[36], np.ones_like(X)], axis=-1)
    V, P = u[0:16].reshape(4, 4).T.astype(np.float64), u[16:32].reshape(4, 4).T.astype(np.float64)
    out = (world @ (P @ V).T)[..., 2] < 0                     # [j, i]
    j, i = np.meshgrid(np.arange(G - 1), np.arange(G - 1), indexing="ij")
    even = np.stack([out[j, i], out[j + 1, i], out[j, i + 1]], -1)
    odd = np.stack([out[j, i + 1], out[j + 1, i], out[j + 1, i + 1]], -1)
    t = np.stack([even, odd], axis=2).reshape(-1, 3)          # primitive 2 (j (G - 1) + i) + odd
    return t.any(axis=1) & ~t.all(axis=1)


def test_the_near_plane_corner_shades_draped_pixels_of_clipped_triangles(oracle):
    c, state, e, sample = draped("drape_near_plane_through_the_terrain")
    assert c["features"] == "both" and c["ambient"]["strength"] > 0 and c["mutation"] == "shadows_off"
    vis, m = e["vis"], e["drape_mask"]
    cut = near_plane_straddlers(c, state["u"])
    straddling = np.zeros(vis.shape, bool)
    straddling[vis != 0] = cut[vis[vis != 0] - 1]
    both = m & straddling
    print(f"\n{int(both.sum())} draped pixels of triangles the near plane cuts, lit < 1 in {int((sample[both][:, 4] < 1).sum())}, amb < 1 in {int((sample[both][:, 5] < 1).sum())}")
    assert both.sum() >= 50
    assert (sample[both][:, 4] < 1).sum() >= 20 and (sample[both][:, 5] < 1).sum() >= 20
    assert (m & ~straddling).any()                            # (and the record path draws draped pixels too)
    # without the shadows the drape's pixels change: a stale lit pointer shows
    after = sf.expected(c, sf.mutated(c, state))
    assert (after["draped"][both] != e["draped"][both]).any()


@pytest.mark.parametrize("name", ["drape_under_spacing_2p5_exaggeration_minus2", "drape_under_spacing_0p3"])
def test_the_spacing_corners_show_an_extent_edge(oracle, name):
    """the extent is in grid coordinates: the written pixels are those whose position over the spacing lies in it, part of the frame"""
    import oracle
    c, state, e, sample = draped(name)
    D = state["drape"]
    assert c["spacing"] != 1.0 and D["filter"] == "nearest" and D["image"][..., 3].all()
    ih, iw = D["image"].shape[:2]
    x0, z0, x1, z1 = D["extent"]
    assert -1.5 < x0 < x1 < 1.5 and -1.5 < z0 < z1 < 1.5
    covered, m = e["vis"] != 0, e["drape_mask"]
    x, z = grid_position(c, state, e["vis"])
    away = lambda v, lo, hi: (np.abs(v - lo) > 1e-3) & (np.abs(v - hi) > 1e-3)     # (the division by the spacing rounds: not at an edge)
    clear = covered & away(x, x0, x1) & away(z, z0, z1)
    inside = (x > x0) & (x < x1) & (z > z0) & (z < z1)
    assert np.array_equal(m[clear], inside[clear])
    assert 0.1 < m.sum() / covered.sum() < 0.9
    assert sum(int((covered & ~m & side).any()) for side in (x < x0, x > x1, z < z0, z > z1)) >= 2
    # and the texel is the one the position over the spacing falls in (every texel distinct)
    decode = oracle.srgb_tables()[0]
    fu, fv = (x - np.float32(x0)) * (np.float32(iw) / (np.float32(x1) - np.float32(x0))), (z - np.float32(z0)) * (np.float32(ih) / (np.float32(z1) - np.float32(z0)))
    sure = m & clear & (np.abs(fu - np.round(fu)) > 0.02) & (np.abs(fv - np.round(fv)) > 0.02)
    assert sure.sum() > 0.5 * m.sum()
    cx, cy = np.floor(fu[sure]).astype(np.int64), np.floor(fv[sure]).astype(np.int64)
    assert np.array_equal(sample[sure][:, 0], decode[cx]) and np.array_equal(sample[sure][:, 1], decode[cy])


def test_the_dense_image_corner(oracle):
    c, state, e, _ = draped("drape_denser_than_the_frame")
    assert state["drape"]["image"].shape == (300, 300, 4) and (c["W"], c["H"]) == (15, 17) and c["mutation"] == "drape_clear"
    assert 0.1 < e["drape_mask"].sum() / (e["vis"] != 0).sum() < 0.9

"""The GPU feature soak's slice (tests/test_gpu_feature_soak.py) is not vacuous: the reference alone (soak_features.case / expected,
no GPU), over exactly the corners and seeds that module runs, covers pixels, rewrites part of them, drapes an image over part of
them, draws overlays, meets every mutation, and is deterministic; the draped image's corners, the late passes' and the flood's and
the spill's hold the edges they are named for; hazed overlay layers cover pixels at opacities strictly inside (0, max_opacity), at
0 and at the cap, every mutation of their flags occurs and does what it must, and their corners hold their edges; no key a case had
before a later generator was added has moved."""
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
        on = sf.featured(c, sf.initial_state(c), overlays=True)
        for state in (on, sf.mutated(c, on), sf.lated(c, on), sf.late_mutated(c, sf.mutated(c, sf.lated(c, on)))):
            a, b = sf.expected(c, state), sf.expected(sf.case(int(c["name"][4:])) if c["name"].startswith("seed") else c, state)
            for k in ("rgba", "vis", "shaded", "mask", "draped", "drape_mask", "late", "haze_opacity", "frame"):
                assert a[k].tobytes() == b[k].tobytes(), k
    # a cached entry made without the drape is never returned for a state with it
    c, cache = sf.case(FIRST_SEED + 7), {}
    state = sf.featured(c, sf.initial_state(c))
    bare = sf.expected(c, dict(state, drape=None), cache)
    with_it = sf.expected(c, state, cache)
    assert not bare["drape_mask"].any() and with_it["drape_mask"].any() and (with_it["frame"] != bare["frame"]).any()
    assert with_it["frame"].tobytes() == sf.expected(c, state)["frame"].tobytes()
    expected_keeps_the_late_passes_apart()


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


# ---- the late passes: mips and anisotropy, the three tints and their fields, haze, supersampling ---------------------------

def test_no_key_older_than_the_late_passes_has_moved():
    """the digest (soak_features.digest: names, values and array bytes of OLD_KEYS) of the slice's seeds and of the corners older
    than the late passes, computed on the commit before the late passes' generator existed"""
    assert sf.digest(sf.case(seed) for seed in SEEDS) == "f937961fa73b2d474bdd3770e7f18db5bce0b3b6af714a22f5821d21b8e7b39a"
    assert sf.digest(sf.CORNERS[i] for i in range(sf.OLD_CORNERS)) == "3f3093f0c0906104c579ceba1b54a8a70fcc15e084847e712536ec3337eee5e4"
    assert set(sf.case(FIRST_SEED)) == set(sf.OLD_KEYS) | {"late", "late_mutation", "late_mutation_args"} | set(sf.WATER_KEYS) | set(sf.HAZED_KEYS)


def test_no_key_older_than_the_water_has_moved():
    """the digest of OLD_KEYS and the three late keys of the slice's seeds and of the 47 corners older than the flood and the spill,
    computed on the commit before their generator existed"""
    keys = sf.OLD_KEYS + ("late", "late_mutation", "late_mutation_args")
    assert sf.digest((sf.case(seed) for seed in SEEDS), keys) == "892ae0c5ec28ccc65906b24782d9cb8918876aed223e07055d63e4e1c27e931d"
    assert sf.digest((sf.CORNERS[i] for i in range(sf.LATE_CORNERS)), keys) == "0d26e23f448e1c352b24e892425bfca31c16341e693a9fcd2dfa731f655952bb"
    assert not any(n.startswith("water_") for n in sf.CORNERS.names[:sf.LATE_CORNERS]) and all(n.startswith("water_") for n in sf.CORNERS.names[sf.LATE_CORNERS:sf.WATER_CORNERS])


@pytest.fixture(scope="module")
def late(oracle):
    """late_shares() of every seed of the slice and of every corner, computed once: (cases by name, shares by name)"""
    cases = {c["name"]: c for c in [sf.case(seed) for seed in SEEDS] + list(sf.CORNERS)}
    return cases, {name: sf.late_shares(c, {}) for name, c in cases.items()}


def test_every_late_pass_value_and_mutation_occurs(late):
    cases, _ = late
    seeds = [cases[f"seed{s}"] for s in SEEDS]
    for p in sf.LATE_PASSES:                                  # measured: mips 27, viewshed 37, cumulative 40, exposure 32, haze 36 of 48
        assert sum(p in c["late"]["on"] for c in seeds) >= len(seeds) / 3.0, p
    assert all(len(c["late"]["on"]) >= 2 for c in seeds) and all(c["late"]["on"] == sf.LATE_PASSES for c in sf.CORNERS)
    L = [c["late"] for c in seeds]
    assert {v["max_anisotropy"] for v in L} == set(sf.ANISOTROPIES) and {v["mip_bias"] for v in L} == set(sf.MIP_BIASES)
    assert {v["supersample"] for v in L} == set(sf.FACTORS)
    assert {len(v["cumulative"]["observers"]) for v in L} == set(sf.OBSERVER_COUNTS) and {len(v["exposure"]["suns"]) for v in L} == set(sf.SUN_COUNTS)
    assert {v["cumulative"]["batch"] for v in L} == set(sf.OBSERVER_BATCHES) and {v["exposure"]["batch"] for v in L} == set(sf.SUN_BATCHES)
    draped = [c for c in seeds if c["drape"] is not None]     # mips on in about two thirds of the draped seeds (the draw gives it 2 in 3; measured 23 of 42)
    assert 0.5 * len(draped) <= sum("mips" in c["late"]["on"] for c in draped) <= 0.85 * len(draped)
    alphas = {v[p][k][3] for v in L for p, k in (("viewshed", "visible_rgba"), ("viewshed", "hidden_rgba"), ("cumulative", "high_rgba"), ("exposure", "low_rgba"))}
    assert {0, 255} <= alphas
    for c in seeds:                                           # the factor respects the C ABI's limit and the cost cap
        f = c["late"]["supersample"]
        assert f * max(c["W"], c["H"]) <= 16384 and (f == 1 or f * f * c["W"] * c["H"] <= sf.SAMPLE_CAP)
    assert all(sf.CORNERS.named(n)["late"]["supersample"] == 1 for n in ("frame16384x24", "frame24x16384"))
    kinds = collections.Counter(c["late_mutation"] for c in cases.values())
    assert all(kinds[k] >= 2 for k in sf.LATE_MUTATIONS), kinds       # (measured: the rarest, mips_off and suns_reweight, 3 times each)
    for c in cases.values():                                  # the pass a mutation touches is on
        assert sf._NEEDS.get(c["late_mutation"], c["late"]["on"][0]) in c["late"]["on"], c["name"]
        one = c["late"]["exposure"]["suns"]
        assert len(one) == 1 or (one[:, 1] <= 0).any() or c["name"].startswith("late_")      # one sun below the horizon


def test_the_late_passes_write_part_of_what_they_cover(late):
    """conditions on the draw (soak_features._late, and _build's defaults for the corners): the draw is what to tune, not a bound"""
    _, stat = late
    print("\n" + sf.describe_late(list(stat.values())))
    for p in sf.LATE_PASSES:
        ch = [s["changed"][p] for s in stat.values() if s["changed"].get(p) is not None]
        # measured: changes a pixel in 46 / 62 (mips), 55 / 74 (viewshed), 67 / 77, 63 / 68, 72 / 72; 10-90 % in 28, 27, 27, 26 and 32 of them
        assert len(ch) >= 40 and sum(v > 0 for v in ch) >= 0.5 * len(ch), (p, ch)
        assert sum(0.1 < v < 0.9 for v in ch) >= 0.25 * len(ch), (p, sum(0.1 < v < 0.9 for v in ch), len(ch))
    mixed = [s["field_mixed"] for s in stat.values() if s["field_mixed"] is not None]
    assert sum(mixed) >= 0.5 * len(mixed), (sum(mixed), len(mixed))                           # measured 63 of 84
    partial = [s["haze_partial"] for s in stat.values() if s["haze_partial"] is not None]
    assert sum(partial) >= 0.5 * len(partial), (sum(partial), len(partial))                   # measured 68 of 83
    lod = [s["lod_above_0"] for s in stat.values() if s["lod_above_0"] is not None]
    assert sum(lod) >= len(lod) / 3.0, (sum(lod), len(lod))                                   # measured 37 of 53
    taps = [s["many_taps"] for s in stat.values() if s["many_taps"] is not None]
    assert sum(taps) >= 0.25 * len(taps), (sum(taps), len(taps))                              # measured 41 of 42


def test_a_late_mutation_shows_unless_it_must_not(late):
    """The same observer vertex and the same observers in another order leave every pixel as it was, in every case: that is the point
    of them.  Every other late mutation changes the frame behind the late passes (under the overlays, whose older draw may cover
    anything) in every case, seed or corner, that covers a pixel when the mutation comes -- after the case's first mutation, as
    run_case applies it.  The one rule of exception, counted here: no pixel covered then, so no terrain to show anything.  A failure
    is settled in soak_features._late (can_show), never here."""
    cases, stat = late
    same = [n for n, c in cases.items() if c["late_mutation"] in ("observer_same_vertex", "cumulative_reorder")]
    assert len(same) >= 8 and not any(stat[n]["mutation_shows"] for n in same)       # (22 such cases)
    for n in same:                                            # (and the mutation is one: the arguments differ)
        c = cases[n]
        a, b = (sf.lated(c, sf.initial_state(c)), sf.late_mutated(c, sf.lated(c, sf.initial_state(c))))
        assert sf.ssm._key(a["late"]) != sf.ssm._key(b["late"]), n
    rest = [n for n in cases if n not in same]
    blank = [n for n in rest if stat[n]["covered_before_late_mutation"] == 0]
    print(f"\n{len(same)} cases whose late mutation must not show, {len(rest)} whose must, of which {len(blank)} cover no pixel then: {blank}")
    assert len(blank) <= 12 and len(rest) - len(blank) >= 60  # measured: 9 of 73 (eight seeds and the sky camera's corner)
    assert [n for n in rest if n not in blank and not stat[n]["mutation_shows"]] == []
    shown = {cases[n]["late_mutation"] for n in rest if n not in blank}
    assert shown == set(sf.LATE_MUTATIONS) - {"observer_same_vertex", "cumulative_reorder"}, shown


def late_state(name):
    c = sf.CORNERS.named(name)
    state = sf.lated(c, sf.featured(c, sf.initial_state(c)))
    return c, state, sf.expected(c, state)


def test_the_late_corners_hold_the_edges_they_are_named_for(oracle):
    by = {c["name"]: c for c in sf.CORNERS}
    assert sf.LATE_CORNERS - sf.OLD_CORNERS == 18 and all(n.startswith("late_") for n in sf.CORNERS.names[sf.OLD_CORNERS:sf.LATE_CORNERS])
    # grid 2, the observer on a corner vertex; grid 3, 33 observers on at most 9 vertices
    c = by["late_grid2_observer_on_a_corner_vertex"]
    assert c["grid"] == 2 and sf.snap(c, c["late"]["viewshed"]["observer"]) == (0, 0)
    c = by["late_grid3_thirty_three_observers"]
    obs = c["late"]["cumulative"]["observers"]
    assert c["grid"] == 3 and len(obs) == 33 and len({sf.snap(c, o) for o in obs}) <= 9 and c["late_mutation"] == "cumulative_reorder"
    # an all-NaN texture: every field is 1, the count is N, the exposure the sum of the weights
    c, state, e = late_state("late_all_nan_texture")
    st, X = e["stages"], c["late"]["exposure"]
    assert np.isnan(c["heights"]).all() and (st["viewshed_field"] == 1).all() and (st["cumulative_field"] == len(c["late"]["cumulative"]["observers"])).all()
    wtot = sf.sem.weight_total(X["suns"], X["weights"])
    assert wtot > 0 and not X["incidence"] and (st["exposure_field"] == wtot).all()
    # the observer on the one texel's NaN vertex
    c, state, e = late_state("late_observer_on_the_nan_vertex")
    i, j = e["stages"]["viewshed_vertex"]
    assert int(np.isnan(c["heights"]).sum()) == 1 and np.isnan(sf.shm.heights(state["u"], c["heights"], c["grid"])[j, i])
    assert any(np.isnan(sf.shm.heights(state["u"], c["heights"], c["grid"])[v[1], v[0]]) for v in (sf.snap(c, o) for o in c["late"]["cumulative"]["observers"]))
    c = by["late_exaggeration0_eye_height0"]
    assert c["exaggeration"] == 0.0 and c["late"]["viewshed"]["eye_height"] == 0.0 and c["late"]["cumulative"]["eye_height"] == 0.0
    assert by["late_exaggeration_minus2"]["exaggeration"] == -2.0
    # the frames one pixel wide and one pixel high cover terrain, and every tint and the haze write covered pixels in them
    for name, size in (("late_frame_of_one_column", (1, 70)), ("late_frame_of_one_row", (130, 1))):
        c, state, e = late_state(name)
        st, cov = e["stages"], e["vis"] != 0
        assert (c["W"], c["H"]) == size and cov.sum() >= 30 and not cov.all()               # (32 of 70 and 99 of 130 pixels)
        wrote = {p: int(((st[p + "_frame"] != before).any(axis=2) & cov).sum())
                 for p, before in (("exposure", e["draped"]), ("cumulative", st["exposure_frame"]), ("viewshed", st["cumulative_frame"]), ("haze", st["viewshed_frame"]))}
        print(f"\n{name}: {int(cov.sum())} covered pixels, written by " + ", ".join(f"{p}: {k}" for p, k in wrote.items()))
        assert all(k >= 5 for k in wrote.values()), (name, wrote)
        assert ((e["draped"] != sf.expected(c, dict(state, late=None))["draped"]).any(axis=2) & cov).any()      # (and the mips move draped pixels)
    # the sky camera covers no pixel, and the haze writes the background
    c, state, e = late_state("late_sky_camera_haze_on_the_background")
    assert not e["vis"].any() and c["late"]["haze"]["background"] and (e["late"] != e["rgba"]).any(axis=2).all()
    assert (e["haze_opacity"] == np.float32(c["late"]["haze"]["max_opacity"]) * np.float32(c["late"]["haze"]["rgba"][3]) / np.float32(255)).all()
    # every sun below the horizon (or on it): no weight, no exposure
    c, state, e = late_state("late_every_sun_below_the_horizon")
    X = c["late"]["exposure"]
    assert (X["suns"][:, 1] <= 0).all() and sf.sem.weight_total(X["suns"], X["weights"]) == 0 and not e["stages"]["exposure_field"].any()
    # a radius below one cell leaves the observer's vertex alone in range
    c, state, e = late_state("late_radius_below_one_cell")
    n = max(c["grid"], 2)
    for r, o in [(c["late"]["viewshed"]["radius"], c["late"]["viewshed"]["observer"])] + [(c["late"]["cumulative"]["radius"], o) for o in c["late"]["cumulative"]["observers"]]:
        assert int(sf.cvm.in_range(n, sf.snap(c, o), sf.cvm.rc(r, c["spacing"], n)).sum()) == 1
    assert e["stages"]["cumulative_field"].max() <= len(c["late"]["cumulative"]["observers"]) and (e["stages"]["cumulative_field"] > 0).sum() <= len(c["late"]["cumulative"]["observers"])
    # a 1 x 1 drape has no pyramid
    c = by["late_drape_1x1_mips_on"]
    assert c["drape"]["image"].shape[:2] == (1, 1) and len(sf.dmm.sizes(1, 1)) == 1 and "mips" in c["late"]["on"]
    # bias -16 samples level 0 everywhere, bias 16 the coarsest level
    for name, bias in (("late_dense_drape_bias_minus16", -16.0), ("late_dense_drape_bias_16", 16.0)):
        c, state, e = late_state(name)
        lod = e["stages"]["drape_sample"][e["drape_mask"]][:, 6]
        top = len(sf.dmm.sizes(300, 300)) - 1
        assert c["drape"]["image"].shape[:2] == (300, 300) and (c["W"], c["H"]) == (15, 17) and c["late"]["mip_bias"] == bias and len(lod) >= 30       # (32 of the 41 covered pixels)
        assert (lod <= 0).all() if bias < 0 else (lod >= top).all()
    # the grazing camera takes sixteen taps somewhere
    c, state, e = late_state("late_anisotropy16_grazing_camera")
    assert c["late"]["max_anisotropy"] == 16 and e["stages"]["drape_sample"][e["drape_mask"]][:, 7].max() == 16
    assert by["late_supersample4_frame1x1"]["late"]["supersample"] == 4 and (by["late_supersample4_frame1x1"]["W"], by["late_supersample4_frame1x1"]["H"]) == (1, 1)
    assert by["late_supersample3_frame15x17"]["late"]["supersample"] == 3 and (by["late_supersample3_frame15x17"]["W"], by["late_supersample3_frame15x17"]["H"]) == (15, 17)


def test_the_late_near_plane_corner_tints_and_hazes_clipped_triangles(oracle):
    c, state, e = late_state("late_near_plane_through_the_terrain")
    st, vis = e["stages"], e["vis"]
    cut = near_plane_straddlers(c, state["u"])
    straddling = np.zeros(vis.shape, bool)
    straddling[vis != 0] = cut[vis[vis != 0] - 1]
    tinted = {p: (st[p + "_frame"] != before).any(axis=2) & straddling
              for p, before in (("exposure", e["draped"]), ("cumulative", st["exposure_frame"]), ("viewshed", st["cumulative_frame"]), ("haze", st["viewshed_frame"]))}
    print("\n" + ", ".join(f"{p}: {int(m.sum())}" for p, m in tinted.items()) + " pixels written on triangles the near plane cuts")
    assert all(m.sum() >= 50 for m in tinted.values())


def expected_keeps_the_late_passes_apart():
    """(of test_expected_is_deterministic) a cached entry made without a late pass is never returned for a state with it, and the
    other way round; one with another pass off neither"""
    c, cache = sf.CORNERS.named("late_supersample3_frame15x17"), {}
    state = sf.featured(c, sf.initial_state(c), overlays=True)
    bare = sf.expected(c, state, cache)
    full = sf.expected(c, sf.lated(c, state), cache)
    assert (full["frame"] != bare["frame"]).any() and np.array_equal(sf.expected(c, state, cache)["frame"], bare["frame"])
    assert full["frame"].tobytes() == sf.expected(c, sf.lated(c, state))["frame"].tobytes()
    seen = {full["late"].tobytes()}
    for p in sf.LATE_PASSES[1:]:                              # each pass off in turn: another frame each time
        s = sf.lated(c, state)
        s["late"][p] = None
        seen.add(sf.expected(c, s, cache)["late"].tobytes())
    assert len(seen) == 5
    ss = sf.expected_supersampled(c, sf.lated(c, state), 3, cache)
    assert ss["samples"].shape == (51, 45, 4) and ss["frame"].shape == (17, 15, 4) and np.array_equal(sf.ssm.resolve(ss["samples"], 3), ss["resolved"])


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


# ---- the flood and the spill ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def water(oracle):
    """water_shares() of every seed of the slice and of every corner, computed once: (cases by name, shares by name)"""
    cases = {c["name"]: c for c in [sf.case(seed) for seed in SEEDS] + list(sf.CORNERS)}
    return cases, {name: sf.water_shares(c, {}) for name, c in cases.items()}


def seed_lists(c):
    """the seed lists of a case's two passes: {pass: (N, 2) array}"""
    return {p: c["water"][p]["seeds"] for p in sf.WATER_PASSES if isinstance(c["water"][p]["seeds"], np.ndarray)}


def test_every_water_value_and_mutation_occurs(water):
    cases, stat = water
    seeds = [cases[f"seed{s}"] for s in SEEDS]
    every = list(cases.values())
    for c in seeds:
        assert c["water"]["on"] and set(c["water"]["on"]) <= set(sf.WATER_PASSES), c["name"]
    assert all(c["water"]["on"] == sf.WATER_PASSES for c in sf.CORNERS)
    for p in sf.WATER_PASSES:                                 # measured: flood on in 36, spill in 41 of 48
        assert sum(p in c["water"]["on"] for c in seeds) >= 24, p
    assert {sf.flood_mode(c["water"]["flood"]) for c in every if "flood" in c["water"]["on"]} == set(sf.FLOOD_MODES)
    assert {sf.spill_mode(c["water"]["spill"]) for c in every if "spill" in c["water"]["on"]} == set(sf.SPILL_MODES)
    assert {c["water"]["level_kind"] for c in seeds} == set(sf.LEVEL_KINDS)
    for c in every:                                           # the level kinds are what they say
        surf = sf.cm.surface(c["heights"], c["grid"])
        fin, level = surf[np.isfinite(surf)], np.float32(c["water"]["flood"]["level"])
        kind = c["water"]["level_kind"]
        assert np.isfinite(level) and (kind != "vertex" or (fin.view(np.uint32) == level.view(np.uint32)).any()), c["name"]
        assert (kind != "below" or level < fin.min()) and (kind != "above" or level > fin.max()), c["name"]
    for p in sf.WATER_PASSES:
        lists = [seed_lists(c)[p] for c in every if p in seed_lists(c) and p in c["water"]["on"]]
        assert {len(s) for s in lists} == set(sf.SEED_COUNTS), (p, sorted({len(s) for s in lists}))
        for s in lists:                                       # one duplicate in every list of three and more
            assert len(s) < 3 or len({tuple(v) for v in s.tolist()}) < len(s)
    for c in every:
        sp, surf = c["spacing"], sf.cm.surface(c["heights"], c["grid"])
        for p, s in seed_lists(c).items():
            assert np.isfinite(s).all() and (np.abs(s) <= 1.9 * sp + 1e-6).all(), (c["name"], p)
    # seeds beyond the grid (they clamp to the border), on a vertex without a height, and for the flood on a dry vertex
    def drawn(c, p):
        """the pass is on and takes a seed list that the draw made (no corner wrote it down)"""
        if p not in seed_lists(c) or p not in c["water"]["on"]:
            return False
        return c["name"].startswith("seed") or "seeds" not in sf._SPECS[sf.CORNERS.names.index(c["name"])][2].get("water", {}).get(p, {})

    beyond = on_nan = on_dry = 0
    for c in every:
        surf = sf.cm.surface(c["heights"], c["grid"])
        for p in sf.WATER_PASSES:
            if not drawn(c, p):
                continue
            s = seed_lists(c)[p]
            v = sf.seed_vertices(c, s)
            beyond += bool((np.abs(s) > 1.5 * c["spacing"]).any())
            there = ~np.isfinite(surf[v[:, 1], v[:, 0]])
            on_nan += bool(there.any())
            if len(s) > 3 and not np.isfinite(surf).all():
                assert there.any(), (c["name"], p)            # (a long list always has one where there is such a vertex)
            if p == "flood":
                dry = ~(surf[v[:, 1], v[:, 0]] < np.float32(c["water"]["flood"]["level"]))
                on_dry += bool(dry.any())
                if len(s) > 3 and not (surf < np.float32(c["water"]["flood"]["level"])).all():
                    assert dry.any(), c["name"]                # (a long list always has one where there is a dry vertex)
    print(f"\nseed lists with a seed beyond the grid: {beyond}, on a vertex without a height: {on_nan}, flood lists with a seed on a dry vertex: {on_dry}")
    assert beyond >= 20 and on_nan >= 3 and on_dry >= 5
    assert {c["water"]["flood_group"] for c in seeds} == set(sf.WATER_GROUPS) and {c["water"]["spill_group"] for c in seeds} == set(sf.WATER_GROUPS)
    assert {c["water"]["spill_flags"] for c in seeds} == {True, False}
    assert {(c["water"]["spill_group"] == 0, c["water"]["spill_flags"]) for c in seeds} == {(a, b) for a in (True, False) for b in (True, False)}
    over = [c["water"]["depth_full_over_range"] for c in seeds]
    assert {v[0] for v in over} == set(sf.DEPTH_FULLS) and {v[1] for v in over} == set(sf.DEPTH_FULLS)
    alphas = [(c["water"][p]["shallow_rgba"][3], c["water"][p]["deep_rgba"][3]) for c in seeds for p in sf.WATER_PASSES]
    assert any(a == 0 for a, _ in alphas) and any(b == 0 for _, b in alphas) and not any(a == 0 and b == 0 for a, b in alphas)
    # a coverage strictly between 0 and 1 (a blended pixel's depth between 0 and depth_full) occurs under both tints, in many cases
    for p in sf.WATER_PASSES:
        part = [s["partial"][p] for s in stat.values() if p in s["partial"]]
        assert sum(part) >= 20, (p, sum(part), len(part))
    kinds = collections.Counter(c["water_mutation"] for c in every)
    assert all(kinds[k] >= 2 for k in sf.WATER_MUTATIONS), kinds
    assert sum(kinds[k] for k in sf.WATER_MUTATIONS if k != "heights_water") >= 0.6 * len(every), kinds     # (heights_water is what a case falls back to)
    for c in every:                                           # the pass a mutation touches is on, and a seed mutation has a list to move
        assert sf._WATER_NEEDS.get(c["water_mutation"], c["water"]["on"][0]) in c["water"]["on"], c["name"]
        if c["water_mutation"] in ("seeds_move", "seeds_nudged"):
            assert any(p in c["water"]["on"] for p in seed_lists(c)), c["name"]
    # the flood identity of DESIGN.md 4t, wherever the flood has sources of its own: flooded == reached & (spill < level)
    assert all(s["identity"] for s in stat.values() if s["identity"] is not None) and sum(s["identity"] is not None for s in stat.values()) >= 60


def test_the_water_writes_part_of_what_it_covers(water):
    """conditions on the draw (soak_features._water), over the 48 seeds, from the reference alone: the draw is what to tune, not a floor"""
    cases, stat = water
    seeds = [stat[f"seed{s}"] for s in SEEDS]
    print("\n" + sf.describe_water(seeds) + "\nwith the corners: " + sf.describe_water(list(stat.values())))
    listed = [s for s in seeds if "flood" in s["on"] and s["flood_mode"] != "everywhere"]
    assert sum(s["proper"] for s in listed) >= len(listed) / 3.0, (sum(s["proper"] for s in listed), len(listed))          # measured 9 of 25
    spilt = [s for s in seeds if "spill" in s["on"]]
    assert sum(s["sinks"] for s in spilt) >= 0.5 * len(spilt), (sum(s["sinks"] for s in spilt), len(spilt))                 # measured 31 of 41
    for p in sf.WATER_PASSES:                                 # measured: the flood 19 and 11 of 29, the spill 24 and 16 of 35
        ch = [s["changed"][p] for s in seeds if s["changed"].get(p) is not None]
        assert len(ch) >= 20 and sum(v > 0 for v in ch) >= 0.5 * len(ch), (p, ch)
        assert sum(0.1 < v < 0.9 for v in ch) >= 0.2 * len(ch), (p, ch)


def test_a_water_mutation_shows_unless_it_must_not(water):
    """seeds_nudged leaves every pixel as it was, in every case: that is the point of it; and after a water_colours_only whose
    colours are all transparent the frame is the one without either pass.  Every other water mutation -- spill_cleared while the
    spill is away -- changes the frame behind the water (under the late passes, which may be opaque, and the overlays) in every
    case, seed or corner, that covers a pixel when the mutation comes, after the first and the late mutation, as run_case applies
    it.  The one rule of exception, counted here: no pixel covered then.  The generator (soak_features._water, can_show) asks the
    two models which vertices get another tint and its own arithmetic which of them the camera has in view; a failure is settled
    there, never here."""
    cases, stat = water
    same = [n for n, c in cases.items() if c["water_mutation"] == "seeds_nudged"]
    assert len(same) >= 6 and not any(stat[n]["mutation_shows"] or stat[n]["mutation_shows_behind_the_late_passes"] for n in same)
    for n in same:                                            # (and the mutation is one: the numbers differ, the vertices do not)
        c = cases[n]
        moved = [p for p in seed_lists(c) if p in c["water"]["on"] and c["water_mutation_args"]["nudged"][p].tobytes() != c["water"][p]["seeds"].tobytes()]
        assert moved, n
        for p in moved:
            assert np.array_equal(sf.seed_vertices(c, c["water_mutation_args"]["nudged"][p]), sf.seed_vertices(c, c["water"][p]["seeds"])), n
    clear = [n for n, c in cases.items() if c["water_mutation"] == "water_colours_only" and c["water_mutation_args"]["transparent"]]
    assert len(clear) >= 1 and all(stat[n]["without_water"] for n in clear), clear
    rest = [n for n in cases if n not in same]
    blank = [n for n in rest if stat[n]["covered_before_the_mutation"] == 0]
    hidden = [n for n in rest if n not in blank and not stat[n]["mutation_shows"]]
    print(f"\n{len(same)} cases whose water mutation must not show, {len(rest)} whose must, of which {len(blank)} cover no pixel then: {blank}; "
          f"{len(hidden)} cover pixels and show nothing: {[(n, cases[n]['water_mutation'], stat[n]['covered_before_the_mutation']) for n in hidden]}")
    assert len(rest) - len(blank) >= 80
    assert hidden == []
    shown = {cases[n]["water_mutation"] for n in rest if n not in blank and n not in hidden}
    assert shown == set(sf.WATER_MUTATIONS) - {"seeds_nudged"}, shown
    final = [n for n in rest if stat[n]["mutation_shows_behind_the_late_passes"]]
    assert len(final) >= 0.8 * (len(rest) - len(blank) - len(hidden)), len(final)            # (the late passes seldom hide it)


def test_the_generators_projection_is_the_uniform_blocks(oracle):
    """soak_features.projection, which tells the water's generator what the camera has in view, against the uniform block"""
    for c in [sf.case(seed) for seed in list(SEEDS)[:12]] + [sf.CORNERS.named("water_near_plane_through_the_terrain"), sf.CORNERS.named("frame16384x24")]:
        P = sf.uniforms(c)[16:32].reshape(4, 4).T
        sx, sy, A, B, C, D = sf.projection(c)
        want = np.array([[sx, 0, 0, 0], [0, sy, 0, 0], [0, 0, A, B], [0, 0, C, D]])
        assert np.allclose(P, want, rtol=1e-5, atol=1e-6), (c["name"], P, want)


def water_state(name):
    c = sf.CORNERS.named(name)
    state = sf.watered(c, sf.lated(c, sf.featured(c, sf.initial_state(c))))
    return c, state, sf.expected(c, state)


def test_the_water_corners_hold_the_edges_they_are_named_for(oracle):
    by = {c["name"]: c for c in sf.CORNERS}
    fields = lambda c: (sf.cm.surface(c["heights"], c["grid"]), sf.flood_of(c, sf.cm.surface(c["heights"], c["grid"]), c["water"]["flood"]),
                        sf.spill_of(c, sf.cm.surface(c["heights"], c["grid"]), c["water"]["spill"]))
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    # grid 2: all border, both passes from it; the highest vertex's height is the level
    c = by["water_grid2_all_border"]
    surf, F, S = fields(c)
    assert c["grid"] == 2 and surf.shape == (2, 2) and sf.flood_mode(c["water"]["flood"]) == "edges" and sf.spill_mode(c["water"]["spill"]) == "edges"
    assert 1 <= F.flooded.sum() < 4 and np.array_equal(F.flooded, F.wet) and S.reached.all() and not S.sink.any()
    # grid 3: from the lowest corner, the centre's height is the level exactly, so it stays dry
    c = by["water_grid3_centre_at_the_level"]
    surf, F, S = fields(c)
    assert c["grid"] == 3 and bits(c["water"]["flood"]["level"]) == bits(surf[1, 1]) and not F.wet[1, 1] and not F.flooded[1, 1] and F.flooded.any()
    v = sf.seed_vertices(c, c["water"]["flood"]["seeds"]).tolist()
    assert len(v) == 1 and v[0][0] in (0, 2) and v[0][1] in (0, 2) and F.flooded[v[0][1], v[0][0]]
    # grids 63 and 64 in white noise: sinks by the thousand
    for name, grid in (("water_grid63_white_noise", 63), ("water_grid64_white_noise", 64)):
        c = by[name]
        surf, F, S = fields(c)
        print(f"\n{name}: {int((S.sink > 0).sum())} sink vertices, {int(F.flooded.sum())} flooded of {int(F.wet.sum())} wet-able")
        assert c["grid"] == grid and not c["smooth"] and c["amp"] == 3.0 and (S.sink > 0).sum() >= 1000 and F.flooded.any() and (F.wet & ~F.flooded).any()
    # grid 130 from one seed: both fields need more than two tile passes, and tiles rest while others run
    c = by["water_grid130_white_noise_from_one_seed"]
    surf, F, S = fields(c)
    assert c["grid"] == 130 and len(c["water"]["flood"]["seeds"]) == 1 and len(c["water"]["spill"]["seeds"]) == 1
    _, passes = sf.fdm.tile_passes(F.wet, sf.fdm.sources(F.wet, F.vertices))
    _, spill_passes, changed = sf.spm.tile_passes(surf, S.vertices)
    print(f"\ngrid 130 from one seed: the flood takes {passes} tile passes, the spill {spill_passes}, changing {changed.tolist()} of 9 tiles")
    assert passes >= 3 and spill_passes >= 3 and (changed[:spill_passes - 1] < 9).any() and F.flooded.sum() > 1000 and S.reached.all() and (S.sink > 0).sum() >= 1000
    assert sf.fdm.tiles_reached(F.flooded)[0] >= 4
    a = c["water_mutation_args"]["moved"]
    assert c["water_mutation"] == "seeds_move" and all(sf.seed_vertices(c, a[p]).tolist() != sf.seed_vertices(c, c["water"][p]["seeds"]).tolist() for p in sf.WATER_PASSES)
    assert (c["water"]["flood_group"], c["water"]["spill_group"], c["water"]["spill_flags"]) == (1, 7, False)
    # the all-NaN texture: nothing wet-able or passable, the frame unchanged; the heights mutation brings ground
    c, state, e = water_state("water_all_nan_texture")
    surf, F, S = fields(c)
    assert np.isnan(c["heights"]).all() and not F.wet.any() and not F.flooded.any() and not S.reached.any() and np.isposinf(S.spill).all() and not S.sink.any()
    assert np.array_equal(sf.behind_the_water(e), e["draped"]) and c["mutation"] == "heights"
    s1 = sf.cm.surface(c["mutation_args"]["heights"], c["grid"])
    assert sf.flood_of(c, s1, c["water"]["flood"]).flooded.any() and sf.spill_of(c, s1, c["water"]["spill"]).reached.all()
    # the only seed on the one texel's vertices without a height: no source; heights_water brings one
    c, state, e = water_state("water_only_seed_on_the_nan_vertex")
    surf, F, S = fields(c)
    assert int(np.isnan(c["heights"]).sum()) == 1 and np.isfinite(surf).sum() > 1000
    for p, M in (("flood", F), ("spill", S)):
        v = sf.seed_vertices(c, c["water"][p]["seeds"]).tolist()
        assert len(v) == 1 and np.isnan(surf[v[0][1], v[0][0]]), p
    assert F.wet.any() and not F.flooded.any() and not S.reached.any() and np.array_equal(sf.behind_the_water(e), e["draped"])
    assert c["water_mutation"] == "heights_water" and c["mutation"] != "heights" and c["late_mutation"] != "heights_again"
    s1 = sf.cm.surface(c["water_mutation_args"]["heights"], c["grid"])
    assert np.isfinite(s1).all() and sf.spill_of(c, s1, c["water"]["spill"]).reached.all() and sf.flood_of(c, s1, c["water"]["flood"]).flooded.any()
    # the plateau: nine consecutive binary32 heights; the level is the middle one and ties with a whole plateau, which stays dry;
    # from the seed on the highest plateau the ties hold sinks, from the border they hold none
    c = by["water_plateau_of_ties"]
    surf, F, S = fields(c)
    values = np.unique(surf)
    level = np.float32(c["water"]["flood"]["level"])
    assert len(values) == 9 and (np.diff(values.view(np.uint32).astype(np.int64)) == 1).all() and level == values[4]
    assert (surf == level).sum() > 20 and not F.wet[surf == level].any() and F.flooded.any()
    v = sf.seed_vertices(c, c["water"]["spill"]["seeds"]).tolist()
    assert len(v) == 1 and surf[v[0][1], v[0][0]] == values[-1] and (S.sink > 0).sum() > 20 and S.reached.all()
    assert not sf.spm.field_heights(surf, "edges").sink.any() and c["water_mutation"] == "spill_mode" and c["water_mutation_args"]["spill_seeds"] == "edges"
    # the bridge: the channel's middle vertex is at the level exactly and dry, so the water from the one end stops in front of it; one
    # binary32 step more (what `<=` would make of it) floods the whole channel -- other bits in the field, other pixels in the frame
    c, state, e = water_state("water_bridge_vertex_at_the_level")
    surf, F, S = fields(c)
    level = np.float32(c["water"]["flood"]["level"])
    assert c["grid"] == 9 and bits(level) == bits(surf[4, 4]) and (surf[4, 1:4] < level).all() and (surf[4, 5:8] < level).all() and (np.delete(surf, 4, axis=0) > level).all()
    assert F.flooded[4, 1:4].all() and int(F.flooded.sum()) == 3 and F.wet[4, 5:8].all() and not F.wet[4, 4] and int(F.wet.sum()) == 6
    over = sf.flood_of(c, surf, dict(c["water"]["flood"], level=float(np.nextafter(level, np.float32(np.inf)))))
    assert int(over.flooded.sum()) == 7 and (over.depth[4, 5:8] > 0).all() and not F.depth[4, 5:8].any()
    wrong = sf.fdm.frame(e["draped"], e["vis"], state["u"], state["heights"], c["grid"], over, **{k: c["water"]["flood"][k] for k in ("shallow_rgba", "deep_rgba", "depth_full")})[0]
    print(f"\nthe bridge: {int((e['stages']['flood_frame'] != e['draped']).any(axis=2).sum())} pixels under water, {int((wrong != e['stages']['flood_frame']).any(axis=2).sum())} more with the bridge wet")
    assert (e["stages"]["flood_frame"] != e["draped"]).any() and (wrong != e["stages"]["flood_frame"]).any(axis=2).sum() >= 20
    full = sf.watered(c, sf.lated(c, sf.featured(c, sf.initial_state(c), overlays=True)))           # (and under the late passes and the overlays)
    wet = dict(full, water=dict(full["water"], flood=dict(full["water"]["flood"], level=float(np.nextafter(level, np.float32(np.inf))))))
    assert (sf.expected(c, wet)["frame"] != sf.expected(c, full)["frame"]).any(axis=2).sum() >= 20
    # the level above and below everything, in each mode
    for m in sf.FLOOD_MODES:
        c = by[f"water_level_above_everything_{m}"]
        surf, F, S = fields(c)
        assert sf.flood_mode(c["water"]["flood"]) == m and F.wet.all() and (F.flooded.all() or m == "seeds") and F.flooded.any()
        c = by[f"water_level_below_everything_{m}"]
        surf, F, S = fields(c)
        assert sf.flood_mode(c["water"]["flood"]) == m and not F.wet.any() and not F.flooded.any()
    # exaggeration 0, then -2: neither field knows it
    c = by["water_exaggeration0_then_minus2"]
    assert c["exaggeration"] == 0.0 and c["mutation"] == "exaggeration" and c["mutation_args"]["exaggeration"] == -2.0
    assert "exaggeration" not in sf.STALE_FLOOD + sf.STALE_SPILL
    # the frames of one pixel, one column and one row cover terrain, and both tints write covered pixels of the column and the row
    for name, size in (("water_frame1x1", (1, 1)), ("water_frame_of_one_column", (1, 70)), ("water_frame_of_one_row", (130, 1))):
        c, state, e = water_state(name)
        st, cov = e["stages"], e["vis"] != 0
        wrote = {"flood": int(((st["flood_frame"] != e["draped"]).any(axis=2) & cov).sum()), "spill": int(((st["spill_frame"] != st["flood_frame"]).any(axis=2) & cov).sum())}
        print(f"\n{name}: {int(cov.sum())} covered pixels, written by " + ", ".join(f"{p}: {k}" for p, k in wrote.items()))
        assert (c["W"], c["H"]) == size and cov.any() and wrote["flood"] >= 1
        assert size == (1, 1) or (wrote["flood"] >= 5 and wrote["spill"] >= 1 and not cov.all())
    c = by["water_supersample3_frame15x17"]
    assert c["late"]["supersample"] == 3 and (c["W"], c["H"]) == (15, 17) and c["water"]["on"] == sf.WATER_PASSES


def test_the_water_near_plane_corner_tints_clipped_triangles(oracle):
    c, state, e = water_state("water_near_plane_through_the_terrain")
    st, vis = e["stages"], e["vis"]
    cut = near_plane_straddlers(c, state["u"])
    straddling = np.zeros(vis.shape, bool)
    straddling[vis != 0] = cut[vis[vis != 0] - 1]
    tinted = {"flood": (st["flood_frame"] != e["draped"]).any(axis=2) & straddling, "spill": (st["spill_frame"] != st["flood_frame"]).any(axis=2) & straddling}
    print("\n" + ", ".join(f"{p}: {int(m.sum())}" for p, m in tinted.items()) + " pixels written on triangles the near plane cuts")
    assert all(m.sum() >= 50 for m in tinted.values())
    assert all((((st[p + "_frame"] != before).any(axis=2)) & ~straddling).any() for p, before in (("flood", e["draped"]), ("spill", st["flood_frame"])))


def test_the_chain_keeps_the_water_apart_and_its_fields_without_the_exaggeration(oracle):
    """a cached entry made without a water pass is never returned for a state with it; the flood and spill fields are kept under a
    key without the exaggeration, so another exaggeration finds them, and another level or source does not"""
    c, cache = sf.CORNERS.named("water_exaggeration0_then_minus2"), {}
    state = sf.lated(c, sf.featured(c, sf.initial_state(c), overlays=True))
    bare = sf.expected(c, state, cache)
    full = sf.expected(c, sf.watered(c, state), cache)
    assert (full["late"] != bare["late"]).any() and np.array_equal(sf.expected(c, state, cache)["frame"], bare["frame"])
    assert full["frame"].tobytes() == sf.expected(c, sf.watered(c, state))["frame"].tobytes()
    seen = {full["late"].tobytes()}
    for p in sf.WATER_PASSES:
        s = sf.watered(c, state)
        s["water"][p] = None
        seen.add(sf.expected(c, s, cache)["late"].tobytes())
    assert len(seen) == 3
    after = sf.expected(c, sf.mutated(c, sf.watered(c, state)), cache)
    assert after["stages"]["flood_field"] is full["stages"]["flood_field"] and after["stages"]["spill_field"] is full["stages"]["spill_field"]
    deeper = sf.watered(c, state)
    deeper["water"]["flood"] = dict(deeper["water"]["flood"], level=deeper["water"]["flood"]["level"] + 0.25)
    assert sf.expected(c, deeper, cache)["stages"]["flood_field"] is not full["stages"]["flood_field"]
    # the order of the two: the spill's tint over the flood's water shows where a pixel takes both
    st = full["stages"]
    u, h, G, W = state["u"], state["heights"], c["grid"], c["water"]
    tint = lambda P: {k: P[k] for k in ("shallow_rgba", "deep_rgba", "depth_full")}
    other = sf.fdm.frame(sf.spm.frame(full["draped"], full["vis"], u, h, G, st["spill_field"], **tint(W["spill"]))[0], full["vis"], u, h, G, st["flood_field"], **tint(W["flood"]))[0]
    assert (other != st["spill_frame"]).any()


# ---- hazed overlay layers ------------------------------------------------------------------------------------------------

def test_no_key_older_than_the_hazed_layers_has_moved():
    """the digest of OLD_KEYS, the three late keys and WATER_KEYS of the slice's seeds and of the 68 corners older than the hazed
    layers, computed on the commit before their generator existed"""
    keys = sf.OLD_KEYS + ("late", "late_mutation", "late_mutation_args") + sf.WATER_KEYS
    assert sf.digest((sf.case(seed) for seed in SEEDS), keys) == "49c31bc9520d16792a9bf824fb8314eccff6c50a9431e46d998eabc362896c63"
    assert sf.digest((sf.CORNERS[i] for i in range(sf.WATER_CORNERS)), keys) == "c09a7566456a36ca4ff6f2c9f11d21671b2ab9ff3bf268464d2c05aa8efc8e50"
    assert sf.WATER_CORNERS == 68 and set(sf.case(FIRST_SEED)) == set(keys) | set(sf.HAZED_KEYS)
    assert not any(n.startswith("hazed_") for n in sf.CORNERS.names[:sf.WATER_CORNERS]) and all(n.startswith("hazed_") for n in sf.CORNERS.names[sf.WATER_CORNERS:])


@pytest.fixture(scope="module")
def hazed(oracle):
    """hazed_shares() of every seed of the slice and of every corner, computed once: (cases by name, shares by name)"""
    cases = {c["name"]: c for c in [sf.case(seed) for seed in SEEDS] + list(sf.CORNERS)}
    return cases, {name: sf.hazed_shares(c, {}) for name, c in cases.items()}


def everything_on(c, **hazed):
    return sf.hazed_on(c, sf.watered(c, sf.lated(c, sf.featured(c, sf.initial_state(c), overlays=True))), **hazed)


def test_without_a_flag_or_without_the_haze_the_frame_is_the_occlusion_models(oracle):
    """expected() composites through overlay_haze_model: with no flag set, or with haze=None, its bytes are occlusion_model.composite's
    over the same layers, the ladder among them -- on eight seeds and every corner"""
    for c in [sf.case(seed) for seed in list(SEEDS)[:8]] + list(sf.CORNERS):
        cache = {}
        for state in (everything_on(c, flags=False), sf.hazed_on(c, sf.featured(c, sf.initial_state(c), overlays=True)),
                      dict(everything_on(c), late=dict(everything_on(c)["late"], haze=None))):
            e = sf.expected(c, state, cache)
            assert len(e["layers"].ranges) == len(sf.eligible(c)) + 1            # (the ladder is there)
            assert np.array_equal(e["frame"], sf.ocm.composite(e["late"], e["vis"], state["u"], state["heights"], c["grid"], e["layers"])), (c["name"], state["hazed"])
        ss = dict(everything_on(c, flags=False))
        if c["late"]["supersample"] > 1 and c["W"] * c["H"] <= 4096:
            f = c["late"]["supersample"]
            e = sf.expected_supersampled(c, ss, f, cache)
            L = sf.layers(sf.unoccluded(c), dict(ss, occlusion={}))
            assert np.array_equal(e["frame"], sf.ssm.composite(e["resolved"], ss["u"], ss["heights"], c["grid"], L)), c["name"]


def test_the_slice_hazes_part_of_what_its_layers_cover(hazed):
    """conditions on the draw (soak_features._hazed: FLAG_SHARE, the ladder), over the 48 seeds with the drawn flags and the ladder,
    from the models alone: the draw is what to tune, never a bound"""
    cases, stat = hazed
    seeds = [stat[f"seed{s}"] for s in SEEDS]
    print("\n" + sf.describe_hazed(seeds) + "\nwith the corners: " + sf.describe_hazed(list(stat.values())))
    on = [s for s in seeds if s["haze_on"]]
    assert len(on) == 36
    assert sum(s["pairs"] > 0 for s in on) >= 30                                # measured 36 of 36
    assert sum(4 * s["middle"] >= s["pairs"] > 0 for s in on) >= 18             # measured 29
    assert sum(s["clear"] > 0 for s in on) >= 4                                 # measured 7
    assert sum(s["differs"] for s in on) >= 30                                  # measured 36
    for s in seeds:                                                             # (without the haze a flag changes no byte)
        assert s["haze_on"] or not (s["pairs"] or s["differs"])
    c48 = [cases[f"seed{s}"] for s in SEEDS]
    assert all(any(c["hazed"]["flags"]) and len(c["hazed"]["flags"]) == len(c["hazed"]["early"]) == len(sf.eligible(c)) == 6 for c in c48)
    assert set().union(*[s["kinds"] for s in seeds]) == {"circle", "square", "cap_butt", "cap_square", "cap_round", "contours"}
    assert sum(s["occluding"] for s in seeds) >= 8                              # measured 44 (a drawn layer; the ladder occludes in every other seed besides)
    assert sum(s["early_then_add"] for s in seeds) >= 12                        # measured 42
    assert sum(c["hazed"]["ladder"]["occlude"] for c in c48) == 24
    for c in cases.values():                                                    # the ladder: twelve opaque draped circles of 5 px from under the eye through the target
        lad = c["hazed"]["ladder"]
        assert lad["xyz"].shape == (sf.LADDER_RUNGS, 3) and lad["size_px"] == 5.0 and lad["rgba"][3] == 255 and lad["drape"] and lad["shape"] == "circle"
        g = lad["xyz"][:, [0, 2]].astype(np.float64)
        assert np.allclose(g[0], [c["eye"][0], c["eye"][2]], atol=1e-5) and np.isfinite(g).all()
        d, t = g[-1] - g[0], np.subtract([c["target"][0], c["target"][2]], g[0])
        assert abs(d[0] * t[1] - d[1] * t[0]) <= 1e-4 * max(1.0, float(np.abs(d).max()) * float(np.abs(t).max())), c["name"]     # (the target lies on its line)


def test_every_hazed_mutation_occurs_and_does_what_it_must(hazed):
    """flag_flip changes the frame in every case, seed or corner, whose flipped layer -- flagged alone, the terrain in front of it
    taken into account -- has a covered pixel with S.ah > 0 when the mutation comes; the cases without one are counted.
    flags_all_off leaves occlusion_model.composite's bytes over the same layers, polygon_refused the frame before it.  A failure is
    settled in soak_features._hazed (can_stand), never here."""
    cases, stat = hazed
    kinds = collections.Counter(cases[f"seed{s}"]["hazed_mutation"] for s in SEEDS)
    assert all(kinds[k] >= 3 for k in sf.HAZED_MUTATIONS), kinds               # measured: flag_flip 4, the others 8 to 10 of the 48 seeds
    for n, c in cases.items():
        kind, a, on = c["hazed_mutation"], c["hazed_mutation_args"], dict(zip(sf.eligible(c), c["hazed"]["flags"]))
        assert kind not in ("flag_flip", "haze_params") or stat[n]["haze_on"], n
        assert kind != "flag_flip" or a["layer"] in on, n
        if kind == "occlusion_on_hazed":                                        # a flagged point or line layer: a drawn one, or the ladder
            k = a["occlusion_layer"]
            assert k == sf.ladder_index(c) or (on[k] and c["overlays"][k][0] in ("points", "lines")), n
        if kind == "haze_params":                                               # another density, start and falloff
            Z = c["late"]["haze"]
            assert all(a["haze"][k] != Z[k] for k in ("density", "start", "falloff")) or n.startswith("hazed_"), n
    flips = [n for n, c in cases.items() if c["hazed_mutation"] == "flag_flip"]
    blank = [n for n in flips if not stat[n]["covers"]]
    print(f"\n{len(flips)} cases flip a flag, of which {len(blank)} cover no pixel with S.ah > 0 on the flipped layer: {blank}")
    assert len(flips) - len(blank) >= 8                                         # measured: 17 of 17 (four seeds, thirteen corners)
    assert [n for n in flips if n not in blank and not stat[n]["mutation_shows"]] == []
    stated = [n for n, c in cases.items() if c["hazed_mutation"] in ("flags_all_off", "polygon_refused")]
    assert len(stated) >= 20 and all(stat[n]["stated"] for n in stated)
    off = [n for n in stated if cases[n]["hazed_mutation"] == "flags_all_off" and stat[n]["haze_on"]]
    assert sum(stat[n]["mutation_shows"] for n in off) >= 0.8 * len(off)       # (and switching every flag off is seen)


def probe_ends(c, state, layer, record=0):
    """overlay_haze_model.probe of one record of one of the case's layers: the ends after clipping and the record itself"""
    L = sf.layers(c, state)
    a, b = L.ranges[L.index[layer]]
    recs = np.concatenate(L.recs[a:b])
    rec = recs[(recs["flags"] & 3) == 2][record]              # (a segment: a round cap's ends are records of their own)
    return sf.ohm.probe(c["W"], c["H"], state["u"], state["heights"], c["grid"], rec, 0, 0, sf.the_haze(state)), rec


def alone(c, state, layer):
    """(pairs, middle, clear) of one layer flagged alone"""
    return sf.hazed_counts(c, state, only=layer)


def test_the_hazed_corners_hold_the_edges_they_are_named_for(hazed):
    cases, stat = hazed
    by = {n: c for n, c in cases.items() if n.startswith("hazed_")}
    assert len(by) == 19 and all(c["late"]["on"] == sf.LATE_PASSES and max(c["W"], c["H"]) <= 130 and c["grid"] <= 65 for c in by.values())
    for n, c in by.items():                                   # the corners' own layers follow the eight drawn calls, or replace them
        assert len(c["overlays"]) >= sf.DRAWN or n in ("hazed_side_array_grows_behind_an_early_flag", "hazed_one_flag_on_the_last_layer"), n
    # a zero-length segment alone in its path covers pixels under the round cap at either width (a segment without length has no
    # direction to extend a butt or a square cap along: the model draws nothing of those)
    c = by["hazed_zero_length_segments_every_cap"]
    state = everything_on(c)
    widths = set()
    for j in range(6):
        kind, kw = c["overlays"][sf.DRAWN + j]
        assert kind == "lines" and [len(p) for p in kw["paths"]] == [2, 3] and (kw["paths"][0][0] == kw["paths"][0][1]).all() and (kw["paths"][1][0] == kw["paths"][1][1]).all()
        widths.add(kw["width_px"])
        only = dict(c, overlays=c["overlays"][:sf.DRAWN + j] + [(kind, dict(kw, paths=kw["paths"][:1]))] + c["overlays"][sf.DRAWN + j + 1:])
        pairs = alone(only, state, sf.DRAWN + j)[0]
        print(f"\nzero-length segment, cap {kw['cap']}, width {kw['width_px']}: {pairs} covered pixels")
        assert (pairs > 0) == (kw["cap"] == "round"), (kw["cap"], kw["width_px"], pairs)
    assert widths == {0.5, 80.0} and {c["overlays"][sf.DRAWN + j][1]["cap"] for j in range(6)} == set(sf.CAPS)
    # the paths through the eye: the near plane cuts them, and the clipped end's y is not the vertex's
    for n in ("hazed_paths_through_the_eye_falloff0p3", "hazed_paths_through_the_eye_fovy170_saturated"):
        c = by[n]
        state = everything_on(c)
        assert c["late"]["haze"]["falloff"] == 0.3
        for layer in (sf.DRAWN, sf.DRAWN + 1):
            p, rec = probe_ends(c, state, layer)
            print(f"\n{n} layer {layer}: clipped ends y {float(p['y_a']):.4f} .. {float(p['y_b']):.4f}, 1/w {float(p['rw_a']):.4f} .. {float(p['rw_b']):.4f}")
            assert p["rw_a"] > 0 and p["rw_b"] > 0
            if layer == sf.DRAWN:                              # (the free path: its y is the record's own)
                assert abs(float(p["y_b"]) - float(rec["p1"][1])) > 0.01 and abs(float(p["y_a"]) - float(rec["p0"][1])) < 1e-6
        assert stat[n]["pairs"] > 0
    s = stat["hazed_paths_through_the_eye_fovy170_saturated"]
    assert by["hazed_paths_through_the_eye_fovy170_saturated"]["fovy"] == 170.0 and s["pairs"] > s["middle"] + s["clear"]      # (pairs at max_opacity)
    # the near-plane camera: a hazed occluding layer beside an unhazed occluding one, and the terrain hides part of the hazed one
    c = by["hazed_near_plane_through_the_terrain"]
    state = everything_on(c)
    (_, a), (_, b) = c["overlays"][sf.DRAWN], c["overlays"][sf.DRAWN + 1]
    on = dict(zip(sf.eligible(c), c["hazed"]["flags"]))
    assert a["occlude"] and b["occlude"] and on[sf.DRAWN] and not on[sf.DRAWN + 1] and c["hazed_mutation_args"]["occlusion_layer"] == sf.DRAWN and c["znear"] == 0.4
    hidden = alone(c, dict(state, occlusion={sf.DRAWN: (False, 0.0)}), sf.DRAWN)[0] - alone(c, state, sf.DRAWN)[0]
    print(f"\nthe near-plane corner: the terrain hides {hidden} covered pixels of the hazed occluding layer")
    assert hidden > 0 and alone(c, state, sf.DRAWN)[0] > 0
    # vertices without a height under draped hazed layers
    c = by["hazed_draped_over_one_nan_texel"]
    assert int(np.isnan(c["heights"]).sum()) == 1 and stat[c["name"]]["pairs"] > 0 and all(c["overlays"][sf.DRAWN + j][1]["drape"] for j in (0, 1))
    c = by["hazed_draped_over_the_all_nan_texture"]
    assert np.isnan(c["heights"]).all() and stat[c["name"]]["pairs"] == 0 and c["mutation"] == "heights"          # (the height upload brings ground under them)
    after = sf.mutated(c, everything_on(c))
    assert sf.hazed_counts(c, after)[0] > 0
    # no opacity, three ways: pairs, every one with S.ah == 0, the unflagged bytes; haze_params brings start to 0
    for n in ("hazed_no_opacity_start_beyond_every_depth", "hazed_no_opacity_max_opacity_0", "hazed_no_opacity_colour_of_alpha_0"):
        s, c = stat[n], by[n]
        assert s["pairs"] > 0 and s["clear"] == s["pairs"] and not s["differs"] and c["hazed_mutation"] == "haze_params" and c["hazed_mutation_args"]["haze"]["start"] == 0.0, n
    Z = [by[n]["late"]["haze"] for n in ("hazed_no_opacity_start_beyond_every_depth", "hazed_no_opacity_max_opacity_0", "hazed_no_opacity_colour_of_alpha_0")]
    assert Z[0]["start"] == 1e6 and Z[1]["max_opacity"] == 0.0 and Z[2]["rgba"][3] == 0
    # the side array: the records behind the early flag are more than four times those before it
    c = by["hazed_side_array_grows_behind_an_early_flag"]
    L = sf.layers(c, everything_on(c))
    before = sum(len(r) for r in L.recs[:L.ranges[L.index[0]][1]])
    total = sum(len(r) for r in L.recs)
    print(f"\nthe growth corner: {before} records when the first flag is set, {total} in the end, {L.segments[1]} contour segments")
    assert c["grid"] == 65 and not c["smooth"] and c["hazed"]["early"][0] and not c["hazed"]["early"][1] and len(c["overlays"][1][1]["levels"]) == 6
    assert total > 4 * before and L.segments[1] >= 2000 and len(c["overlays"][2][1]["xyz"]) == 300 and c["overlays"][2][1]["size_px"] == 1.0
    c = by["hazed_one_flag_on_the_last_layer"]
    assert c["hazed"]["flags"] == (False, False, True) and c["hazed"]["early"][2] is False and c["hazed_mutation"] == "readd" and c["overlays"][-1][0] == "points"
    # the staircase: a hazed contour layer with a level on a plateau
    c = by["hazed_contours_on_the_staircase"]
    surf = sf.cm.surface(c["heights"], c["grid"])
    k = next(i for i, (kind, _) in enumerate(c["overlays"]) if kind == "contours")
    assert dict(zip(sf.eligible(c), c["hazed"]["flags"]))[k] and max(int((surf == v).sum()) for v in c["overlays"][k][1]["levels"]) > 20
    assert c["mutation"] == "heights" and alone(c, everything_on(c), k)[0] > 0
    # frames of one pixel, one column and one row under a 64-px point and an 80-px line
    for n, size in (("hazed_frame1x1", (1, 1)), ("hazed_frame_of_one_column", (1, 70)), ("hazed_frame_of_one_row", (130, 1))):
        c = by[n]
        assert (c["W"], c["H"]) == size and c["overlays"][sf.DRAWN][1]["size_px"] == 64.0 and c["overlays"][sf.DRAWN + 1][1]["width_px"] == 80.0
        assert alone(c, everything_on(c), sf.DRAWN)[0] > 0 and alone(c, everything_on(c), sf.DRAWN + 1)[0] > 0, n
    assert by["hazed_frame_of_one_row"]["fovy"] == sf.CORNERS.named("late_frame_of_one_row")["fovy"]
    for n, f, size in (("hazed_supersample3_frame15x17", 3, (15, 17)), ("hazed_supersample4_frame1x1", 4, (1, 1))):
        c = by[n]
        assert c["late"]["supersample"] == f and (c["W"], c["H"]) == size and stat[n]["pairs"] > 0
        e = sf.expected_supersampled(c, everything_on(c), f)
        assert (e["frame"] != sf.expected_supersampled(c, everything_on(c, flags=False), f)["frame"]).any(), n
    for n, ex, sp in (("hazed_exaggeration0_spacing0p3", 0.0, 0.3), ("hazed_exaggeration_minus2_spacing2p5", -2.0, 2.5)):
        c = by[n]
        assert (c["exaggeration"], c["spacing"]) == (ex, sp) and c["overlays"][sf.DRAWN][1]["drape"] and not c["overlays"][sf.DRAWN + 1][1]["drape"]
        assert alone(c, everything_on(c), sf.DRAWN)[0] > 0 and alone(c, everything_on(c), sf.DRAWN + 1)[0] > 0, n


def test_expected_is_deterministic_with_the_hazed_state(oracle):
    for c in [sf.case(FIRST_SEED + 3), sf.CORNERS.named("hazed_side_array_grows_behind_an_early_flag")]:
        on = everything_on(c)
        for state in [on] + [s for _, s in sf.hazed_steps(c, on)] + [sf.mutated(c, sf.hazed_mutated(c, on))]:
            a, b = sf.expected(c, state), sf.expected(sf.case(int(c["name"][4:])) if c["name"].startswith("seed") else c, state)
            assert a["frame"].tobytes() == b["frame"].tobytes()
    # a cached entry made under other flags is never returned
    c, cache = sf.CORNERS.named("hazed_zero_length_segments_every_cap"), {}
    on = everything_on(c)
    seen = {sf.expected(c, s, cache)["frame"].tobytes() for s in (on, everything_on(c, flags=False), sf.hazed_mutated(c, on), dict(on, hazed=None))}
    assert len(seen) == 4 and sf.expected(c, on, cache)["frame"].tobytes() == sf.expected(c, on)["frame"].tobytes()

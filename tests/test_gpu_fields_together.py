"""The seven per-vertex fields of one handle -- shadow, sky view (4i), viewshed (4l), cumulative viewshed (4m), sun
exposure (4n), flood (4s), spill (4t) -- keep their caches apart: each is computed again for its own inputs alone; all seven for the
heights; five for the exaggeration, which the flood and the spill (fields in units of h before it) do not know; none for seeds that
move inside their vertices' cells, and none for a diagnostic call; a forgotten viewshed observer does not restart its counter.  Every
field is held to its CPU model bit for bit after every change.  Grid 130: the scans' 64-step chunks carry across a boundary, and the
flood and the spill run 3 x 3 tiles."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from support import assert_field, terrain, uniforms, viridis
import ambient_model as abm
import cumulative_viewshed_model as cvm
import flood_model as fdm
import shadow_model as shm
import spill_model as spm
import sun_exposure_model as sem
import viewshed_model as vsm
from overlay_scenes import heights

W, H, GRID = 96, 64, 130
SHADOWS = dict(strength=0.8, softness=0.05, bias=0.01)
SCAN = dict(eye_height=0.4, target_height=0.02, softness=0.05, bias=0.01)
EXPOSURE = dict(incidence=True, softness=0.05, bias=0.01)
FIELDS = ("shadow", "ambient", "viewshed", "cumulative", "exposure", "flood", "spill")
OLD = FIELDS[:4]


def test_each_field_follows_its_own_inputs_alone():
    from vulkan_forge_amd._ambient import directions
    dirs = directions(4)
    h0 = heights(4, (97, 131))
    # the flood's seeds on their vertices (a nudge below stays inside the cell): one in each of two tiles; the spill from the border
    S = dict(h=h0, sun=(0.9, 0.5, 0.31), exag=0.6, reach=8.0, observer=(0.41, -0.87), observers=[(-1.5, -1.5), (0.0, 0.0), (0.9, 1.2)],
             suns=[shm.sun_vector(12.0, 70.0), shm.sun_vector(40.0, 200.0), shm.sun_vector(-5.0, 10.0)],
             level=fdm.field_level(fdm.cm.surface(h0, GRID), 0.5), flood_seeds=[fdm.vertex_xz((3, 3), GRID), fdm.vertex_xz((100, 80), GRID)], spill_seeds="edges")
    t = terrain(W, H, GRID, S["h"], viridis())

    def apply_scene():
        if S.pop("new_heights", False):
            t.set_height(S["h"])
        t.set_uniforms(uniforms(W, H, exag=S["exag"], sun=S["sun"]))
        t.set_shadows(True, **SHADOWS)
        t.set_ambient_occlusion(True, strength=0.6, reach=S["reach"], directions=dirs)
        t.set_viewshed(S["observer"], **SCAN)
        t.set_cumulative_viewshed(S["observers"], **SCAN)
        t.set_sun_exposure(np.array(S["suns"], np.float32), **EXPOSURE)
        t.set_flood(S["level"], S["flood_seeds"])
        t.set_spill(S["spill_seeds"])

    def models():
        u = uniforms(W, H, exag=S["exag"], sun=S["sun"])
        return dict(shadow=shm.field(u, S["h"], GRID, **SHADOWS), ambient=abm.field(u, S["h"], GRID, dirs, S["reach"]),
                    viewshed=vsm.field(u, S["h"], GRID, S["observer"], **SCAN)[0], cumulative=cvm.field(u, S["h"], GRID, S["observers"], **SCAN)[0],
                    exposure=sem.field(u, S["h"], GRID, np.array(S["suns"], np.float32), None, **EXPOSURE),
                    flood=fdm.field(u, S["h"], GRID, S["level"], S["flood_seeds"]).depth, spill=spm.field(u, S["h"], GRID, S["spill_seeds"]).spill)

    READ = dict(shadow=t.shadow_field, ambient=t.sky_view_field, viewshed=t.viewshed_field, cumulative=t.cumulative_viewshed_field,
                exposure=t.sun_exposure_field, flood=t.flood_field, spill=t.spill_field)

    def scans():
        return dict(shadow=t.shadow_scans(), ambient=t.ambient_scans(), viewshed=t.viewshed_scans(), cumulative=t.cumulative_viewshed_scans(),
                    exposure=t.sun_exposure_scans(), flood=t.flood_scans(), spill=t.spill_scans())

    def check(what, moved, order=FIELDS):
        """the fields equal the models, those of `moved` are new ones, and the counters of `moved`, no others, went up by one"""
        nonlocal want, count
        before, want = want, models()
        for name in order:
            assert_field(READ[name](), want[name], f"{what}: {name} field")
            if before is not None:
                assert (name in moved) == bool((want[name].view(np.uint32) != before[name].view(np.uint32)).any()), f"{what}: the {name} model"
        count = {name: count[name] + (name in moved) for name in count}
        assert scans() == count, what

    want, count = None, dict.fromkeys(FIELDS, 0)
    apply_scene()
    assert scans() == count
    check("first read", FIELDS)
    assert count == dict.fromkeys(FIELDS, 1)
    for name in FIELDS:
        assert (want[name] != want[name].flat[0]).mean() > 0.02, f"the {name} field is a trivial one"
    assert np.isfinite(want["spill"]).all() and (want["flood"] > 0).mean() > 0.02 and (want["flood"] == 0).mean() > 0.02
    check("read again in another order", (), order=("spill", "cumulative", "flood", "ambient", "shadow", "exposure", "viewshed"))

    S["sun"] = (-0.31, 0.4, 0.9)
    apply_scene()
    check("a new sun", ("shadow",))
    S["reach"] = 5.0
    apply_scene()
    check("a new reach", ("ambient",))
    S["observer"] = (-0.6, 0.2)
    apply_scene()
    check("the observer at another vertex", ("viewshed",))
    S["observers"] = [S["observers"][0], (0.3, -1.1), S["observers"][2]]
    apply_scene()
    check("one cumulative observer replaced", ("cumulative",))
    S["suns"] = [S["suns"][0], shm.sun_vector(25.0, 300.0), S["suns"][2]]
    apply_scene()
    check("a new sun list", ("exposure",))
    S["level"] = fdm.field_level(fdm.cm.surface(S["h"], GRID), 0.6)
    apply_scene()
    check("a new level", ("flood",))
    S["flood_seeds"] = [fdm.vertex_xz((89, 127), GRID), fdm.vertex_xz((76, 26), GRID)]      # (in two ponds beside the water the first seeds fed)
    apply_scene()
    check("the flood's seeds at other vertices", ("flood",))
    assert 0 < (want["flood"] > 0).sum() < 200
    S["spill_seeds"] = [spm.vertex_xz((3, 3), GRID), spm.vertex_xz((100, 80), GRID)]
    apply_scene()
    check("the spill from seeds, not the border", ("spill",))
    step = 3.0 / (GRID - 1)
    nudge = lambda seeds: [(x + 0.2 * step, z - 0.2 * step) for x, z in seeds]
    for key in ("flood_seeds", "spill_seeds"):
        assert nudge(S[key]) != S[key] and np.array_equal(fdm.seed_vertices(nudge(S[key]), 1.0, GRID), fdm.seed_vertices(S[key], 1.0, GRID))
        S[key] = nudge(S[key])
    apply_scene()
    check("seeds nudged inside their cells", ())
    stood = {name: want[name].copy() for name in ("flood", "spill")}
    S["exag"] = 1.6
    apply_scene()
    check("a new exaggeration", ("shadow", "ambient", "viewshed", "cumulative", "exposure"))
    for name in ("flood", "spill"):                           # (neither model knows the exaggeration: the same bits)
        assert np.array_equal(want[name].view(np.uint32), stood[name].view(np.uint32)), name
    S["h"], S["new_heights"] = heights(9, (97, 131)), True
    apply_scene()
    check("new heights", FIELDS)

    # the diagnostic calls launch every field again and again, and count nothing (they time the frame rendered last)
    t.render()
    t.read_rgba()
    assert scans() == count
    for stage in (t.shadow_stage, t.ambient_stage, t.viewshed_stage, t.flood_stage, t.spill_stage):
        ms = stage(1)
        assert ms[0] > 0 and ms[1] > 0 and scans() == count, stage.__name__
    assert t.cumulative_viewshed_stage(1) > 0 and scans() == count
    assert t.sun_exposure_stage(1) > 0 and scans() == count
    check("after the diagnostic calls", ())

    # a forgotten observer takes its field along, not its counter
    t.clear_viewshed()
    assert scans() == count
    from vulkan_forge_amd.cabi import VfError
    with pytest.raises(VfError, match="no observer set"):
        t.viewshed_field()
    apply_scene()
    assert_field(t.viewshed_field(), want["viewshed"], "the observer set again")
    count["viewshed"] += 1
    assert scans() == count and count["viewshed"] == 5
    assert {name: count[name] for name in OLD} == dict(shadow=4, ambient=4, viewshed=5, cumulative=4)      # (what the four older fields counted before)
    t.close()

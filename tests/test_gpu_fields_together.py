"""The four per-vertex fields of one handle -- shadow, sky view (4i), viewshed (4l), cumulative viewshed (4m) -- keep
their caches apart: each is computed again for its own inputs alone, all four for the exaggeration and the heights, none for a
diagnostic call; a forgotten viewshed observer does not restart its counter.  Every field is held to its CPU model bit for bit after
every change.  Grid 130: the scans' 64-step chunks carry across a boundary."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
for _model in ("overlay_model", "polygon_model", "occlusion_model", "shadow_model", "ambient_model", "viewshed_model", "cumulative_viewshed_model"):
    sys.path.insert(0, os.path.join(HERE, _model))
import ambient_model as abm  # noqa: E402
import cumulative_viewshed_model as cvm  # noqa: E402
import shadow_model as shm  # noqa: E402
import viewshed_model as vsm  # noqa: E402
from overlay_scenes import heights  # noqa: E402
from test_gpu_viewshed import assert_field, terrain, uniforms, viridis  # noqa: E402

W, H, GRID = 96, 64, 130
SHADOWS = dict(strength=0.8, softness=0.05, bias=0.01)
SCAN = dict(eye_height=0.4, target_height=0.02, softness=0.05, bias=0.01)


def test_each_field_follows_its_own_inputs_alone():
    from vulkan_forge_amd._ambient import directions
    dirs = directions(4)
    S = dict(h=heights(4, (97, 131)), sun=(0.9, 0.5, 0.31), exag=0.6, reach=8.0, observer=(0.41, -0.87), observers=[(-1.5, -1.5), (0.0, 0.0), (0.9, 1.2)])
    t = terrain(W, H, GRID, S["h"], viridis())

    def apply_scene():
        if S.pop("new_heights", False):
            t.set_height(S["h"])
        t.set_uniforms(uniforms(W, H, exag=S["exag"], sun=S["sun"]))
        t.set_shadows(True, **SHADOWS)
        t.set_ambient_occlusion(True, strength=0.6, reach=S["reach"], directions=dirs)
        t.set_viewshed(S["observer"], **SCAN)
        t.set_cumulative_viewshed(S["observers"], **SCAN)

    def models():
        u = uniforms(W, H, exag=S["exag"], sun=S["sun"])
        return dict(shadow=shm.field(u, S["h"], GRID, **SHADOWS), ambient=abm.field(u, S["h"], GRID, dirs, S["reach"]),
                    viewshed=vsm.field(u, S["h"], GRID, S["observer"], **SCAN)[0], cumulative=cvm.field(u, S["h"], GRID, S["observers"], **SCAN)[0])

    READ = dict(shadow=t.shadow_field, ambient=t.sky_view_field, viewshed=t.viewshed_field, cumulative=t.cumulative_viewshed_field)

    def scans():
        return dict(shadow=t.shadow_scans(), ambient=t.ambient_scans(), viewshed=t.viewshed_scans(), cumulative=t.cumulative_viewshed_scans())

    def check(what, moved, order=("shadow", "ambient", "viewshed", "cumulative")):
        """the fields equal the models, those of `moved` are new ones, and the counters of `moved`, no others, went up by one"""
        nonlocal want, count
        before, want = want, models()
        for name in order:
            assert_field(READ[name](), want[name], f"{what}: {name} field")
            if before is not None:
                assert (name in moved) == bool((want[name].view(np.uint32) != before[name].view(np.uint32)).any()), f"{what}: the {name} model"
        count = {name: count[name] + (name in moved) for name in count}
        assert scans() == count, what

    want, count = None, dict(shadow=0, ambient=0, viewshed=0, cumulative=0)
    apply_scene()
    assert scans() == count
    check("first read", ("shadow", "ambient", "viewshed", "cumulative"))
    assert count == dict(shadow=1, ambient=1, viewshed=1, cumulative=1)
    for name in ("shadow", "ambient", "viewshed", "cumulative"):
        assert (want[name] != want[name].flat[0]).mean() > 0.02, f"the {name} field is a trivial one"
    check("read again in another order", (), order=("cumulative", "ambient", "shadow", "viewshed"))

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
    S["exag"] = 1.6
    apply_scene()
    check("a new exaggeration", ("shadow", "ambient", "viewshed", "cumulative"))
    S["h"], S["new_heights"] = heights(9, (97, 131)), True
    apply_scene()
    check("new heights", ("shadow", "ambient", "viewshed", "cumulative"))

    # the diagnostic calls launch every field again and again, and count nothing (they time the frame rendered last)
    t.render()
    t.read_rgba()
    assert scans() == count
    for stage in (t.shadow_stage, t.ambient_stage, t.viewshed_stage):
        ms = stage(1)
        assert ms[0] > 0 and ms[1] > 0 and scans() == count, stage.__name__
    assert t.cumulative_viewshed_stage(1) > 0 and scans() == count
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
    t.close()

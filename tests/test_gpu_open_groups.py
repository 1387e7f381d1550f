"""The box hand-over from pass A to the line loop: the tile kernel with line groups no longer works a
survivor's box out of its vertices in raster_fast -- pass A packs it beside the survivor, compacted in place -- and the strip
instantiation shares the survivor words.  Whatever shape an item has, the frame must stay the oracle's bit for bit: whole tiles, strips of
32, 16 and 4 pixels (asked for through injected plan feedback), both line loops forced, colour and stored visibility (the
visibility read draws the frame again with the visibility-storing instantiations), small frames whose last tile column and row are 8
pixels wide, a coarse and a fine grid, a close view whose triangles are longer than a tile, and a frame drawn twice."""
import numpy as np
import pytest

import plan_model as pm
from support import cabi  # noqa: F401
from test_gpu_plan_feedback import Rig, camera, oracle_frame

pytestmark = pytest.mark.gpu

COARSE = (200, 136, 33)           # 4 x 3 tiles, the last column and the last row 8 pixels
FINE = (300, 200, 137)            # 5 x 4 tiles, triangles of a few pixels
CLOSE = ((0.0, 0.4, 0.0), (0.5, 0.0, 0.4), (0.0, 1.0, 0.0), 70.0, 0.05, 100.0)   # grid 33 from just above the surface: triangles up to 78 lines on their SHORT side at 200 x 136
CUTS = (0, 1, 2, 4)               # whole tiles, strips of 32, 16 and 4 pixels


def uniforms(oracle, size, cam):
    W, H, _ = size
    return oracle.look_at_uniforms(1, W, H, *CLOSE) if cam == "close" else camera(oracle, cam, W, H)


@pytest.fixture(scope="module")
def rigs(cabi, oracle, luts):
    made = {}

    def get(size, cam):
        if (size, cam) not in made:
            made[(size, cam)] = Rig(cabi, oracle, luts, size, uniforms(oracle, size, cam))
        return made[(size, cam)]
    yield get
    for r in made.values():
        r.close()


VIEWS = [(COARSE, "default"), (COARSE, "fill"), (COARSE, "close"), (FINE, "default"), (FINE, "fill")]


@pytest.mark.parametrize("size,cam", VIEWS, ids=[f"{s[0]}x{s[1]}g{s[2]}-{c}" for s, c in VIEWS])
@pytest.mark.parametrize("groups", (0, 1))
def test_every_item_shape_draws_the_oracle_frame(rigs, size, cam, groups):
    rig = rigs(size, cam)
    rig.t.set_raster_groups(groups)
    for k in CUTS:
        # (the close view's plan is not held to the model of the cut rule: primitives beside the eye send items to the complete launch, and
        #  the plan cuts three of its tiles finer than the table asks -- the frame is what is checked there, under whatever cuts it got)
        cuts, _req, _mode = rig.frame(pm.uniform_cut_table(k, rig.tx, size[0]), exact=cam != "close")
        assert rig.t.raster_groups()[0] == groups
        busy = cuts >= 0
        assert busy.sum() >= 4
        if cam != "close":
            assert (cuts[busy & rig.full] == k).all() and (cuts[busy & ~rig.full] == 0).all()  # the strips asked for; the 8-pixel column stays whole
    rig.t.render()                                           # the same frame once more: nothing of the first one's tile state is left over
    rig.compare()


def test_the_close_view_holds_a_triangle_longer_than_a_tile(oracle, luts):
    """what the close view is for: a triangle whose box is more than 64 lines on its short side lies across a tile edge whatever the
    axis it is walked along, and every item it reaches sees it clamped to that item's rectangle"""
    _rgba, vis = oracle_frame(oracle, luts, uniforms(oracle, COARSE, "close"), COARSE)
    ys, xs = np.nonzero(vis)
    ids = vis[ys, xs]
    longest = 0
    for i in np.unique(ids):
        m = ids == i
        longest = max(longest, min(int(np.ptp(ys[m])), int(np.ptp(xs[m]))) + 1)
    assert longest > 64, longest

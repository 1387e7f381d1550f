"""The frame plan under INJECTED tile times (vf_terrain_debug_set_plan_feedback): every cut the plan can make is asked
for on purpose, the item codes of each frame are held to the model of the cut rule (tests/plan_model.py), and every frame to the CPU
oracle -- EXACT colour and stored visibility bit for bit, the one FAST frame within RGBA_TOL.  "Feedback steers speed only, never a
pixel" is the property under test; what the feedback IS no longer depends on the machine's timing that day.

A frame here: inject, render, read the colour and the item codes, then read the visibility -- which draws the frame again with the
visibility-storing tile kernel, planned from the same injected words in the other plan state."""

import numpy as np
import pytest

import plan_model as pm
from conftest import heightmap
from support import cabi  # noqa: F401
from test_gpu_parity import EXACT, FAST, RGBA_TOL

pytestmark = pytest.mark.gpu

SMALL = (300, 200, 65)            # 5 x 4 tiles: the last column 44 pixels wide, the last row 8 high
# The frame-filling camera of overlay_scenes shows the terrain as a patch about 1.05 frame heights wide, so upright frames fill best.  The
# sizes are the smallest (in tiles, sides 10 .. 14 and 40 .. 55 tiles) whose oracle frame shows terrain in enough tiles -- busy tiles are
# at least those:
BUDGET = (704, 896, 129)          # 145 of 11 x 14 tiles, all full-width: 137 tiles that ask for 16 strips ask for more than the 2048 extra items
LARGE = (2752, 3392, 257)         # 2071 of 43 x 53 tiles.  The split budget turns a tile away only once fewer than 15 of its 2048 items are left,
                                  # so it grants at least 2034: 2063 busy tiles make more than one 4096-item run of the sort whatever the atomics' order
HEIGHT_SEED = 5


def camera(oracle, name, W, H):
    from overlay_scenes import CAMERAS
    return oracle.look_at_uniforms(1, W, H, *CAMERAS[name])


_ORACLE = {}


def oracle_frame(oracle, luts, u, size):
    """(rgba, vis) of the whole frame, made once per (uniforms, size)"""
    W, H, G = size
    key = (np.asarray(u, np.float32).tobytes(), size)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.render_terrain(u, W, H, G, heightmap(HEIGHT_SEED, G), luts["viridis"], nthreads=min(16, oracle.max_threads()))
    return _ORACLE[key]


class Rig:
    """A whole-frame handle past its first two frames, with per-item statistics: inject -> render -> compare."""

    def __init__(self, cabi, oracle, luts, size, u, stats=True, warm=True):
        self.cabi, self.oracle, self.luts, self.size = cabi, oracle, luts, size
        W, H, G = size
        self.ntx, self.nty = (W + 63) // 64, (H + 63) // 64
        self.n = self.ntx * self.nty
        self.tx, self.ty = np.tile(np.arange(self.ntx), self.nty), np.repeat(np.arange(self.nty), self.ntx)
        self.full = pm.tile_widths(self.tx, W) == 64
        self.stats = stats
        self.t = t = cabi.Terrain(W, H, G, luts["viridis"])
        t.set_height(heightmap(HEIGHT_SEED, G)); t.set_shade_precision(EXACT)
        if stats:
            t.enable_timing(True)
        self.pose(u)
        if warm:
            t.render(); t.render()                           # the static estimate's frames: the injection is refused before them

    def close(self):
        self.t.close()

    def pose(self, u):
        self.u = np.asarray(u, np.float32)
        self.t.set_uniforms(self.u)

    def covered(self, vis):
        W, H, _ = self.size
        pad = np.zeros((self.nty * 64, self.ntx * 64), bool)
        pad[:H, :W] = vis > 0
        return pad.reshape(self.nty, 64, self.ntx, 64).any(axis=(1, 3)).ravel()

    def compare(self, fast=False):
        """the frame rendered last against the oracle; returns (cuts per tile or None, mode word)"""
        t = self.t
        ref_rgba, ref_vis = oracle_frame(self.oracle, self.luts, self.u, self.size)
        rgba = t.read_rgba()
        codes = t.item_stats()[:, 0] if self.stats else None
        cuts = pm.items_to_cuts(codes, self.n) if self.stats else None
        mode = t.plan_mode()
        if cuts is not None:
            print(f"{self.size[0]}x{self.size[1]}: {len(codes)} items, {int((cuts >= 0).sum())} busy tiles, cuts {np.bincount(cuts[cuts >= 0], minlength=5).tolist()}, mode {mode}")
        else:
            print(f"{self.size[0]}x{self.size[1]}: mode {mode}")
        vis = t.read_visibility()
        assert t.plan_mode() == mode                         # (the visibility frame is not "the frame rendered last")
        bad = int((vis != ref_vis).sum())
        assert bad == 0, f"visibility differs at {bad} pixels"
        d = int(np.abs(rgba.astype(np.int16) - ref_rgba.astype(np.int16)).max(initial=0))
        assert d <= (RGBA_TOL if fast else 0), f"RGBA differs from the oracle by {d} LSB"
        if cuts is not None:
            lost = np.flatnonzero(self.covered(ref_vis) & (cuts < 0))
            assert len(lost) == 0, f"tiles {lost[:8].tolist()} show terrain and have no work item"
        return cuts, mode

    def frame(self, words, lgs=None, pieces=None, fast=False, moving=False, exact=True):
        """inject, render, compare with the oracle and with the model's request; returns (cuts, request, mode)"""
        lgs = np.zeros(self.n, np.uint8) if lgs is None else lgs
        pieces = np.zeros((self.n, 64), np.uint32) if pieces is None else pieces
        self.t.set_plan_feedback(words, lgs, pieces)
        self.t.render()
        cuts, mode = self.compare(fast)
        if cuts is None:
            return None, None, mode
        W = self.size[0]
        req = pm.request(words, lgs, pieces, self.tx, self.ty, W, self.ntx, self.nty, True, cuts >= 0, moving=moving)
        assert (cuts[~self.full] <= 0).all(), "a tile narrower than 64 pixels was cut"
        if exact:
            pm.check_against_request(cuts, req)
        else:                                                # (the lookup through the camera motion is not modelled)
            assert int(((1 << cuts[cuts >= 0]) - 1).sum()) <= pm.SPLIT_BUDGET
        return cuts, req, mode


@pytest.fixture(scope="module")
def small(cabi, oracle, luts):
    rigs = {}

    def get(cam):
        if cam not in rigs:
            rigs[cam] = Rig(cabi, oracle, luts, SMALL, camera(oracle, cam, SMALL[0], SMALL[1]))
        rigs[cam].pose(camera(oracle, cam, SMALL[0], SMALL[1]))
        rigs[cam].t.set_shade_precision(EXACT); rigs[cam].t.set_raster_groups(-1)
        return rigs[cam]
    yield get
    for r in rigs.values():
        r.close()


# ---- the small frame: every cut, on purpose ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ["default", "fill"])
@pytest.mark.parametrize("k", range(5))
def test_every_full_width_tile_in_2_to_the_k_strips(small, cam, k):
    rig = small(cam)
    words = pm.uniform_cut_table(k, rig.tx, SMALL[0])
    for groups in (0, 1):                                    # both line loops of the raster stage
        rig.t.set_raster_groups(groups)
        cuts, req, mode = rig.frame(words)
        assert rig.t.raster_groups()[0] == groups
        busy = cuts >= 0
        assert busy[rig.full].sum() >= 4 and (busy[~rig.full].any() or cam != "fill")
        assert not req["limited"] and (req["lg"][busy & rig.full] == k).all()
        assert (cuts[busy & rig.full] == k).all()            # the cut the test is named for: strips of 64 >> k pixels
        assert (cuts[busy & ~rig.full] == 0).all()           # the edge column stays whole, heavy as its words are
        assert mode == 0                                     # a resting plan from the handle's own state
    if k == 4:                                               # once in fast precision: 4-pixel strips through the fast fragment path
        rig.t.set_shade_precision(FAST)
        cuts, _, _ = rig.frame(words, fast=True)
        assert (cuts[(cuts >= 0) & rig.full] == 4).all()


@pytest.mark.parametrize("seed", range(16))
def test_seeded_random_tables(small, seed):
    rig = small("fill")
    words, lgs, pieces = pm.random_table(seed, rig.n)
    cuts, req, mode = rig.frame(words, lgs, pieces)
    assert not req["limited"] and mode == 0
    assert (cuts >= 0).sum() >= 17


def test_all_zero_and_overflowing_tables(small):
    rig = small("fill")
    cuts, req, _ = rig.frame(np.zeros(rig.n, np.uint32), np.full(rig.n, 4, np.uint8), np.full((rig.n, 64), 0xFFFFFFFF, np.uint32))
    assert req["quantum"] == 0 and (cuts <= 0).all()         # no times at all: the static fall-back orders the frame, nothing is split
    words = np.full(rig.n, 0xFFFFFFFF, np.uint32)
    cuts, req, _ = rig.frame(words)
    assert int(words.astype(np.uint64).sum()) > 1 << 32 and req["quantum"] == 7 * rig.n * 0xFFFFFFFF // 4096
    assert (cuts[(cuts >= 0) & rig.full] == 4).all()         # 4096 / (7 * 20) = 29 quanta each
    words[::2] = 1
    cuts, req, _ = rig.frame(words, np.full(rig.n, 4, np.uint8), np.full((rig.n, 64), 0xFFFFFFFF, np.uint32))    # every lift saturates
    assert (req["seen"][cuts >= 0] == 0xFFFFFFFF // 2).all()


# ---- the budget ----------------------------------------------------------------------------------------------------------------------
def test_the_split_budget_runs_out(cabi, oracle, luts):
    W, H, _ = BUDGET
    rig = Rig(cabi, oracle, luts, BUDGET, camera(oracle, "fill", W, H))
    try:
        words, lgs, pieces = np.ones(rig.n, np.uint32), np.full(rig.n, 4, np.uint8), np.full((rig.n, 64), 1000, np.uint32)
        cuts, req, _ = rig.frame(words, lgs, pieces)
        busy = (cuts >= 0) & rig.full
        assert busy.sum() >= 137, int(busy.sum())
        assert req["quantum"] == 1 and (req["lg"][busy] == 4).all() and req["limited"]       # 8000 quanta each: 16 strips asked for every tile
        extra = int(((1 << cuts[busy]) - 1).sum())
        print(f"budget: {int(busy.sum())} busy full-width tiles, asked {req['extra']} extra items, got {extra}")
        assert extra <= pm.SPLIT_BUDGET
        assert (cuts[busy] < 4).any()                        # the fall-back ran: a tile got fewer strips than it asked for
        assert extra >= pm.SPLIT_BUDGET - 14                 # ... and only because the budget was gone: the first tile is turned away with fewer than 15 items left
    finally:
        rig.close()


def test_more_than_4096_items_under_injected_times(cabi, oracle, luts):
    """The one large case: 2049 busy tiles and the 2048 items of the split budget are more than one 4096-item run of k_plan_sort."""
    W, H, _ = LARGE
    rig = Rig(cabi, oracle, luts, LARGE, camera(oracle, "fill", W, H))
    try:
        rng = np.random.default_rng(77)
        words = rng.integers(1, 50, rig.n).astype(np.uint32)
        lgs = rng.integers(1, 5, rig.n).astype(np.uint8)
        pieces = np.exp2(rng.uniform(2.0, 20.0, (rig.n, 64))).astype(np.uint32)
        rig.t.set_plan_feedback(words, lgs, pieces)
        rig.t.render()
        codes = rig.t.item_stats()[:, 0]
        cuts, _ = rig.compare()                              # (the permutation: every part of every busy tile once; the pixels)
        print(f"large: {int((cuts >= 0).sum())} busy tiles, {len(codes)} items")
        assert (cuts >= 0).sum() >= 2049, int((cuts >= 0).sum())
        assert len(codes) > 4096, len(codes)
        req = pm.request(words, lgs, pieces, rig.tx, rig.ty, W, rig.ntx, rig.nty, True, cuts >= 0)
        assert req["limited"]
        pm.check_against_request(cuts, req)
    finally:
        rig.close()


# ---- the plan's modes ----------------------------------------------------------------------------------------------------------------
def test_every_plan_mode_under_injected_times(cabi, oracle, luts):
    W, H, _ = SMALL
    C = cabi
    u = {name: oracle.look_at_uniforms(1, W, H, *pm.orbit_camera(a)) for name, a in pm.MODE_POSES.items()}
    rig = Rig(cabi, oracle, luts, SMALL, u["rest"])
    try:
        seen = []
        steps = [("rest", 0), ("fast", C.VF_PLAN_MOTION_MAP | C.VF_PLAN_DILATE), ("jump", C.VF_PLAN_FRESH | C.VF_PLAN_DILATE), ("jump", None),
                 ("jump", 0), ("slow", C.VF_PLAN_DILATE), ("slow", 0)]
        for step, (pose, want) in enumerate(steps):
            rig.pose(u[pose])
            words, lgs, pieces = pm.random_table(100 + step, rig.n)
            # which words a motion map lands on is float arithmetic: every other mode's cut is the model's, with the neighbourhood rule
            # of a moving camera where the plan says so
            rig.t.set_plan_feedback(words, lgs, pieces)
            rig.t.render()
            cuts, mode = rig.compare()
            seen.append(mode)
            if want is not None:
                assert mode == want, (step, pose, mode)
            assert not mode & (C.VF_PLAN_FIRST | C.VF_PLAN_QUEUED_AHEAD)
            if mode & C.VF_PLAN_MOTION_MAP:
                assert int(((1 << cuts[cuts >= 0]) - 1).sum()) <= pm.SPLIT_BUDGET
            else:
                req = pm.request(words, lgs, pieces, rig.tx, rig.ty, W, rig.ntx, rig.nty, True, cuts >= 0, moving=bool(mode & C.VF_PLAN_DILATE))
                pm.check_against_request(cuts, req)
        print("modes:", seen)
        assert any(m & C.VF_PLAN_MOTION_MAP for m in seen)
        assert any(m & C.VF_PLAN_FRESH and m & C.VF_PLAN_DILATE for m in seen)
        assert any(m == C.VF_PLAN_DILATE for m in seen)
        assert any(m == 0 for m in seen)
    finally:
        rig.close()


def test_a_plan_queued_ahead_reads_the_injected_times_and_an_injection_drops_one(cabi, oracle, luts):
    """Without statistics a camera at rest has its next plan queued behind the frame (or behind the read-back of a caller that waits).
    Injected before the frame that queues it, the words steer the plan queued ahead; injected after it, they throw it away and the
    frame is planned again from the previous frame's state."""
    W, H, _ = SMALL
    C = cabi
    rig = Rig(cabi, oracle, luts, SMALL, camera(oracle, "fill", W, H), stats=False)
    try:
        t = rig.t
        words, lgs, pieces = pm.random_table(200, rig.n)
        t.set_plan_feedback(words, lgs, pieces)
        t.render(); t.read_rgba()                            # the third frame of a resting camera: the next plan goes out
        t.render()
        assert t.plan_mode() == C.VF_PLAN_QUEUED_AHEAD
        rig.compare()
        for _ in range(2):                                   # (the visibility read-back has thrown the next plan away: two frames queue one again)
            t.render(); t.read_rgba()
        assert t.plan_mode() & C.VF_PLAN_QUEUED_AHEAD
        t.set_plan_feedback(*pm.random_table(201, rig.n))    # a plan is queued ahead now: dropped here
        t.render()
        assert t.plan_mode() == C.VF_PLAN_FRESH | C.VF_PLAN_DILATE      # fresh at a resting camera: only the drop does that
        rig.compare()
        t.render()
        assert t.plan_mode() == 0
        rig.compare()
    finally:
        rig.close()


# ---- shards --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tiles0", "tiles1", "band1"])
def test_shards_under_random_tables(cabi, oracle, luts, layout):
    W, H, G = SMALL
    u = camera(oracle, "fill", W, H)
    ref_rgba, ref_vis = oracle_frame(oracle, luts, u, SMALL)
    ntx = (W + 63) // 64
    t = cabi.Terrain(W, H, G, luts["viridis"])
    try:
        t.set_height(heightmap(HEIGHT_SEED, G)); t.set_uniforms(u); t.set_shade_precision(EXACT)
        t.enable_timing(True)
        rank = int(layout[-1])
        if layout.startswith("tiles"):
            t.set_tile_shard(rank, 2, 0)
            lay = cabi.tile_layout(W, H, rank, 2, 0, lib=t.lib)
            tx, ty = lay[:, 0], lay[:, 1]
        else:
            t.set_shard(rank, 2, 64)
            rows = np.flatnonzero((np.arange(H) // 64) % 2 == rank)
            n = ntx * ((len(rows) + 63) // 64)
            tx, ty = np.arange(n) % ntx, np.arange(n) // ntx
        n = t.local_tiles()
        assert n == len(tx) and n >= 8
        full = pm.tile_widths(tx, W) == 64
        with pytest.raises(cabi.VfError):
            t.set_plan_feedback(np.ones(n, np.uint32))       # a new layout: back to the static estimate's frames
        t.render(); t.render()
        for seed in (300, 301, 302):
            words, lgs, pieces = pm.random_table(seed, n)
            t.set_plan_feedback(words, lgs, pieces)
            t.render()
            cuts = pm.items_to_cuts(t.item_stats()[:, 0], n)
            req = pm.request(words, lgs, pieces, tx, ty, W, ntx, (H + 63) // 64, False, cuts >= 0)      # shards: times at face value
            assert (cuts[~full] <= 0).all()
            pm.check_against_request(cuts, req)
            if layout.startswith("tiles"):
                tiles = t.read_tiles()
                for k in range(n):
                    want = ref_rgba[ty[k] * 64:(ty[k] + 1) * 64, tx[k] * 64:(tx[k] + 1) * 64]
                    assert np.array_equal(tiles[k][:want.shape[0], :want.shape[1]], want), (seed, k)
                    assert cuts[k] >= 0 or not (ref_vis[ty[k] * 64:(ty[k] + 1) * 64, tx[k] * 64:(tx[k] + 1) * 64] > 0).any()
            else:
                assert np.array_equal(t.read_rgba(), ref_rgba[rows]), seed
                assert np.array_equal(t.read_visibility(), ref_vis[rows]), seed
        assert t.plan_mode() == 0
    finally:
        t.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(cabi, oracle, luts):
    import ctypes as ct
    W, H, _ = SMALL
    u = camera(oracle, "fill", W, H)
    rig = Rig(cabi, oracle, luts, SMALL, u, warm=False)
    t = rig.t
    try:
        n = t.local_tiles()
        ones, lg0 = np.ones(n, np.uint32), np.zeros(n, np.uint8)
        mode = ct.c_uint32(77)
        assert t.lib.vf_terrain_debug_plan_mode(t.t, ct.byref(mode)) == cabi.VF_ERR_INVALID and mode.value == 77     # nothing rendered yet
        for frame in range(2):                               # a fresh handle, and one frame on: refused
            with pytest.raises(cabi.VfError, match="render two frames first"):
                t.set_plan_feedback(ones)
            t.render()
            assert t.plan_mode() == (cabi.VF_PLAN_FIRST, cabi.VF_PLAN_FRESH | cabi.VF_PLAN_DILATE)[frame]
        rig.compare()
        words = pm.uniform_cut_table(3, rig.tx, W)
        t.set_plan_feedback(words)                           # accepted: every full-width tile in 8 strips ...
        f = t.lib.vf_terrain_debug_set_plan_feedback
        bad_lg = lg0.copy(); bad_lg[-1] = 5
        assert f(None, ones.ctypes.data, lg0.ctypes.data, None, n) == cabi.VF_ERR_INVALID
        assert f(t.t, None, lg0.ctypes.data, None, n) == cabi.VF_ERR_INVALID
        assert f(t.t, ones.ctypes.data, None, None, n) == cabi.VF_ERR_INVALID
        assert f(t.t, ones.ctypes.data, lg0.ctypes.data, None, n - 1) == cabi.VF_ERR_INVALID
        assert f(t.t, ones.ctypes.data, bad_lg.ctypes.data, None, n) == cabi.VF_ERR_INVALID
        assert t.lib.vf_terrain_debug_plan_mode(t.t, None) == cabi.VF_ERR_INVALID
        assert t.lib.vf_terrain_debug_plan_mode(None, ct.byref(mode)) == cabi.VF_ERR_INVALID
        t.render()                                           # ... and the refused calls' all-ones tables have not replaced it
        cuts, _ = rig.compare()
        assert (cuts[(cuts >= 0) & rig.full] == 3).all()
        t.render()
        rig.compare()
    finally:
        rig.close()

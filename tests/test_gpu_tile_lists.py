"""Per-tile candidate lists (k_tile_lists): while a plan state's set-up records stand, the blocks that can reach each local
tile are listed once, off the frames' chain, and the tile kernel of later frames drawn from that state filters its tile's list instead
of testing the block ranges.  Scheduling and culling only: every frame below is held to the CPU oracle for the inputs it was drawn
from -- EXACT colour 0 LSB, visibility bit for bit -- never to a frame drawn the other way, and vf_terrain_debug_tile_lists says which
way it was drawn.

Settle: four frames of one view, each read back (a waiting caller: the lists of the state just drawn are queued behind the read-back's
copy).  The first two fill the two plan states, the next two reuse them and queue their lists; the fifth frame reads a list.

Shapes: 200 x 136 is four by three tiles with a partial tile in both directions; grid 33 is four blocks per side, grid 137 seventeen
with partial blocks in the last row and column."""
import ctypes as C

import numpy as np
import pytest

import plan_model as pm
from conftest import DEFAULT_CAMERA, FILL_CAMERA, heightmap
from support import cabi  # noqa: F401
from test_gpu_parity import EXACT

pytestmark = pytest.mark.gpu

SMALL = (200, 136)
CAM_B = ((-2.4, 1.1, 2.9), (0.1, 0.0, -0.2), (0.0, 1.0, 0.0), 55.0, 0.1, 100.0)
GRAZING = ((0.0, 0.5, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 0.1, 100.0)     # grid 2049: a tile on the horizon sees > 128 block rows
FAR = ((3.0, 6.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 30.0, 0.1, 100.0)         # grid 1025 inside one 64 x 64 tile: > 4096 entries in 128 rows
INSIDE = ((0.2, 0.0, 0.3), (0.0, 0.0, -0.5), (0.0, 1.0, 0.0), 60.0, 0.01, 100.0)    # the eye between the terrain's heights
NEAR_CUT = ((1.2, 0.4, 1.2), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 0.6, 100.0)    # the near plane cuts the terrain


_REF = {}


def reference(oracle, luts, u, W, H, G, h):
    key = (np.asarray(u, np.float32).tobytes(), W, H, G, h.tobytes())
    if key not in _REF:
        _REF[key] = oracle.render_terrain(u, W, H, G, h, luts["viridis"], nthreads=min(16, oracle.max_threads()))
    return _REF[key]


class View:
    """One handle of a waiting caller (render + read_rgba) and the inputs its frames are drawn from."""

    def __init__(self, cabi, oracle, luts, size, G, cam=DEFAULT_CAMERA, seed=11, stats=False, share_ctx=None):
        self.cabi, self.oracle, self.luts, self.G = cabi, oracle, luts, G
        self.W, self.H = size
        self.t = cabi.Terrain(self.W, self.H, G, luts["viridis"], share_ctx=share_ctx)
        self.t.set_shade_precision(EXACT)
        if stats:
            self.t.enable_timing(True)
        self.heights(heightmap(seed, G))
        self.pose(oracle.look_at_uniforms(1, self.W, self.H, *cam))
        self.tiles = None                                    # (rank, nranks, skew) of a tile shard

    def close(self):
        self.t.close()

    def pose(self, u):
        self.u = np.ascontiguousarray(u, np.float32)
        self.t.set_uniforms(self.u)

    def heights(self, h):
        self.h = np.ascontiguousarray(h, np.float32)
        self.t.set_height(self.h)

    def shard(self, rank, nranks, skew=3):
        self.tiles = (rank, nranks, skew)
        self.t.set_tile_shard(rank, nranks, skew)

    def frame(self):
        """one frame, read back; returns (colour as read, the query's answer for it)"""
        self.t.render()
        got = self.t.read_tiles() if self.tiles else self.t.read_rgba()
        return got, self.t.tile_lists()

    def settle(self, frames=4):
        for _ in range(frames):
            self.frame()

    def exact(self, used, visibility=True):
        """the next frame against the oracle; `used`: must it have read a list (True), must it not (False), either (None)"""
        got, info = self.frame()
        print(f"{self.W}x{self.H} grid {self.G}: {info}")
        if used is not None:
            assert info["used"] == used, info
        rgba, vis = reference(self.oracle, self.luts, self.u, self.W, self.H, self.G, self.h)
        if self.tiles:
            lay = self.cabi.tile_layout(self.W, self.H, *self.tiles, lib=self.t.lib)
            assert len(lay) == len(got)
            for (tx, ty), tile in zip(lay, got):
                want = rgba[ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64]
                d = int(np.abs(tile[:want.shape[0], :want.shape[1]].astype(np.int16) - want.astype(np.int16)).max(initial=0))
                assert d == 0, (int(tx), int(ty), d)
            return info
        d = int(np.abs(got.astype(np.int16) - rgba.astype(np.int16)).max(initial=0))
        assert d == 0, f"RGBA differs from the oracle by {d} LSB"
        if visibility:                                       # (a diagnostic frame in the other plan state: it reads that state's list too)
            bad = int((self.t.read_visibility() != vis).sum())
            assert bad == 0, f"visibility differs at {bad} pixels"
        return info

    def settled(self):
        """four frames, then: both plan states carry lists, and the next frames -- one from each state -- read them and are exact"""
        self.settle()
        a = self.exact(True, visibility=False)
        b = self.exact(True)
        for info in (a, b):
            assert info["built"] and info["tiles_fallback"] == 0, info
            assert info["tiles_listed"] == self.t.local_tiles(), info
        return b


def busy_rows_per_tile(vis, G):
    """per tile of the oracle's visibility: the span of block rows its visible primitives come from (a lower bound of the list's)"""
    nm1 = G - 1
    H, W = vis.shape
    spans = []
    for ty in range((H + 63) // 64):
        for tx in range((W + 63) // 64):
            v = vis[ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64].astype(np.int64)
            v = v[v > 0]
            if len(v):
                by = (v - 1) // 2 // nm1 // 8
                spans.append(int(by.max() - by.min() + 1))
    return spans


# ---- basic views ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", [DEFAULT_CAMERA, FILL_CAMERA], ids=["default", "fill"])
@pytest.mark.parametrize("G", [33, 137])
def test_settled_views_read_their_lists(cabi, oracle, luts, G, cam):
    v = View(cabi, oracle, luts, SMALL, G, cam)
    try:
        _, first = v.frame()
        assert not first["used"] and not first["built"], first      # a one-shot render builds nothing
        info = v.settled()
        assert info["entries"] > 0 and info["units_asked"] <= info["capacity"], info
    finally:
        v.close()


def test_the_switch_off_builds_nothing(cabi, oracle, luts, monkeypatch):
    monkeypatch.setenv("VF_NO_TILE_LISTS", "1")              # (read when the handle is created)
    v = View(cabi, oracle, luts, SMALL, 137)
    monkeypatch.delenv("VF_NO_TILE_LISTS")
    try:
        v.settle()
        for _ in range(2):
            info = v.exact(False)
            assert not info["built"] and info["tiles_listed"] == 0, info
    finally:
        v.close()


# ---- strips: every strip of a tile filters the tile's list ---------------------------------------------------------------------------
@pytest.mark.parametrize("cam", [DEFAULT_CAMERA, FILL_CAMERA], ids=["default", "fill"])
@pytest.mark.parametrize("k", [1, 4])
def test_strips_filter_the_tiles_list(cabi, oracle, luts, cam, k):
    v = View(cabi, oracle, luts, SMALL, 137, cam, stats=True)
    try:
        v.settle()
        ntx, nty = (v.W + 63) // 64, (v.H + 63) // 64
        tx = np.tile(np.arange(ntx), nty)
        full = pm.tile_widths(tx, v.W) == 64
        for _ in range(2):                                   # one frame from each plan state
            v.t.set_plan_feedback(pm.uniform_cut_table(k, tx, v.W))
            v.exact(True, visibility=False)
            cuts = pm.items_to_cuts(v.t.item_stats()[:, 0], ntx * nty)
            assert (cuts[(cuts >= 0) & full] == k).all() and (cuts >= 0)[full].any(), cuts
    finally:
        v.close()


# ---- frame sizes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(300, 200), (64, 64)], ids=["300x200", "64x64"])
def test_frame_sizes(cabi, oracle, luts, size):
    """a last tile column narrower than 64 pixels; a frame of one tile"""
    v = View(cabi, oracle, luts, size, 137)
    try:
        v.settled()
    finally:
        v.close()


# ---- shards: lists are per local tile ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["rank 1 of 3", "stripe map"])
def test_tile_shards(cabi, oracle, luts, layout):
    v = View(cabi, oracle, luts, SMALL, 137, FILL_CAMERA)
    try:
        if layout == "stripe map":
            v.shard(1, 2, cabi.register_stripe_map(np.array([1, 0, 0, 1], np.uint8), 0, 2))
        else:
            v.shard(1, 3)
        assert 0 < v.t.local_tiles() < 12
        v.settled()
    finally:
        v.close()


# ---- fallback: a buffer that holds no list, or some ----------------------------------------------------------------------------------
def test_tiles_that_do_not_fit_fall_back(cabi, oracle, luts):
    v = View(cabi, oracle, luts, SMALL, 137)
    try:
        whole = v.settled()
        assert whole["units_asked"] > 8
        v.t.set_tile_list_capacity(0)                        # nothing fits: every tile that a block reaches goes without
        v.settle()
        for _ in range(2):
            info = v.exact(True)                             # (the empty tiles' lists are lists)
            assert info["built"] and info["entries"] == 0 and info["capacity"] == 0, info
            assert info["tiles_fallback"] > 0 and info["tiles_listed"] + info["tiles_fallback"] == 12, info
        none = info
        v.t.set_tile_list_capacity(whole["units_asked"] // 2)   # some fit, whichever workgroups come first
        v.settle()
        for _ in range(2):
            info = v.exact(True)
            assert 0 < info["tiles_fallback"] < none["tiles_fallback"] and 0 < info["entries"] < whole["entries"], (info, none, whole)
            assert info["tiles_listed"] + info["tiles_fallback"] == 12, info
        v.t.set_tile_list_capacity()                         # the default again
        v.settle()
        info = v.exact(True)
        assert info["tiles_fallback"] == 0 and info["entries"] == whole["entries"], (info, whole)
    finally:
        v.close()


# ---- more than one chunk -------------------------------------------------------------------------------------------------------------
def test_more_than_128_block_rows_reach_a_tile(cabi, oracle, luts):
    G = 2049
    v = View(cabi, oracle, luts, SMALL, G, GRAZING)
    try:
        _, vis = reference(oracle, luts, v.u, v.W, v.H, G, v.h)
        spans = busy_rows_per_tile(vis, G)
        assert max(spans) > 128, spans                       # (the rows of the VISIBLE primitives alone: the list's span is no smaller)
        v.settled()
    finally:
        v.close()


def test_more_than_4096_entries_inside_128_rows(cabi, oracle, luts):
    G = 1025                                                 # 128 block rows: one chunk's worth of steps, several chunks' worth of entries
    v = View(cabi, oracle, luts, (64, 64), G, FAR)
    try:
        info = v.settled()
        assert info["tiles_listed"] == 1 and info["entries"] > 4096, info
    finally:
        v.close()


# ---- generic primitives reach the complete variant through the list ------------------------------------------------------------------
@pytest.mark.parametrize("cam", [INSIDE, NEAR_CUT], ids=["inside", "near plane"])
def test_clipped_primitives(cabi, oracle, luts, cam):
    v = View(cabi, oracle, luts, SMALL, 137, cam)
    try:
        _, vis = reference(oracle, luts, v.u, v.W, v.H, 137, v.h)
        assert (vis > 0).mean() > 0.1
        v.settled()
    finally:
        v.close()


# ---- invalidation --------------------------------------------------------------------------------------------------------------------
def test_geometry_changes_drop_the_lists_and_the_sun_does_not(cabi, oracle, luts):
    v = View(cabi, oracle, luts, SMALL, 137)
    try:
        v.settled()
        sun = v.u.copy(); sun[32:35] = (-0.3, 0.9, 0.2)
        v.pose(sun)                                          # shading only: the lists stay
        for _ in range(2):
            assert v.exact(True, visibility=False)["built"]
        v.pose(oracle.look_at_uniforms(1, v.W, v.H, *CAM_B))  # another view
        for _ in range(2):
            info = v.exact(False, visibility=False)          # both states are rebuilt: no list is read, none is left
            assert not info["built"], info
        v.settled()
        v.heights(heightmap(23, 137) * np.float32(1.5))      # other heights
        for _ in range(2):
            assert not v.exact(False, visibility=False)["built"]
        v.settled()
        v.shard(1, 2)                                        # another layout
        for _ in range(2):
            assert not v.exact(False, visibility=False)["built"]
        v.settled()
    finally:
        v.close()


def test_closing_a_handle_with_a_builder_queued(cabi, oracle, luts):
    for frames in (3, 4):                                    # the third and fourth frames queue the builders
        v = View(cabi, oracle, luts, SMALL, 137)
        for _ in range(frames):
            v.t.render()
        v.t.read_rgba()
        v.close()
    v = View(cabi, oracle, luts, SMALL, 137)                 # the device is still well: a settled view on a fresh handle
    try:
        v.settled()
    finally:
        v.close()


# ---- ordering: a frame that reads a list waits for its builder -----------------------------------------------------------------------
def test_frames_queued_behind_a_larger_handle_wait_for_their_lists(cabi, oracle, luts):
    """The pattern of test_gpu_geometry_reuse.py: frames back to back into device buffers, nothing waits until the end, and a larger
    handle on the same context goes first -- this handle's frames find the one before them in flight (plan streams: the builders run on
    the set-up stream beside the plan chain), and a frame that read a list not yet built would show."""
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    W, H = SMALL
    n, slots = 8, []
    for _ in range(n):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), W * H * 4) == 0
        slots.append(p.value)
    v = View(cabi, oracle, luts, SMALL, 137)
    busy = cabi.Terrain(2048, 2048, 1024, luts["viridis"], share_ctx=v.t)
    try:
        busy.set_uniforms(oracle.look_at_uniforms(1, 2048, 2048, *FILL_CAMERA))
        modes = []
        for k in range(n):
            v.t.set_output_device(slots[k])
            if k in (0, 4):
                for _ in range(4):
                    busy.render()
            v.t.render()
            modes.append(v.t.plan_mode(geometry=True))
        v.t.sync()
        info = v.t.tile_lists()
        print("modes", modes, info)
        assert info["built"] and info["used"], info
        assert not any(m & cabi.VF_PLAN_TILE_LISTS for m in modes[:4]) and all(m & cabi.VF_PLAN_TILE_LISTS for m in modes[4:]), modes
        rgba, _ = reference(oracle, luts, v.u, W, H, 137, v.h)
        for k in range(n):
            out = np.empty((H, W, 4), np.uint8)
            assert hip.hipMemcpy(out.ctypes.data, slots[k], out.nbytes, 2) == 0          # hipMemcpyDeviceToHost
            d = int(np.abs(out.astype(np.int16) - rgba.astype(np.int16)).max(initial=0))
            assert d == 0, (k, d)
    finally:
        busy.close()
        v.close()
        for p in slots:
            hip.hipFree(p)

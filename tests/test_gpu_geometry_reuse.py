"""Block boxes and set-up records are reused while the geometry inputs stand ("two generations").

A plan state's conservative boxes, ranges, segment list, block records, generic masks and vertex records are a pure function of the
geometry inputs -- view, projection, spacing, exaggeration, heights, shard layout -- and plan_frame rebuilds them only when one of those
changed (VF_PLAN_GEOMETRY_REUSED says when it did not).  Every sequence below is a list of frames on one handle; every frame is held to
the CPU oracle for the inputs it was drawn from -- EXACT colour 0 LSB, the one FAST frame of a sequence within RGBA_TOL -- never to
another frame of the library, and the reuse bit of every frame is asserted.

Visibility: reading it draws the frame again in the OTHER plan state, which would change the very sequence under test (the state it
fills is stamped).  So frame k's visibility is read on a handle of its own that replays frames 0 .. k and then reads it -- the frame's
colour was compared in the sequence itself, its visibility in the replay, both against the oracle.

Shapes: 200 x 136 is four by three tiles with a partial tile in both directions; grid 33 is four blocks per side and one set-up segment,
grid 137 is 17 blocks per side: two 16-block segments per row and a last row and column of partial blocks."""
import ctypes as C

import numpy as np
import pytest

import plan_model as pm
from conftest import DEFAULT_CAMERA, FILL_CAMERA, heightmap
from support import cabi  # noqa: F401
from test_gpu_parity import EXACT, FAST, RGBA_TOL

pytestmark = pytest.mark.gpu

W, H = 200, 136
NTX, NTY = (W + 63) // 64, (H + 63) // 64
GRIDS = (33, 137)
CAM_B = ((-2.4, 1.1, 2.9), (0.1, 0.0, -0.2), (0.0, 1.0, 0.0), 55.0, 0.1, 100.0)
REFERENCE, SPEC_T32 = 0, 1
FRAME_BYTES = W * H * 4
SLOTS = 16                        # device frames of a sequence that reads nothing back between its frames


@pytest.fixture(scope="module")
def hip(cabi):
    """the HIP runtime the library already loaded (matched by soname): device frames of the test's own"""
    lib = C.CDLL("libamdhip64.so.7")
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    lib.hipFree.argtypes = [C.c_void_p]
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return lib


_REF = {}


def reference(oracle, luts, st, G):
    """(rgba, vis) of the oracle for a frame's inputs: the rows of a band shard from the oracle's rank render, the tiles of a tile shard
    cut from its whole frame (it renders no tile shards), each made once"""
    shard = st["shard"]
    band = shard if shard and shard[0] == "band" else None
    key = (st["u"].tobytes(), st["h"].tobytes(), st["shade_mode"], G, band)
    if key not in _REF:
        kw = dict(rank=band[1], nranks=band[2], band_h=band[3]) if band else {}
        _REF[key] = oracle.render_terrain(st["u"], W, H, G, st["h"], luts["viridis"], nthreads=min(8, oracle.max_threads()),
                                          shade_mode=st["shade_mode"], **kw)
    rgba, vis = _REF[key]
    if band:
        rows = ((np.arange(H) // band[3]) % band[2]) == band[1]
        return rgba[rows], vis[rows]
    return rgba, vis


class Seq:
    """One handle and the frames drawn on it.  style: how the caller behaves between frames --
         "sync"      render + sync, no read-back (every frame into a device buffer of its own, read at the end)
         "readback"  render + read_rgba (a waiting caller: its plans are queued behind the read-back's copy)
         "queued"    frames back to back, nothing waits until the end (plan streams in use, plans made ahead)"""

    def __init__(self, cabi, hip, oracle, luts, G, style, h0=None, u0=None):
        self.cabi, self.hip, self.oracle, self.luts, self.G, self.style = cabi, hip, oracle, luts, G, style
        self.args = dict(h0=h0, u0=u0)
        self.t = cabi.Terrain(W, H, G, luts["viridis"])
        self.st = dict(u=None, h=None, shade_mode=REFERENCE, precision=EXACT, shard=None)
        self.frames = []                                     # (changes, inputs, host colour or slot, reuse bit, mode word)
        self.slots, self.dev_h, self.busy = [], None, None
        if style != "readback":                              # made now: an allocation between two frames would wait for the device
            for _ in range(SLOTS):
                p = C.c_void_p()
                assert hip.hipMalloc(C.byref(p), FRAME_BYTES) == 0
                self.slots.append(p.value)
        if style == "queued":
            # The plan streams are made for a caller whose frame arrives while the one before it is in flight.  A 4 x 3-tile frame is over
            # before the next call comes in, so a larger handle on the SAME context (and so the same stream) goes first: the first frames
            # of this handle queue behind its cold frames, and the second finds the first still waiting.
            self.busy = cabi.Terrain(2048, 2048, 1024, luts["viridis"], share_ctx=self.t)
            self.busy.set_uniforms(oracle.look_at_uniforms(1, 2048, 2048, *FILL_CAMERA))
        self.t.set_shade_precision(EXACT)
        self.apply(dict(h=heightmap(11, G) if h0 is None else h0, u=oracle.look_at_uniforms(1, W, H, *DEFAULT_CAMERA) if u0 is None else u0))

    def close(self):
        if self.busy is not None:
            self.busy.close()
        self.t.close()
        for p in self.slots:
            self.hip.hipFree(p)
        if self.dev_h:
            self.hip.hipFree(self.dev_h)
        self.slots, self.dev_h = [], None

    def apply(self, ch):
        t, st = self.t, self.st
        if "h" in ch:                                        # host heights: the library's own copy
            st["h"] = np.ascontiguousarray(ch["h"], np.float32); t.set_height(st["h"])
        if "h_dev" in ch:                                    # new values written THROUGH one device pointer, handed over again
            st["h"] = np.ascontiguousarray(ch["h_dev"], np.float32)
            t.sync()
            if not self.dev_h:
                p = C.c_void_p()
                assert self.hip.hipMalloc(C.byref(p), st["h"].nbytes) == 0
                self.dev_h = p.value
            assert self.hip.hipMemcpy(self.dev_h, st["h"].ctypes.data, st["h"].nbytes, 1) == 0         # hipMemcpyHostToDevice
            t.set_height_device(self.dev_h, st["h"].shape[1], st["h"].shape[0])
        if "u" in ch:
            st["u"] = np.ascontiguousarray(ch["u"], np.float32); t.set_uniforms(st["u"])
        if "shade_mode" in ch:
            st["shade_mode"] = ch["shade_mode"]; t.set_shade_mode(ch["shade_mode"])
        if "precision" in ch:
            st["precision"] = ch["precision"]; t.set_shade_precision(ch["precision"])
        if "shard" in ch:
            s = st["shard"] = ch["shard"]
            if s is None:
                t.set_shard(0, 1, 64)
            elif s[0] == "band":
                t.set_shard(s[1], s[2], s[3])
            else:
                t.set_tile_shard(s[1], s[2], s[3])
        if "timing" in ch:
            t.enable_timing(bool(ch["timing"]), stats=True)
        if "feedback" in ch:
            t.set_plan_feedback(*ch["feedback"])
        if ch.get("read_visibility"):                        # a diagnostic frame in front of this one: it plans in the other plan state
            _, vis = reference(self.oracle, self.luts, self.drawn, self.G)
            assert np.array_equal(t.read_visibility(), vis)

    def frame(self, reuse=None, **ch):
        """apply the changes, draw one frame, behave as the style says; returns the mode word (all bits)"""
        t = self.t
        self.apply(ch)
        tiles = self.st["shard"] is not None and self.st["shard"][0] == "tiles"
        got = None
        if self.style == "readback" or tiles:
            t.render()
            got = t.read_tiles() if tiles else t.read_rgba()
        else:
            got = len(self.frames)
            assert got < SLOTS
            t.set_output_device(self.slots[got])
            if self.busy is not None and got == 0:
                for _ in range(4):
                    self.busy.render()
            t.render()
            if self.style == "sync":
                t.sync()
        mode = t.plan_mode(geometry=True)
        self.drawn = dict(self.st)
        self.frames.append((dict(ch), self.drawn, got, t.geometry_reused(), mode))
        if reuse is not None:
            assert t.geometry_reused() == reuse, (len(self.frames), [f[3] for f in self.frames])
        return mode

    def colour(self, k):
        st, got = self.frames[k][1], self.frames[k][2]
        if isinstance(got, int):
            rows = self.t.local_rows() if st["shard"] else H
            out = np.empty((rows, W, 4), np.uint8)
            assert self.hip.hipMemcpy(out.ctypes.data, self.slots[got], out.nbytes, 2) == 0            # hipMemcpyDeviceToHost
            return out
        return got

    def check(self, visibility=True):
        """every frame's colour against the oracle for ITS inputs; then every frame's visibility, on handles that replay the frames"""
        self.t.sync()
        fast_frames = 0
        for k, (_, st, _, _, _) in enumerate(self.frames):
            rgba, _ = reference(self.oracle, self.luts, st, self.G)
            got = self.colour(k)
            if st["shard"] is not None and st["shard"][0] == "tiles":
                lay = self.cabi.tile_layout(W, H, st["shard"][1], st["shard"][2], st["shard"][3], lib=self.t.lib)
                assert len(lay) == len(got)
                for (tx, ty), tile in zip(lay, got):
                    want = rgba[ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64]
                    d = int(np.abs(tile[:want.shape[0], :want.shape[1]].astype(np.int16) - want.astype(np.int16)).max(initial=0))
                    assert d == 0, (k, int(tx), int(ty), d)
                continue
            d = int(np.abs(got.astype(np.int16) - rgba.astype(np.int16)).max(initial=0))
            print(f"frame {k + 1}: max |dRGBA| {d} LSB, precision {st['precision']}, reused {self.frames[k][3]}, mode {self.frames[k][4]}")
            fast = st["precision"] == FAST and st["shade_mode"] == REFERENCE
            fast_frames += fast
            assert d <= (RGBA_TOL if fast else 0), (k + 1, d)
        if visibility:
            for k in range(len(self.frames)):
                self.replay_visibility(k)
        return fast_frames

    def replay_visibility(self, k):
        st = self.frames[k][1]
        if st["shard"] is not None and st["shard"][0] == "tiles":
            return                                           # (a tile-major shard has no rows to read a visibility from)
        r = Seq(self.cabi, self.hip, self.oracle, self.luts, self.G, self.style, **self.args)
        try:
            for ch, _, _, reused, _ in self.frames[:k + 1]:
                r.frame(**ch)
                assert r.t.geometry_reused() == reused       # (the replay is the same sequence)
            _, vis = reference(self.oracle, self.luts, st, self.G)
            got = r.t.read_visibility()
            bad = int((got != vis).sum())
            assert bad == 0, f"frame {k + 1}: visibility differs at {bad} pixels"
        finally:
            r.close()


def uniforms(oracle, cam=DEFAULT_CAMERA, **kw):
    u = oracle.look_at_uniforms(1, W, H, *cam)
    for k, v in kw.items():
        if k == "sun":
            u[32:35] = v
        else:
            u[{"exposure": 35, "spacing": 36, "h_range": 37, "exag": 38}[k]] = v
    return u


# ---- rest ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", ["sync", "readback", "queued"])
@pytest.mark.parametrize("G", GRIDS)
def test_rest_reuses_from_the_third_frame_on(cabi, hip, oracle, luts, G, style):
    """Seven frames of one camera: each of the two plan states pays the full pass once, then both are reused.  A waiting caller with
    and without a read-back between the frames, and frames queued back to back (plan streams, plans made ahead)."""
    s = Seq(cabi, hip, oracle, luts, G, style)
    try:
        modes = [s.frame(reuse=k >= 2) for k in range(6)]
        modes.append(s.frame(reuse=True, precision=FAST))    # (a shading-only change: still reused)
        print(style, "modes:", modes)
        if style != "sync":                                  # a camera at rest: plans were made ahead and, reused, still are
            assert any(m & cabi.VF_PLAN_QUEUED_AHEAD and m & cabi.VF_PLAN_GEOMETRY_REUSED for m in modes), modes
        assert s.check() == 1
    finally:
        s.close()


# ---- shading-only changes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", ["readback", "queued"])
@pytest.mark.parametrize("G", GRIDS)
def test_shading_only_changes_keep_the_geometry_and_the_plan_made_ahead(cabi, hip, oracle, luts, G, style):
    """Sun, exposure, u[37], shade mode and precision between frames of a resting camera: the reuse bit stays set, a plan made ahead
    survives (VF_PLAN_QUEUED_AHEAD stays set) and the frame is the oracle's for the NEW values."""
    s = Seq(cabi, hip, oracle, luts, G, style)
    try:
        for k in range(4):
            s.frame(reuse=k >= 2)
        assert s.t.plan_mode() & cabi.VF_PLAN_QUEUED_AHEAD, "the fourth frame of a resting camera takes a plan made ahead"
        changes = [dict(u=uniforms(oracle, sun=(-0.3, 0.9, 0.2))), dict(u=uniforms(oracle, sun=(-0.3, 0.9, 0.2), exposure=1.7)),
                   dict(u=uniforms(oracle, sun=(-0.3, 0.9, 0.2), exposure=1.7, h_range=0.6)), dict(shade_mode=SPEC_T32),
                   dict(shade_mode=REFERENCE), dict(precision=FAST), dict(precision=EXACT, u=uniforms(oracle, sun=(0.9, 0.2, -0.1)))]
        for ch in changes:
            mode = s.frame(reuse=True, **ch)
            assert mode & cabi.VF_PLAN_QUEUED_AHEAD, (ch.keys(), mode)
        assert s.check() == 1
    finally:
        s.close()


# ---- geometry changes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["view", "projection", "spacing", "exaggeration"])
@pytest.mark.parametrize("G", GRIDS)
def test_a_geometry_change_pays_the_full_pass_on_exactly_two_frames(cabi, hip, oracle, luts, G, what):
    """A A A B A A A: going to B and coming back are two changes (a counter, not a hash); after each, each plan state pays once."""
    a = uniforms(oracle)
    b = {"view": uniforms(oracle, CAM_B), "spacing": uniforms(oracle, spacing=0.8), "exaggeration": uniforms(oracle, exag=1.6)}.get(what)
    if what == "projection":
        b = oracle.look_at_uniforms(1, W, H, *(DEFAULT_CAMERA[:3] + (52.0,) + DEFAULT_CAMERA[4:]))
        assert np.array_equal(a[:16], b[:16]) and not np.array_equal(a[16:32], b[16:32])
    s = Seq(cabi, hip, oracle, luts, G, "readback", u0=a)
    try:
        for k, (u, reuse) in enumerate([(a, False), (a, False), (a, True), (b, False), (a, False), (a, False), (a, True)]):
            s.frame(reuse=reuse, u=u)
        s.frame(reuse=True, precision=FAST)
        assert s.check() == 1
    finally:
        s.close()


# ---- heights -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["h", "h_dev"])
@pytest.mark.parametrize("G", GRIDS)
def test_new_heights_pay_the_full_pass(cabi, hip, oracle, luts, G, how):
    """set_height with other content of the same size; set_height_device with the SAME pointer after new values were written through
    it (a device copy of the test's own): the full pass runs on both plan states and the frames are the oracle's on the new heights."""
    s = Seq(cabi, hip, oracle, luts, G, "readback")
    try:
        s.frame(reuse=False, **{how: heightmap(21, G)})
        s.frame(reuse=False)
        s.frame(reuse=True)
        s.frame(reuse=False, **{how: heightmap(22, G) * np.float32(1.5)})
        s.frame(reuse=False)
        s.frame(reuse=True)
        s.frame(reuse=True, precision=FAST)
        assert s.check() == 1
    finally:
        s.close()


# ---- layout --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GRIDS)
def test_a_new_shard_layout_pays_the_full_pass(cabi, hip, oracle, luts, G):
    """Tile shard rank 0 -> 1 of 2, a registered stripe map, row bands, and back to the whole frame: k_block_boxes drops the blocks of
    the other rank's tiles, so every layout fills both plan states anew."""
    word = cabi.register_stripe_map(np.array([1, 0, 0, 1], np.uint8), 0, 2)
    s = Seq(cabi, hip, oracle, luts, G, "readback", u0=uniforms(oracle, FILL_CAMERA))
    try:
        for k in range(3):
            s.frame(reuse=k >= 2)
        for shard in (("tiles", 0, 2, 0), ("tiles", 1, 2, 0), ("tiles", 1, 2, word), ("band", 1, 2, 64), None):
            s.frame(reuse=False, shard=shard)
            s.frame(reuse=False)
            s.frame(reuse=True)
        s.frame(reuse=True, precision=FAST)
        assert s.check() == 1
    finally:
        s.close()


# ---- diagnostics and feedback between reused frames ----------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GRIDS)
def test_a_visibility_frame_between_reused_frames(cabi, hip, oracle, luts, G):
    """render_visibility plans in the other plan state: that state's geometry stands too, the diagnostic frame is the oracle's and the
    frames around it stay reused.  With uniforms of OTHER geometry set since the frame was drawn, the diagnostic frame is still the
    drawn frame's, and nothing built for it is taken for the live inputs."""
    s = Seq(cabi, hip, oracle, luts, G, "readback")
    try:
        for k in range(3):
            s.frame(reuse=k >= 2)
        s.frame(reuse=True, read_visibility=True)
        s.frame(reuse=True, read_visibility=True)
        # uniforms of other geometry are set, then the visibility is read: it is frame 5's (Seq.apply sets u before it reads)
        s.frame(reuse=False, read_visibility=True, u=uniforms(oracle, CAM_B))
        s.frame(reuse=False)
        s.frame(reuse=True, precision=FAST)
        assert s.check() == 1
    finally:
        s.close()


@pytest.mark.parametrize("G", GRIDS)
def test_injected_feedback_changes_the_cuts_not_the_geometry(cabi, hip, oracle, luts, G):
    """Two different cut tables on consecutive reused frames: the item codes follow the tables (the model of the cut rule), the geometry
    is reused, the frames are the oracle's."""
    n = NTX * NTY
    tx, ty = np.tile(np.arange(NTX), NTY), np.repeat(np.arange(NTY), NTX)
    s = Seq(cabi, hip, oracle, luts, G, "readback", u0=uniforms(oracle, FILL_CAMERA))
    try:
        s.frame(reuse=False, timing=True)
        s.frame(reuse=False)
        seen = []
        for lg in (3, 1):                                    # every full-width tile in 8 strips, then in 2
            words, lgs, pieces = pm.uniform_cut_table(lg, tx, W), np.zeros(n, np.uint8), np.zeros((n, 64), np.uint32)
            s.frame(reuse=True, feedback=(words, lgs, pieces))
            cuts = pm.items_to_cuts(s.t.item_stats()[:, 0], n)
            req = pm.request(words, lgs, pieces, tx, ty, W, NTX, NTY, True, cuts >= 0)
            pm.check_against_request(cuts, req)
            seen.append(cuts.copy())
        assert not np.array_equal(seen[0], seen[1]), "the two tables ask for different cuts"
        s.frame(reuse=True, precision=FAST)
        assert s.check() == 1
    finally:
        s.close()


@pytest.mark.parametrize("G", GRIDS)
def test_a_reused_frame_rasterises_the_blocks_of_a_fresh_one(cabi, hip, oracle, luts, G):
    """Timing level 1 statistics: blocks_rasterised of a reused frame equals that of the same frame drawn by the full pass on a fresh
    handle.  Both frames are fed one table of tile times, so that both are cut alike (an injection is accepted from a handle's third
    frame on, and that frame would be a reused one: the fresh handle is handed its heights again in front of it, which is a geometry
    change of the same content).

    The camera and the heights: blocks_rasterised counts the (tile, block) pairs left after the tile kernel's early-out, and the
    early-out asks whether every pixel of the block's box is final AT THE MOMENT a wave looks -- waves pull blocks asynchronously, so
    wherever one block row hides another the count differs from frame to frame with nothing changed (the parent commit, default
    camera over noise heights, ten identical frames: 63 every time at grid 33, 570 ... 585 at grid 137).  It is a function of the inputs
    where nothing hides anything: the top-down camera over the analytic surface alone (zero texture; slopes below 0.33 under rays steeper
    than 1.7), where a block's own pixels are never final before the block is drawn."""
    h = np.zeros((G, G), np.float32)
    u = uniforms(oracle, FILL_CAMERA)
    n = NTX * NTY
    tx = np.tile(np.arange(NTX), NTY)
    table = (pm.uniform_cut_table(2, tx, W), np.zeros(n, np.uint8), np.zeros((n, 64), np.uint32))
    pairs = {}
    for kind in ("reused", "fresh"):
        s = Seq(cabi, hip, oracle, luts, G, "readback", h0=h, u0=u)
        try:
            s.frame(reuse=False, timing=True)
            s.frame(reuse=False)
            if kind == "reused":
                s.frame(reuse=True)
                s.frame(reuse=True)
                s.frame(reuse=True, feedback=table)
            else:
                s.frame(reuse=False, h=h, feedback=table)
            pairs[kind] = int(s.t.timings()["blocks_rasterised"])
            s.frame(precision=FAST)
            assert s.check() == 1
        finally:
            s.close()
    print("blocks rasterised:", pairs)
    assert pairs["reused"] == pairs["fresh"] and pairs["reused"] > 0


@pytest.mark.parametrize("G", GRIDS)
def test_heights_in_device_memory_are_cached_before_the_second_frames_plan(cabi, hip, oracle, luts, G):
    """Heights handed over in device memory are cached by the next frame -- a handle's first, on the caller's stream.  The second
    frame's plan chain runs on the plan streams and has no event of its plan state to wait for yet: it must still come after the
    rebuild, or its plan state is filled from the cache as it was (and, reused, stays so).  Queued behind a larger handle's frames
    the first frame has not started when the second is planned."""
    s = Seq(cabi, hip, oracle, luts, G, "queued")
    try:
        s.frame(reuse=False, h_dev=heightmap(31, G) * np.float32(1.4))
        s.frame(reuse=False)
        for _ in range(4):
            s.frame(reuse=True)
        s.frame(reuse=True, precision=FAST)
        assert s.check() == 1
    finally:
        s.close()

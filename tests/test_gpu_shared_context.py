"""Handles that share a context, drawn on several streams of the caller's with nothing waiting in between, at the C ABI
on one thread.  The context's plan streams are shared, a frame's host round trips (the flood's and the spill's fixpoint words, the
overlays' pair count, the contours' segment count) happen while the other handle's work sits on those streams, and a frame that
follows one of the same handle on another stream waits for that one's `drawn` event: a mistake in any of this shows as wrong
pixels, so every frame, plane and field is held to the oracle under the CPU models (tests/soak_handles.py: expected, field), bit for
bit, never to another frame of the library.

Each test shows that the order was needed: where work goes onto a second stream it asks hipStreamQuery about the first, and a run
that never hears "not ready" fails as vacuous.

`P`: 257 x 131 (5 x 3 tiles, partial in both directions), grid 130 (17 x 17 blocks, 3 x 3 flood / spill tiles, scans across a 64-step
chunk); the small ones 96 x 64.  `Q`, the filler: 2048 x 2048, grid 1024, the fill camera, no pass -- the handle
tests/test_gpu_tile_lists.py keeps a stream occupied with; here its frames are compared too."""
import numpy as np
import pytest

import soak_handles as sh
from support import cabi  # noqa: F401

pytestmark = pytest.mark.gpu

P_ON = ("shadows", "ambient", "flood", "spill")              # the relight pass; two fields that iterate to a fixpoint with the host in the loop
SUN_B, CAM_B = sh.SUNS[1], 3


@pytest.fixture
def hip():
    h = sh.Hip()
    yield h
    h.close()


@pytest.fixture(scope="module")
def memo():
    return {}                                                # the reference frames and vertex fields, shared by the tests of this module


def p_inputs(seed=21, layers=True):
    rng = np.random.default_rng(seed)
    x = sh.handle(rng, *sh.P_SIZE, sh.P_GRID, on=P_ON, cam=2)
    if layers:                                               # one occluding line layer (reads d_vis) and one contour layer: a pair count read back per frame
        x = sh.with_layer(x, sh.line_layer(rng, occlude=True))
        x = sh.with_layer(x, sh.contour_layer(x["h"], x["G"]))
    return x


def q_inputs():
    return sh.handle(np.random.default_rng(22), *sh.Q_SIZE, sh.Q_GRID, cam=2)


def assert_frame(hip, slot, x, memo, what):
    n, where = sh.differing(hip.read(slot, (x["H"], x["W"], 4)), sh.expected(x, memo)["frame"])
    assert n == 0, f"{what}: {n} pixels differ from the model, first at {where}"


def test_two_handles_on_two_streams_with_nothing_waiting_until_the_end(cabi, hip, oracle, memo):
    ROUNDS = 8
    xP, xQ = p_inputs(), q_inputs()
    sP, sQ = hip.stream(), hip.stream()
    slotP = [hip.slot(sh.frame_bytes(xP)) for _ in range(ROUNDS)]
    slotQ = [hip.slot(sh.frame_bytes(xQ)) for _ in range(ROUNDS)]
    P = sh.create(cabi, xP)
    Q = sh.create(cabi, xQ, share_ctx=P)
    drawn, modes, asked, busy = [], [], 0, 0
    try:
        for r in range(ROUNDS):
            if r == 4:                                       # a new sun: the shadow field is computed again while frames are in flight
                xP = sh.changed(xP, sun=SUN_B)
                P.set_uniforms(sh.uniforms(xP))
            if r == 6:                                       # another view: both plan states are rebuilt, no list is read
                xP = sh.changed(xP, cam=CAM_B)
                P.set_uniforms(sh.uniforms(xP))
            if r:
                asked, busy = asked + 1, busy + hip.busy(sP)  # Q's frame goes onto its stream: is P's last frame still on its own?
            Q.set_output_device(slotQ[r])
            Q.render(sQ)
            asked, busy = asked + 1, busy + hip.busy(sQ)      # P's frame goes onto its stream: is Q's still on its own?
            P.set_output_device(slotP[r])
            P.render(sP)
            modes.append(P.plan_mode(geometry=True))
            drawn.append(xP)
        P.sync()
        Q.sync()
        print(f"shared context, two streams: {busy} of {asked} times the other stream was not ready when work went onto this one; plan modes {modes}")
        for r in range(ROUNDS):
            assert_frame(hip, slotP[r], drawn[r], memo, f"P, round {r} (its stream; Q on the other)")
        for r in range(ROUNDS):
            assert_frame(hip, slotQ[r], xQ, memo, f"Q, round {r}")
        # the at-rest rule (tests/test_gpu_geometry_reuse.py, tests/test_gpu_tile_lists.py): both plan states are built by
        # frames 0 and 1 and reused from frame 2 on, the sun leaves them standing, the view of round 6 does not; a state's lists are
        # queued behind the frame that reused it first and read by that state's next frame
        reused = [bool(m & cabi.VF_PLAN_GEOMETRY_REUSED) for m in modes]
        lists = [bool(m & cabi.VF_PLAN_TILE_LISTS) for m in modes]
        assert reused == [False, False, True, True, True, True, False, False], modes
        assert lists == [False, False, False, False, True, True, False, False], modes
        assert busy > 0, f"vacuous: the other stream was idle all {asked} times work went onto a stream"
    finally:
        Q.close()
        P.close()


def test_one_handle_on_alternating_streams_and_device_reads_on_a_third(cabi, hip, oracle, memo):
    FRAMES = 6
    xP, xQ = p_inputs(seed=23, layers=False), q_inputs()
    xT = sh.handle(np.random.default_rng(24), *sh.P_SMALL, sh.P_GRID, on=("shadows", "flood"), supersample=2, cam=2)
    xT = sh.with_layer(xT, sh.contour_layer(xT["h"], xT["G"]))
    A, B, Cs = hip.stream(), hip.stream(), hip.stream()
    slots = [hip.slot(sh.frame_bytes(xP)) for _ in range(FRAMES + 1)]
    n = xP["G"]
    d_depth, d_prim = hip.slot(xP["W"] * xP["H"] * 4), hip.slot(xP["W"] * xP["H"] * 4)
    d_shadow, d_flood = hip.slot(n * n * 4), hip.slot(n * n * 4)
    d_samples, d_twin = hip.slot(4 * sh.frame_bytes(xT)), hip.slot(sh.frame_bytes(xT))
    P = sh.create(cabi, xP)
    Q = sh.create(cabi, xQ, share_ctx=P)
    T = sh.create(cabi, xT, share_ctx=P)
    drawn, asked, busy = [], 0, 0

    def alternate(k, into):
        nonlocal xP, asked, busy
        s, other = (A, B) if k % 2 == 0 else (B, A)
        xP = sh.changed(xP, sun=sh.SUNS[1 + k % 3])          # a new sun in between: no frame equals the one before it
        P.set_uniforms(sh.uniforms(xP))
        if k:
            asked, busy = asked + 1, busy + hip.busy(other)   # the frame goes onto `s`: is the one before it still on the other stream?
        P.set_output_device(into)
        P.render(s)
        return xP

    try:
        # the first frame computes the flood and the spill with the host in the loop; the six behind it queue without a host wait
        P.set_output_device(slots[FRAMES])
        P.render(A)
        first = xP
        for _ in range(4):                                   # four cold frames of the filler on A, the handle's frame behind them
            Q.render(A)
        for k in range(FRAMES):
            drawn.append(alternate(k, slots[k]))
        hip.wait(A)
        hip.wait(B)
        assert_frame(hip, slots[FRAMES], first, memo, "the first frame")
        for k in range(FRAMES):
            assert_frame(hip, slots[k], drawn[k], memo, f"frame {k} on stream {'AB'[k % 2]}, the one before it on the other")
        n_q, where = sh.differing(Q.read_rgba().reshape(xQ["H"], xQ["W"], 4), sh.expected(xQ, memo)["frame"])
        assert n_q == 0, f"the filler's own frame: {n_q} pixels differ, first at {where}"
        # again into the handle's own buffer, now under an occluding layer and contours (a host wait for the pair count inside every
        # frame; the composite that reads d_vis is the frame's tail): only the last frame is read back
        rng = np.random.default_rng(25)
        for layer in (sh.line_layer(rng, occlude=True), sh.contour_layer(xP["h"], xP["G"])):
            sh.add_layer(P, layer)
            xP = sh.with_layer(xP, layer)
        for _ in range(2):
            Q.render(B)
        for k in range(FRAMES):
            last = alternate(k + 1, None)
        # the twin's frame on A, then three device reads on a third stream with no host wait between them
        T.set_output_device(d_twin)
        T.render(A)
        asked, busy = asked + 1, busy + hip.busy(A)
        P.gbuffer_device(depth=d_depth, primitive=d_prim, stream=Cs)
        P.shadow_field_device(d_shadow, Cs)
        P.flood_field_device(d_flood, Cs)
        T.samples_device(d_samples, Cs)
        hip.wait(Cs)
        print(f"one handle, alternating streams: {busy} of {asked} times the other stream was not ready when work went onto this one")
        e = sh.expected(last, memo)
        n_f, where = sh.differing(P.read_rgba().reshape(last["H"], last["W"], 4), e["frame"])
        assert n_f == 0, f"the last frame in the handle's own buffer: {n_f} pixels differ, first at {where}"
        want = sh.planes(last, e["vis"])
        for name, slot, dtype in (("depth", d_depth, np.float32), ("primitive", d_prim, np.uint32)):
            n_p, where = sh.differing(hip.read(slot, (last["H"], last["W"]), dtype), want[name])
            assert n_p == 0, f"gbuffer plane {name} read on a third stream: {n_p} pixels differ, first at {where}"
        for name, slot in (("shadow", d_shadow), ("flood", d_flood)):
            n_v, where = sh.differing(hip.read(slot, (n, n), np.float32), sh.field(last, name))
            assert n_v == 0, f"{name} field read on a third stream: {n_v} vertices differ, first at {where}"
        eT = sh.expected(xT, memo)
        n_s, where = sh.differing(hip.read(d_samples, eT["samples"].shape), eT["samples"])
        assert n_s == 0, f"the twin's samples read on a third stream: {n_s} differ, first at {where}"
        T.sync()
        assert_frame(hip, d_twin, xT, memo, "the supersampled twin's frame")
        assert busy > 0, f"vacuous: the other stream was idle all {asked} times work went onto a stream"
    finally:
        T.close()
        Q.close()
        P.close()


def test_a_handle_closed_while_its_neighbour_has_frames_in_flight(cabi, hip, oracle, memo):
    xP = p_inputs()
    x2 = sh.handle(np.random.default_rng(26), *sh.P_SMALL, sh.P_GRID, on=("shadows", "viewshed"), cam=0)
    x3 = sh.handle(np.random.default_rng(27), *sh.P_SMALL, sh.P_GRID, on=("ambient", "spill", "haze"), cam=1)
    sP, s2 = hip.stream(), hip.stream()
    slotP = [hip.slot(sh.frame_bytes(xP)) for _ in range(5)]
    slot2 = [hip.slot(sh.frame_bytes(x2)) for _ in range(2)]
    slot3 = hip.slot(sh.frame_bytes(x3))
    P = sh.create(cabi, xP)
    P2 = P3 = None
    drawn = []

    def frame(k):
        nonlocal xP
        xP = sh.changed(xP, sun=sh.SUNS[k % len(sh.SUNS)])
        P.set_uniforms(sh.uniforms(xP))
        P.set_output_device(slotP[k])
        P.render(sP)
        drawn.append(xP)

    try:
        frame(0)
        P2 = sh.create(cabi, x2, share_ctx=P)
        P2.set_output_device(slot2[0])
        P2.render(s2)
        frame(1)
        P2.set_output_device(slot2[1])
        P2.render(s2)
        frame(2)
        P2.close()                                           # between two queued frames of its neighbour
        P2 = None
        frame(3)
        P3 = sh.create(cabi, x3, share_ctx=P)
        P3.set_output_device(slot3)
        P3.render(s2)
        frame(4)
        P.sync()
        P3.sync()
        for k in range(5):
            assert_frame(hip, slotP[k], drawn[k], memo, f"P, frame {k}")
        for k in range(2):
            assert_frame(hip, slot2[k], x2, memo, f"the handle that was closed, frame {k}")
        assert_frame(hip, slot3, x3, memo, "the handle made in its place")
    finally:
        for t in (P3, P2, P):
            if t is not None:
                t.close()

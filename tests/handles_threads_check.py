"""Handles of one context on several THREADS: the child process of tests/test_gpu_handle_threads.py, which starts it once
under a time limit and reads the lines it prints, one `CHECK <name> OK|FAIL <text>` per check.  At most four threads; every join has
a timeout, and a thread that does not come back ends the process with exit code 2 and a `HUNG` line (nothing is started after it).
Exit code 0: every check passed; 1: some check failed.

  abi      three threads, each with its own cabi.Terrain on the first one's context and its own stream, start from a barrier and draw
           six frames of their own scene into device slots; between frames each provokes a refusal of its own and reads the library's
           error text, which is per thread (include/vf_hip.h).  Every frame equals its model, every thread reads its own text only.
  pool     three threads, each with its own vulkan_forge.Scene of 1024 x 1024 (4 MiB frames: the smallest the process-wide pool of
           page-locked buffers serves), call render_rgba() five times under five suns and KEEP the arrays; all fifteen equal the oracle
           after the joins -- a pool buffer handed to two owners, or reused under a live array, shows.  Which arrays are page-locked
           is not asserted: the pool's allowance is the process's, and the threads race for it by design.
  borrow   one Scene; a thread calls render_batch(poses), the main thread polls set_exposure() of the same object until it returns:
           every poll returns or raises RuntimeError("Already borrowed"), at least one raises (none: `vacuous`), and the batch's
           first and last frames equal the oracle."""
import os
import sys
import threading
import time

import numpy as np

import soak_handles as sh
import support  # noqa: F401  (the repository root on sys.path)

JOIN_S = 60.0
FAILED = []


def report(name, ok, text):
    print(f"CHECK {name} {'OK' if ok else 'FAIL'} {text}", flush=True)
    if not ok:
        FAILED.append(name)


def join_all(threads, what):
    deadline = time.time() + JOIN_S
    for th in threads:
        th.join(max(0.0, deadline - time.time()))
    hung = [th.name for th in threads if th.is_alive()]
    if hung:
        print(f"HUNG {what}: {hung} did not come back within {JOIN_S:.0f} s", flush=True)
        os._exit(2)


def guarded(errors, fn):
    def body(*a):
        try:
            fn(*a)
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(f"{threading.current_thread().name}: {type(e).__name__}: {e}")
    return body


# ---- abi -------------------------------------------------------------------------------------------------------------------------------
FRAMES = 6
REFUSALS = ("no observer set (vf_terrain_set_viewshed)", "softness must be a finite number > 0", "reach must be a finite number in [1, 1024]")


def refuse(k, t):
    """thread k's own refusal -> the text the library left for this thread"""
    from vulkan_forge_amd import cabi
    if k == 0:
        try:
            t.viewshed_field()
        except cabi.VfError as e:
            return str(e)
        return "(no refusal)"
    if k == 1:
        rc = t.lib.vf_terrain_set_shadows(t.t, 1, 0.8, 0.0, 0.01)                  # softness = 0
    else:
        d = sh.sf._round(4)
        rc = t.lib.vf_terrain_set_ambient(t.t, 1, 0.6, 0.0, len(d), d.ctypes.data)  # reach = 0
    return t.lib.vf_last_error().decode() if rc != 0 else "(no refusal)"


def check_abi(oracle):
    from vulkan_forge_amd import cabi
    cabi.load()
    hip = sh.Hip()
    scenes = [sh.handle(np.random.default_rng(31), 257, 131, 130, on=("flood",), cam=2),
              sh.handle(np.random.default_rng(32), 96, 64, 130, on=("shadows",), cam=0),
              sh.handle(np.random.default_rng(33), 130, 3, 65, on=("ambient",), cam=3)]
    slots = [[hip.slot(sh.frame_bytes(x)) for _ in range(FRAMES)] for x in scenes]
    streams = [hip.stream() for _ in scenes]
    first = sh.create(cabi, scenes[0])
    first.clear_viewshed()                                   # (thread 0's refusal: a field without an observer)
    handles, texts, errors = [first, None, None], [[], [], []], []
    # (the inputs and uniform blocks of every frame are made here: the threads call nothing but the library)
    drawn = [[sh.changed(x, sun=sh.SUNS[(k + f) % len(sh.SUNS)]) for f in range(FRAMES)] for k, x in enumerate(scenes)]
    blocks = [[sh.uniforms(x) for x in xs] for xs in drawn]
    barrier = threading.Barrier(3, timeout=JOIN_S)

    def work(k):
        if k:
            handles[k] = sh.create(cabi, scenes[k], share_ctx=first)
        t = handles[k]
        barrier.wait()
        for f in range(FRAMES):
            t.set_uniforms(blocks[k][f])
            t.set_output_device(slots[k][f])
            t.render(streams[k])
            texts[k].append(refuse(k, t))
        t.sync()

    threads = [threading.Thread(target=guarded(errors, work), args=(k,), name=f"abi-{k}", daemon=True) for k in range(3)]
    for th in threads:
        th.start()
    join_all(threads, "abi")
    if errors:
        for name in ("abi_frames", "abi_error_text"):
            report(name, False, "; ".join(errors))
        return
    bad, memo = [], {}
    for k in range(3):
        for f in range(FRAMES):
            x = drawn[k][f]
            n, where = sh.differing(hip.read(slots[k][f], (x["H"], x["W"], 4)), sh.expected(x, memo)["frame"])
            if n:
                bad.append(f"thread {k} frame {f}: {n} pixels differ, first at {where}")
    report("abi_frames", not bad, "; ".join(bad) or f"{3 * FRAMES} frames of three threads equal their models")
    wrong = [f"thread {k} read {sorted(set(texts[k]))}" for k in range(3) if set(texts[k]) != {REFUSALS[k]}]
    report("abi_error_text", not wrong, "; ".join(wrong) or f"each of three threads read its own text {FRAMES} times")
    for t in reversed(handles):
        t.close()
    hip.close()


# ---- pool ------------------------------------------------------------------------------------------------------------------------------
POOL_SIZE, POOL_GRID, POOL_FRAMES = 1024, 128, 5


def check_pool(oracle):
    import vulkan_forge as vf
    import vulkan_forge_amd
    lut = vulkan_forge_amd.colormap_rgba8("viridis")
    kept, blocks, heights, errors = [[], [], []], [[], [], []], [], []
    for k in range(3):
        heights.append(sh.heights(np.random.default_rng(40 + k), (POOL_GRID + k, POOL_GRID + 2)))
    barrier = threading.Barrier(3, timeout=JOIN_S)

    def work(k):
        s = vf.Scene(POOL_SIZE, POOL_SIZE, grid=POOL_GRID)
        s.set_shade_precision("exact")
        s.set_height_from_r32f(heights[k])
        s.set_camera_look_at(*sh.CAMERAS[(k + 1) % len(sh.CAMERAS)])
        barrier.wait()
        for f in range(POOL_FRAMES):
            s.set_sun(15.0 + 11.0 * f + 3.0 * k, 40.0 * f + 100.0 * k)
            blocks[k].append(np.array(s.debug_uniforms_f32(), np.float32))
            kept[k].append(s.render_rgba())                   # (kept: the pool must not hand this buffer out again)

    threads = [threading.Thread(target=guarded(errors, work), args=(k,), name=f"pool-{k}", daemon=True) for k in range(3)]
    for th in threads:
        th.start()
    join_all(threads, "pool")
    if errors:
        report("pool_frames", False, "; ".join(errors))
        return
    bad = []
    for k in range(3):
        for f in range(POOL_FRAMES):
            want, _ = oracle.render_terrain(blocks[k][f], POOL_SIZE, POOL_SIZE, POOL_GRID, heights[k], lut, nthreads=min(16, oracle.max_threads()))
            n, where = sh.differing(kept[k][f], want.reshape(POOL_SIZE, POOL_SIZE, 4))
            if n:
                bad.append(f"thread {k} array {f}: {n} pixels differ, first at {where}")
    report("pool_frames", not bad, "; ".join(bad) or f"{3 * POOL_FRAMES} kept arrays of three threads equal the oracle")


# ---- borrow ------------------------------------------------------------------------------------------------------------------------------
BORROW_SIZE, BORROW_GRID, POSES = (640, 480), 256, 64


def check_borrow(oracle):
    import vulkan_forge as vf
    import vulkan_forge_amd
    W, H = BORROW_SIZE
    lut = vulkan_forge_amd.colormap_rgba8("viridis")
    h = sh.heights(np.random.default_rng(50), (BORROW_GRID, BORROW_GRID))
    s = vf.Scene(W, H, grid=BORROW_GRID)
    s.set_shade_precision("exact")
    s.set_height_from_r32f(h)
    poses = [((2.2 * np.cos(a), 1.4, 2.2 * np.sin(a)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0) for a in np.linspace(0.2, 2.9, POSES)]
    poses = [(tuple(float(v) for v in e), t, up, f, zn, zf) for e, t, up, f, zn, zf in poses]
    ends = []
    for p in (poses[-1], poses[0]):                          # the uniform blocks of the first and the last pose, from the object itself
        s.set_camera_look_at(*p)
        ends.append(np.array(s.debug_uniforms_f32(), np.float32))
    u_last, u_first = ends
    exposure = float(u_first[35])
    going, out, errors = threading.Event(), {}, []

    def work():
        going.set()
        t0 = time.perf_counter()
        out["frames"] = s.render_batch(poses)
        out["seconds"] = time.perf_counter() - t0

    th = threading.Thread(target=guarded(errors, work), name="borrow", daemon=True)
    th.start()
    if not going.wait(JOIN_S):
        print("HUNG borrow: the thread never started", flush=True)
        os._exit(2)
    polls = raised = 0
    other = []
    t0 = time.perf_counter()
    while th.is_alive() and time.perf_counter() - t0 < JOIN_S:
        polls += 1
        try:
            s.set_exposure(exposure)
        except RuntimeError as e:
            if type(e) is RuntimeError and str(e) == "Already borrowed":
                raised += 1
            else:
                other.append(f"{type(e).__name__}: {e}")
    polled = time.perf_counter() - t0
    join_all([th], "borrow")
    if errors:
        for name in ("borrow_guard", "borrow_frames"):
            report(name, False, "; ".join(errors))
        return
    period = polled / max(polls, 1)
    text = (f"render_batch of {POSES} poses took {1e3 * out['seconds']:.1f} ms; {polls} polls of set_exposure, one every {1e6 * period:.1f} us, {raised} raised "
            f"'Already borrowed'")
    ok = not other and raised >= 1 and out["seconds"] >= 50.0 * period
    if raised == 0:
        text = "vacuous: no poll met the borrow; " + text
    report("borrow_guard", ok, text + ("; other errors: " + "; ".join(other[:3]) if other else ""))
    bad = []
    for name, k, u in (("first", 0, u_first), ("last", POSES - 1, u_last)):
        want, _ = oracle.render_terrain(u, W, H, BORROW_GRID, h, lut, nthreads=min(16, oracle.max_threads()))
        n, where = sh.differing(np.asarray(out["frames"][k]), want.reshape(H, W, 4))
        if n:
            bad.append(f"the {name} frame: {n} pixels differ, first at {where}")
    s.set_exposure(exposure)                                 # the borrow went back
    report("borrow_frames", not bad, "; ".join(bad) or "the first and the last frame of the polled batch equal the oracle")


def main():
    import oracle                                            # (built by the suite's session fixture, as the library is)
    for check, names in ((check_abi, ("abi_frames", "abi_error_text")), (check_pool, ("pool_frames",)), (check_borrow, ("borrow_guard", "borrow_frames"))):
        t0 = time.time()
        try:
            check(oracle)
        except Exception as e:  # noqa: BLE001 - a check that raised has failed; the next one still runs
            for name in names:
                report(name, False, f"{type(e).__name__}: {e}")
        print(f"({check.__name__}: {time.time() - t0:.1f} s)", flush=True)
    return 1 if FAILED else 0


if __name__ == "__main__":
    sys.exit(main())

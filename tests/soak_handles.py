"""Handles together: several handles of ONE context, drawn on several streams of the caller's with their work
interleaved, every frame and field held to the CPU models.  The library of tests/test_gpu_shared_context.py, tests/handles_threads_check.py,
tests/test_gpu_handle_soak.py (the GPU slice) and tests/test_handle_soak_cases.py (the slice is not vacuous; CPU only), and a script.
A sibling of tests/soak_features.py: test infrastructure, nothing of it is shipped.  Every comparison is equality against the oracle's
frame under supersample_model.chain (the library's order of passes) and the overlay models; never against another run of the library.

    handle(rng, W, H, G, ...)     the inputs of one handle: sizes, heights, camera, sun, the parameters of every pass of kFramePassTable,
                                  which of them are on, the overlay layers
    apply(t, inp), set_pass(...)  those inputs on a cabi.Terrain
    expected(inp, memo)           the frame and visibility the handle must show; field(inp, name) a per-vertex field
    Hip                           the few runtime calls the tests make themselves: device slots, streams of the caller's, stream queries
    case(seed)                    a seeded interleaving: handles, streams and operations -- pure numpy, no GPU, no oracle
    run_case(c)                   the GPU side of one case -> mismatches; run(first, cases, budget) a window of seeds

usage: soak_handles.py [first_seed] [cases] [time_budget_s]"""
import ctypes as C
import sys
import time

import numpy as np

import model_support  # noqa: F401  (first: the repository root and the model directories on sys.path)
import ambient_model as abm
import contour_model as cm
import cumulative_viewshed_model as cvm
import flood_model as fdm
import gbuffer_model as gbm
import occlusion_model as ocm
import shadow_model as shm
import soak_features as sf
import spill_model as spm
import sun_exposure_model as sem
import supersample_model as ssm
import viewshed_model as vsm

f32 = np.float32
EXACT = 0
NOT_READY = 600                                               # hipErrorNotReady: what hipStreamQuery says of a stream with work in flight
PASSES = ("shadows", "ambient", "drape", "flood", "spill", "exposure", "cumulative", "viewshed", "haze")      # kFramePassTable, in its order
FIELDS = ("shadow", "sky", "flood", "spill", "exposure", "cumulative", "viewshed")
CAMERAS = (((1.8, 1.3, 1.8), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0),
           ((-1.5, 0.8, 1.9), (0.1, 0.0, -0.2), (0.0, 1.0, 0.0), 55.0, 0.1, 100.0),
           ((0.0, 2.2, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 60.0, 0.1, 100.0),
           ((1.3, 0.7, -1.6), (0.0, 0.0, 0.1), (0.0, 1.0, 0.0), 50.0, 0.1, 100.0))
SUNS = ((0.9, 0.5, 0.31), (-0.31, 0.4, 0.9), (0.2, 0.3, -0.9), (-0.8, 0.25, -0.4), (0.5, 1.0, 0.3))
SCAN = dict(eye_height=0.4, target_height=0.02, softness=0.05, bias=0.01)
P_SIZE, P_SMALL, P_GRID = (257, 131), (96, 64), 130           # the `P` handles of DESIGN.md 5f: 5 x 3 tiles; 17 x 17 blocks, 3 x 3 flood / spill tiles
Q_SIZE, Q_GRID = (2048, 2048), 1024                           # the filler: the handle tests/test_gpu_tile_lists.py keeps a stream occupied with


def lut():
    return sf.lut("viridis")


# ---- the inputs of a handle --------------------------------------------------------------------------------------------------------------
def heights(rng, shape):
    return (rng.random(shape, dtype=f32) * f32(0.6) - f32(0.3)).astype(f32)


def pass_params(rng, h, G):
    """the parameters of every pass, as supersample_model.chain takes them, for heights `h` on grid G (the flood's level: the median of
    the surface, so that part of the ground floods from the border)"""
    surf = cm.surface(h, G)
    obs = rng.uniform(-1.4, 1.4, (3, 2)).astype(f32)
    return dict(
        shadows=dict(strength=0.8, softness=0.05, bias=0.01),
        ambient=dict(strength=0.6, reach=float(rng.choice([5.0, 8.0])), directions=sf._round(4)),
        drape=dict(image=sf.drape_image(rng, int(rng.choice([7, 37])), int(rng.choice([3, 16])), 4), extent=(-1.1, -0.8, 0.9, 1.2), opacity=0.7, filter="linear"),
        flood=dict(level=fdm.field_level(surf, float(rng.choice([0.4, 0.5, 0.6]))), seeds="edges", shallow_rgba=(96, 176, 224, 128), deep_rgba=(16, 64, 160, 224),
                   depth_full=0.1),
        spill=dict(seeds="edges", shallow_rgba=(224, 96, 176, 160), deep_rgba=(160, 16, 64, 224), depth_full=0.05),
        exposure=dict(suns=np.array([shm.sun_vector(12.0, 70.0), shm.sun_vector(40.0, 200.0), shm.sun_vector(-5.0, 10.0)], f32), weights=None, incidence=True,
                      softness=0.05, bias=0.01, high_rgba=(255, 208, 64, 160), low_rgba=(0, 0, 64, 96)),
        cumulative=dict(observers=obs, radius=None, high_rgba=(64, 255, 96, 160), low_rgba=(0, 0, 0, 0), **SCAN),
        viewshed=dict(observer=(float(obs[0, 0]), float(obs[0, 1])), radius=None, visible_rgba=(64, 255, 96, 96), hidden_rgba=(255, 32, 32, 96), **SCAN),
        haze=dict(density=0.5, rgba=(200, 215, 235, 255), start=0.0, falloff=None, base=0.0, max_opacity=1.0, background=False))


def line_layer(rng, occlude=True):
    n = int(rng.integers(3, 7))
    path = np.column_stack([rng.uniform(-1.4, 1.4, n), rng.uniform(0.0, 0.3, n), rng.uniform(-1.4, 1.4, n)]).astype(f32)
    return ("lines", dict(paths=[path], width_px=float(rng.choice([2.0, 7.0])), rgba=(255, 64, 32, 255), cap="round", drape=False, occlude=occlude, depth_bias=1e-2))


def contour_layer(h, G, count=4):
    fin = cm.surface(h, G)
    lv = np.linspace(float(fin.min()), float(fin.max()), count + 2)[1:-1].astype(f32)
    return ("contours", dict(levels=lv, width_px=1.0, rgba=(16, 16, 16, 255), lift=0.0, join="round", occlude=False, depth_bias=1e-2))


def handle(rng, W, H, G, on=(), supersample=1, tex=None, cam=0):
    """The inputs of a handle.  `on`: the passes that are on; `params` holds every pass's parameters, on or off (the setters store
    them either way, and the fields can be read either way); `layers`: [(kind, keywords, the heights the layer was added under)]."""
    h = heights(rng, tex or (G + 1, G + 3))
    return dict(W=W, H=H, G=G, ss=supersample, h=h, cam=cam, sun=SUNS[0], params=pass_params(rng, h, G), on=tuple(p for p in PASSES if p in on), layers=[])


def changed(inp, **kw):
    """a copy of the inputs with some replaced (the arrays are never written to: a copy shares them)"""
    out = dict(inp, **kw)
    out["layers"] = list(out["layers"])
    return out


def with_layer(inp, layer):
    return changed(inp, layers=inp["layers"] + [(layer[0], layer[1], inp["h"])])


def uniforms(inp):
    """the handle's uniform block (the oracle's own arithmetic for the camera)"""
    import oracle
    u = np.array(oracle.look_at_uniforms(1, inp["W"], inp["H"], *CAMERAS[inp["cam"]]), f32).reshape(44)
    u[32:35] = inp["sun"]
    return u


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
def features(inp):
    return {p: (dict(inp["params"][p]) if p in inp["on"] else None) for p in PASSES}


def model_layers(inp, u, occluding=True):
    L = cm.Layers()
    for kind, kw, h_then in inp["layers"]:
        kw = dict(kw) if occluding else dict(kw, occlude=False)
        if kind == "lines":
            L.lines(kw["paths"], **{a: v for a, v in kw.items() if a != "paths"})
        else:                                                 # (the snapshot rule of vf_terrain_add_contours: the heights of the moment it was added)
            L.contours(h_then, inp["G"], u, kw["levels"], **{a: v for a, v in kw.items() if a != "levels"})
    return L


def expected(inp, memo=None):
    """-> dict frame (H, W, 4), vis and, for a supersampled handle, samples (f H, f W, 4): the oracle's frame at the sample size, the
    passes in the library's order (supersample_model.chain), the resolve, the overlays.  `memo`: a dict that keeps the vertex fields
    and the results for a caller that asks again."""
    import oracle
    u, f, W, H, G, h = uniforms(inp), inp["ss"], inp["W"], inp["H"], inp["G"], inp["h"]
    key = ("frame", u.tobytes(), f, W, H, G, h.shape, h.tobytes(), inp["on"], ssm._key(inp["params"]), ssm._key([(k, kw, x.tobytes()) for k, kw, x in inp["layers"]]))
    if memo is not None and key in memo:
        return memo[key]
    rgba, vis = oracle.render_terrain(u, f * W, f * H, G, h, lut(), want_vis=True, nthreads=min(8, oracle.max_threads()))
    st = {}
    s = ssm.chain(rgba.reshape(f * H, f * W, 4), vis, u, h, G, lut(), stages=st, memo=memo, **features(inp))
    frame = ssm.resolve(s, f)
    if inp["layers"]:
        frame = ocm.composite(frame, vis if f == 1 else np.zeros((H, W), np.uint32), u, h, G, model_layers(inp, u, occluding=f == 1))
    out = dict(frame=frame, vis=vis, samples=s, u=u)
    if memo is not None:
        memo[key] = out
    return out


def field(inp, name):
    """a per-vertex field of the handle's inputs (its pass on or off: the parameters are stored either way), (n, n) float32"""
    u, h, G, P = uniforms(inp), inp["h"], inp["G"], inp["params"]
    if name == "shadow":
        return shm.field(u, h, G, **P["shadows"])
    if name == "sky":
        return abm.field(u, h, G, P["ambient"]["directions"], P["ambient"]["reach"])
    if name == "flood":
        return fdm.field(u, h, G, P["flood"]["level"], P["flood"]["seeds"]).depth
    if name == "spill":
        return spm.field(u, h, G, P["spill"]["seeds"]).spill
    if name == "exposure":
        X = P["exposure"]
        return sem.field(u, h, G, X["suns"], X["weights"], incidence=X["incidence"], softness=X["softness"], bias=X["bias"])
    if name == "cumulative":
        return cvm.field(u, h, G, P["cumulative"]["observers"], radius=P["cumulative"]["radius"], **SCAN)[0]
    assert name == "viewshed", name
    return vsm.field(u, h, G, P["viewshed"]["observer"], **SCAN)[0]


def planes(inp, vis):
    depth, position, normal = gbm.planes(vis, uniforms(inp), inp["h"], inp["G"])
    return dict(depth=depth, position=position, normal=normal, primitive=vis)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def differing(got, want):
    """(count, first positions) of the pixels or vertices at which two arrays differ bit for bit"""
    d = np.ascontiguousarray(got).view(np.uint8).reshape(want.shape[:2] + (-1,)) != np.ascontiguousarray(want).view(np.uint8).reshape(want.shape[:2] + (-1,))
    d = d.any(axis=2)
    return int(d.sum()), np.argwhere(d)[:4].tolist()


# ---- the inputs on a handle --------------------------------------------------------------------------------------------------------------
def set_pass(t, inp, p):
    """pass `p` on the handle as the inputs have it: on or off, with its parameters either way"""
    on, P = p in inp["on"], inp["params"][p]
    if p == "shadows":
        t.set_shadows(on, **P)
    elif p == "ambient":
        t.set_ambient_occlusion(on, **P)
    elif p == "drape":
        if on:
            t.set_drape(P["image"], extent=P["extent"], opacity=P["opacity"], filter=P["filter"])
        else:
            t.clear_drape()
    elif p == "flood":
        t.set_flood(P["level"], P["seeds"], enabled=on, **{k: P[k] for k in ("shallow_rgba", "deep_rgba", "depth_full")})
    elif p == "spill":
        t.set_spill(P["seeds"], enabled=on, **{k: P[k] for k in ("shallow_rgba", "deep_rgba", "depth_full")})
    elif p == "exposure":
        t.set_sun_exposure(P["suns"], enabled=on, **{k: v for k, v in P.items() if k != "suns"})
    elif p == "cumulative":
        t.set_cumulative_viewshed(P["observers"], enabled=on, **{k: v for k, v in P.items() if k != "observers"})
    elif p == "viewshed":
        t.set_viewshed(P["observer"], enabled=on, **{k: v for k, v in P.items() if k != "observer"})
    else:
        t.set_haze(P["density"], enabled=on, **{k: v for k, v in P.items() if k != "density"})


def add_layer(t, layer):
    kind, kw = layer[0], layer[1]
    if kind == "lines":
        offs = np.concatenate([[0], np.cumsum([len(p) for p in kw["paths"]])]).astype(np.uint32)
        k = t.add_lines(np.concatenate(kw["paths"]), offs, width_px=kw["width_px"], rgba=kw["rgba"], cap=sf.CAPS.index(kw["cap"]), drape=kw["drape"])
        if kw["occlude"]:
            t.set_layer_occlusion(k, True, kw["depth_bias"])
    else:
        t.add_contours(kw["levels"], width_px=kw["width_px"], rgba=kw["rgba"], lift=kw["lift"], join=sf.JOINS.index(kw["join"]), occlude=kw["occlude"],
                       depth_bias=kw["depth_bias"])


def apply(t, inp):
    """all of the inputs on a fresh handle (layers that were added under other heights than the inputs hold now cannot be: the caller
    drops them first)"""
    t.set_shade_precision(EXACT)
    t.set_height(inp["h"])
    t.set_uniforms(uniforms(inp))
    for p in PASSES:
        set_pass(t, inp, p)
    for layer in inp["layers"]:
        assert layer[2] is inp["h"]
        add_layer(t, layer)


def create(cabi, inp, share_ctx=None):
    t = cabi.Terrain(inp["W"], inp["H"], inp["G"], lut(), share_ctx=share_ctx, supersample=None if inp["ss"] == 1 else inp["ss"])
    apply(t, inp)
    return t


# ---- the runtime calls the tests make themselves -----------------------------------------------------------------------------------------
class Hip:
    """Device slots made up front, streams of the caller's (non-blocking: no implicit order with the NULL stream), stream queries."""
    NON_BLOCKING = 1

    def __init__(self):
        self.lib = lib = C.CDLL("libamdhip64.so.7")
        lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        lib.hipFree.argtypes = [C.c_void_p]
        lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        lib.hipStreamDestroy.argtypes = [C.c_void_p]
        lib.hipStreamQuery.argtypes = [C.c_void_p]
        lib.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.slots, self.streams = [], []

    def slot(self, nbytes):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), max(int(nbytes), 4)) == 0
        assert self.lib.hipMemset(p, 0xA5, max(int(nbytes), 4)) == 0      # (no frame and no field reads like this filling)
        self.slots.append(p.value)
        return p.value

    def stream(self):
        s = C.c_void_p()
        assert self.lib.hipStreamCreateWithFlags(C.byref(s), self.NON_BLOCKING) == 0
        self.streams.append(s.value)
        return s.value

    def busy(self, stream):
        """is work still in flight on `stream`?  ("not ready" is an answer, not an error: it is cleared)"""
        rc = self.lib.hipStreamQuery(stream)
        if rc == NOT_READY:
            self.lib.hipGetLastError()
            return True
        assert rc == 0, f"hipStreamQuery: {rc}"
        return False

    def wait(self, stream):
        assert self.lib.hipStreamSynchronize(stream) == 0

    def read(self, slot, shape, dtype=np.uint8):
        out = np.empty(shape, dtype)
        assert self.lib.hipMemcpy(out.ctypes.data, slot, out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
        return out

    def close(self):
        for p in self.slots:
            self.lib.hipFree(p)
        for s in self.streams:
            self.lib.hipStreamDestroy(s)
        self.slots, self.streams = [], []


def frame_bytes(inp):
    return inp["W"] * inp["H"] * 4


# ---- the seeded interleaving ---------------------------------------------------------------------------------------------------------------
KINDS = ("render", "uniforms_same", "uniforms_shading", "uniforms_camera", "height", "toggle_pass", "toggle_layer", "field_host", "field_device", "read_rgba",
         "recreate")
_LOTS = dict(render=9.0, uniforms_same=0.7, uniforms_shading=1.2, uniforms_camera=1.0, height=0.7, toggle_pass=1.6, toggle_layer=0.8, field_host=0.7,
             field_device=0.9, read_rgba=0.8, recreate=0.5)
# operations during which the host may wait for the device (a field read into device memory computes the field first, and waits for it)
HOST_WAITS = ("height", "toggle_layer", "field_host", "field_device", "read_rgba", "recreate")
SHAPES = ((P_SIZE, 130), (P_SMALL, 130), ((130, 3), 65), ((200, 136), 33), ((64, 64), 17), (P_SMALL, 33), (P_SIZE, 65))
STREAM = 0x5EED5


def case(seed):
    """A case: dict name, handles (the inputs each starts from), streams (how many), ops.  An op: dict kind, h (the handle), and by kind
    s (a stream), field, inputs (what the handle holds behind the op: what a frame or a field produced by it is compared with), layer,
    p (the pass toggled).  Handle 0 owns the context and is never closed before the end."""
    rng = np.random.default_rng([seed, STREAM])
    nh, ns = int(rng.integers(2, 4)), int(rng.integers(2, 4))
    shapes = [SHAPES[i] for i in rng.choice(len(SHAPES), nh, replace=seed % 3 == 0)]
    state = []
    for (W, H), G in shapes:
        on = [p for p in PASSES if rng.random() < 0.3] or [str(rng.choice(PASSES))]
        state.append(handle(rng, W, H, G, on=on, cam=int(rng.integers(0, len(CAMERAS)))))
    first = [changed(x) for x in state]
    nops = int(rng.integers(12, 21))
    ops, rendered = [], [False] * nh
    kinds, lots = list(KINDS), np.array([_LOTS[k] for k in KINDS])
    while len(ops) < nops:
        k = str(rng.choice(kinds, p=lots / lots.sum()))
        h = int(rng.integers(0, nh))
        left = nops - len(ops)
        owed = [j for j in range(nh) if not rendered[j]]
        if owed and left <= len(owed):                        # (no handle goes without a frame)
            k, h = "render", owed[0]
        if (k == "read_rgba" and not rendered[h]) or (k == "recreate" and h == 0):
            continue
        x = state[h]
        op = dict(kind=k, h=h)
        if k == "render":
            op["s"] = int(rng.integers(0, ns))
            rendered[h] = True
        elif k == "uniforms_shading":
            x = changed(x, sun=SUNS[(SUNS.index(x["sun"]) + int(rng.integers(1, len(SUNS)))) % len(SUNS)])
        elif k == "uniforms_camera":
            x = changed(x, cam=(x["cam"] + int(rng.integers(1, len(CAMERAS)))) % len(CAMERAS))
        elif k == "height":                                   # (the layers stay: a contour layer keeps the lines of the heights it was added under)
            x = changed(x, h=heights(rng, x["h"].shape))
        elif k == "toggle_pass":
            p = op["p"] = str(rng.choice(PASSES))
            x = changed(x, on=tuple(q for q in PASSES if (q in x["on"]) != (q == p)))
        elif k == "toggle_layer":
            if x["layers"]:
                x = changed(x, layers=[])
            else:
                op["layer"] = line_layer(rng, occlude=bool(rng.random() < 0.6)) if rng.random() < 0.6 else contour_layer(x["h"], x["G"])
                x = with_layer(x, op["layer"])
        elif k in ("field_host", "field_device"):
            op["field"] = str(rng.choice(FIELDS))
            if k == "field_device":
                op["s"] = int(rng.integers(0, ns))
        elif k == "recreate":                                 # a new handle in its place, with the inputs as they stand; layers added under other heights go
            x = changed(x, layers=[l for l in x["layers"] if l[2] is x["h"]])
            rendered[h] = False
        state[h] = op["inputs"] = x
        ops.append(op)
    return dict(name=f"seed {seed}", seed=seed, handles=first, streams=ns, ops=ops)


def render_pairs(c):
    """the ordered stream pairs (a, b), a != b, of two renders with no operation between them during which the host may wait (only
    set_uniforms and pass settings, which queue nothing and wait for nothing) -> (pairs of one handle, pairs across two handles)"""
    same, across, last = set(), set(), None
    for op in c["ops"]:
        if op["kind"] == "render":
            if last is not None and last[1] != op["s"]:
                (same if last[0] == op["h"] else across).add((last[1], op["s"]))
            last = (op["h"], op["s"])
        elif op["kind"] in HOST_WAITS:
            last = None
    return same, across


def run_case(c, cabi=None, hip=None, stats=None):
    """One case on the GPU -> list of (name, op index, what, count of differing pixels or vertices, first positions).  The frames and
    the device reads go into slots made up front and are read when everything is queued; the host reads are compared as they come."""
    if cabi is None:
        from vulkan_forge_amd import cabi
    own_hip = hip is None
    hip = Hip() if own_hip else hip
    bad, memo, later = [], {}, []
    streams = [hip.stream() for _ in range(c["streams"])]
    # every slot up front: an allocation between two frames would wait for the device
    slot = {}
    for i, op in enumerate(c["ops"]):
        x = op["inputs"]
        if op["kind"] == "render":
            slot[i] = hip.slot(frame_bytes(x))
        elif op["kind"] == "field_device":
            slot[i] = hip.slot(max(x["G"], 2) ** 2 * 4)
    T = []
    try:
        for inp in c["handles"]:
            T.append(create(cabi, inp, share_ctx=T[0] if T else None))
        prev = None
        for i, op in enumerate(c["ops"]):
            k, t, x = op["kind"], T[op["h"]], op["inputs"]
            if k == "render":
                if stats is not None and prev is not None and prev != streams[op["s"]]:
                    stats["second_stream"] += 1
                    stats["not_ready"] += int(hip.busy(prev))
                t.set_output_device(slot[i])
                t.render(streams[op["s"]])
                prev = streams[op["s"]]
                later.append((i, "frame", x))
            elif k.startswith("uniforms"):
                t.set_uniforms(uniforms(x))
            elif k == "height":
                t.set_height(x["h"])
            elif k == "toggle_pass":
                set_pass(t, x, op["p"])
            elif k == "toggle_layer":
                if "layer" in op:
                    add_layer(t, op["layer"])
                else:
                    t.clear_overlays()
            elif k == "field_host":
                n, where = differing(READ[op["field"]][0](t), field(x, op["field"]))
                if n:
                    bad.append((c["name"], i, f"{op['field']} field read on the host", n, where))
            elif k == "field_device":
                READ[op["field"]][1](t, slot[i], streams[op["s"]])
                later.append((i, "field", x))
            elif k == "read_rgba":
                n, where = differing(t.read_rgba().reshape(x["H"], x["W"], 4), expected(x_of_last_frame(c, i), memo)["frame"])
                if n:
                    bad.append((c["name"], i, "read_rgba", n, where))
            elif k == "recreate":
                t.close()
                T[op["h"]] = create(cabi, x, share_ctx=T[0])
        for s in streams:
            hip.wait(s)
        for t in T:
            t.sync()
        for i, what, x in later:
            op = c["ops"][i]
            if what == "frame":
                n, where = differing(hip.read(slot[i], (x["H"], x["W"], 4)), expected(x, memo)["frame"])
            else:
                g = max(x["G"], 2)
                n, where = differing(hip.read(slot[i], (g, g), f32), field(x, op["field"]))
            if n:
                bad.append((c["name"], i, f"{what} of handle {op['h']} ({x['W']}x{x['H']} grid {x['G']}, on: {x['on']}) on stream {op['s']}"
                            + (f": {op['field']}" if what == "field" else ""), n, where))
    finally:
        for t in reversed(T):
            t.close()
        if own_hip:
            hip.close()
    return bad


def x_of_last_frame(c, i):
    """the inputs the last frame of op i's handle before op i was drawn from"""
    h = c["ops"][i]["h"]
    for op in reversed(c["ops"][:i]):
        if op["h"] == h and op["kind"] == "render":
            return op["inputs"]
        assert not (op["h"] == h and op["kind"] == "recreate")
    raise AssertionError("read_rgba before the first frame")


READ = dict(shadow=(lambda t: t.shadow_field(), lambda t, d, s: t.shadow_field_device(d, s)),
            sky=(lambda t: t.sky_view_field(), lambda t, d, s: t.sky_view_field_device(d, s)),
            flood=(lambda t: t.flood_field(), lambda t, d, s: t.flood_field_device(d, s)),
            spill=(lambda t: t.spill_field(), lambda t, d, s: t.spill_field_device(d, s)),
            exposure=(lambda t: t.sun_exposure_field(), lambda t, d, s: t.sun_exposure_field_device(d, s)),
            cumulative=(lambda t: t.cumulative_viewshed_field(), lambda t, d, s: t.cumulative_viewshed_field_device(d, s)),
            viewshed=(lambda t: t.viewshed_field(), lambda t, d, s: t.viewshed_field_device(d, s)))

FRESH_SEED = 70000                                            # the script's default window: apart from the suite's (test_gpu_handle_soak.py)


def run(first=FRESH_SEED, cases=100, budget=400.0, verbose=True):
    """seeds first .. first + cases - 1, until `budget` seconds have passed -> dict cases, bad, stats, summary"""
    from vulkan_forge_amd import cabi
    cabi.load()
    t0 = time.time()
    bad, done = [], 0
    stats = dict(second_stream=0, not_ready=0)
    for seed in range(first, first + cases):
        if time.time() - t0 > budget:
            break
        c = case(seed)
        b = run_case(c, cabi, stats=stats)
        for m in b:
            if verbose:
                print(f"MISMATCH {m[0]} op {m[1]}: {m[2]}: {m[3]} differ, first at {m[4]}", flush=True)
        bad.extend(b)
        done += 1
    summary = (f"handle soak: {done} cases from seed {first}: {len(bad)} mismatches; {stats['second_stream']} renders went onto another stream than the render "
               f"before them, {stats['not_ready']} of them while that stream was not ready; {time.time() - t0:.1f} s")
    if verbose:
        print(summary, flush=True)
    return dict(cases=done, bad=bad, stats=stats, summary=summary, seconds=time.time() - t0)


if __name__ == "__main__":
    first = int(sys.argv[1]) if len(sys.argv) > 1 else FRESH_SEED
    cases = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    budget = float(sys.argv[3]) if len(sys.argv) > 3 else 400.0
    sys.exit(1 if run(first, cases, budget)["bad"] else 0)

"""What the CPU models (tests/*_model) share: where they are, what each is built from, how its library is built and loaded, how its C
functions are declared and called, and the opening lines of their frame functions.  Imports nothing native and no pytest.

Importing this module puts every tests/*_model directory and the repository root on sys.path (once): a model, a test or a tool
imports it (or tests/support.py, which does) first and then the models by name.

    import model_support as ms
    lib = ms.load("shadow_model", {"shm_heights": "i32(f32*, f32*, f32*, u32, u32, u32)", ...})
    lib.shm_heights(h, u, tex, tw, th, grid)        # numpy arrays as they are: checked, never converted

A signature is `<return>(<parameter>, ...)`:
    i8 u8 i16 u16 i32 u32 i64 u64 f32 f64     a scalar of that C type (`int` is i32); as a return type also `void`
    T*                                        a pointer to elements of scalar type T: the call takes a C-contiguous ndarray of exactly
                                              that dtype and passes its address
    T*?                                       the same, or None (a null pointer)
    recN*                                     a pointer to records of N bytes each (the overlay models' OVIN records are rec48): a
                                              C-contiguous ndarray whose items are N bytes, whatever their fields
Anything else handed to a pointer parameter -- another dtype, a strided view, a list, an address, None where no `?` stands -- raises
TypeError naming the function and the parameter's index, before the C function runs.  Nothing is converted or copied here: the models
write their results through these pointers, so a copy would lose them, and a float64 array read as float32 is a wrong oracle.
"""
import ctypes as C
import glob
import os
import re
import subprocess
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

for _p in (*sorted(glob.glob(os.path.join(HERE, "*_model" + os.sep))), ROOT):     # (once: a second import finds them there)
    _p = _p.rstrip(os.sep)
    if _p not in sys.path:
        sys.path.insert(0, _p)


# ---- what a model is built from, and its library ----

INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"(\.\./\w+/\w+\.c)"', re.M)


def source(name):
    """the C file of model `name` (tests/<name>/<name>.c); a path to a C file stands for itself (the made-up models of the tests)"""
    return name if name.endswith(".c") else os.path.join(HERE, name, name + ".c")


def sources(name):
    """[the model's C file, then every model source it includes, directly or through another, in the order the compiler reads them]"""
    out = [os.path.normpath(source(name))]
    for f in out:                                              # (grows while it is read)
        with open(f) as fh:
            for inc in INCLUDE.findall(fh.read()):
                p = os.path.normpath(os.path.join(os.path.dirname(f), inc))
                if p not in out:
                    out.append(p)
    return out


SCALARS = {"i8": C.c_int8, "u8": C.c_uint8, "i16": C.c_int16, "u16": C.c_uint16, "i32": C.c_int32, "u32": C.c_uint32, "i64": C.c_int64,
           "u64": C.c_uint64, "f32": C.c_float, "f64": C.c_double}
DTYPES = {"i8": np.int8, "u8": np.uint8, "i16": np.int16, "u16": np.uint16, "i32": np.int32, "u32": np.uint32, "i64": np.int64,
          "u64": np.uint64, "f32": np.float32, "f64": np.float64}
SIGNATURE = re.compile(r"\s*(\w+)\s*\((.*)\)\s*")


class Pointer:
    """a pointer parameter: the element dtype (or the record size) and whether None may stand for it"""

    def __init__(self, spec):
        self.spec = spec
        self.nullable = spec.endswith("?")
        elem = spec.rstrip("?")[:-1]
        self.itemsize = int(elem[3:]) if elem.startswith("rec") else None
        self.dtype = None if elem.startswith("rec") else np.dtype(DTYPES[elem])

    def address(self, a, where):
        if a is None and self.nullable:
            return None
        if not isinstance(a, np.ndarray) or not a.flags.c_contiguous or (a.dtype != self.dtype if self.dtype else a.dtype.itemsize != self.itemsize):
            got = f"{a.dtype} ndarray, C-contiguous: {a.flags.c_contiguous}" if isinstance(a, np.ndarray) else type(a).__name__
            raise TypeError(f"{where}: wants {self.spec} (a C-contiguous ndarray of exactly that element type), got {got}")
        return a.ctypes.data


def parse(signature):
    """'i32(f32*, u8*?, u32)' -> (the ctypes return type or None, [a ctypes scalar type or a Pointer per parameter])"""
    m = SIGNATURE.fullmatch(signature)
    assert m, signature
    params = [p.strip() for p in m.group(2).split(",")] if m.group(2).strip() else []
    return None if m.group(1) == "void" else SCALARS[m.group(1)], [Pointer(p) if "*" in p else SCALARS[p] for p in params]


def declare(library, name, signature):
    """the function `name` of a loaded library under `signature`; AttributeError if the library does not export it"""
    restype, params = parse(signature)
    fn = C.CFUNCTYPE(restype, *[C.c_void_p if isinstance(p, Pointer) else p for p in params])((name, library))
    pointers = [(k, p) for k, p in enumerate(params) if isinstance(p, Pointer)]

    def call(*args):
        if len(args) != len(params):
            raise TypeError(f"{name}: takes {len(params)} arguments, got {len(args)}")
        raw = list(args)                                       # (`args` keeps the arrays alive over the call)
        for k, p in pointers:
            raw[k] = p.address(args[k], f"{name} parameter {k}")
        return fn(*raw)

    call.__name__ = name
    return call


_loaded = {}


def load(name, signatures, build_dir=None):
    """-> the functions of `signatures` (name: signature) of model `name`, as attributes.  The library is build/lib<name>.so, compiled
    again when it is missing or older than any file of sources(name); one per process.  `build_dir`: another directory than build/, for
    the test that a stale library is rebuilt."""
    src = source(name)
    out = os.path.join(build_dir or os.path.join(ROOT, "build"), "lib" + os.path.splitext(os.path.basename(src))[0] + ".so")
    if out not in _loaded:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in sources(name)):
            tmp = out + f".{os.getpid()}.tmp"
            subprocess.check_call(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", tmp, "-lm"])
            os.replace(tmp, out)
        library = C.CDLL(out)
        _loaded[out] = types.SimpleNamespace(**{f: declare(library, f, s) for f, s in signatures.items()})
    return _loaded[out]


# ---- the opening lines of the models' functions ----

def pack(rgba):
    """(r, g, b, a) bytes -> the colour word the records and the tints carry"""
    r, g, b, a = (int(v) for v in rgba)
    return r | g << 8 | b << 16 | a << 24


def u44(uniforms):
    """the scene's 44 uniforms as contiguous float32"""
    return np.ascontiguousarray(uniforms, np.float32).reshape(44)


def lut(lut_rgba8):
    """the handle's 256 sRGB texels as the 1024 contiguous bytes the shade passes read"""
    return np.ascontiguousarray(lut_rgba8, np.uint8).reshape(1024)


def field(a):
    """a vertex field as contiguous float32; None stays None (the feature is off)"""
    return None if a is None else np.ascontiguousarray(a, np.float32)


def texture(height):
    """-> (the height texture as contiguous float32, its width, its height): the three arguments the C functions take for it"""
    tex = np.ascontiguousarray(height, np.float32)
    return tex, tex.shape[1], tex.shape[0]


def frame(rgba, vis, uniforms, height):
    """What a function over a frame starts from -> (a writable copy of the frame as (H, W, 4) uint8 (None without `rgba`), vis as
    contiguous (H, W) uint32, then W, H, u44, the texture, its width, its height: the scene, in the order the C functions take it)

        out, vis, *scene = ms.frame(rgba, vis, uniforms, height)
        lib().xxm_frame(out, plane, vis, *scene, grid, ...)"""
    vis = np.ascontiguousarray(vis, np.uint32)
    H, W = vis.shape
    out = None if rgba is None else np.ascontiguousarray(rgba, np.uint8).reshape(H, W, 4).copy()
    return (out, vis, W, H, u44(uniforms), *texture(height))

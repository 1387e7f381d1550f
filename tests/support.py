"""What the GPU and model tests share: paths, bit comparisons, the scene uniforms, a C-ABI handle on a height field, the oracle's
frame (one cache for the whole process), the `vf` / `cabi` fixtures and the run of a check script in a child process.

Importing this module imports nothing native (no oracle, vulkan_forge, vulkan_forge_amd or torch): test modules are collected before
the session fixture has built those, so everything that needs them is imported inside the functions."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from model_support import HERE, ROOT            # (importing it puts the repository root and the model directories on sys.path)


@pytest.fixture(scope="module")
def vf():
    import vulkan_forge
    return vulkan_forge


@pytest.fixture(scope="module")
def cabi():
    from vulkan_forge_amd import cabi as m
    m.load()
    return m


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def digest(h):
    """a cache key for a whole array: its shape and a hash of all of its bytes"""
    h = np.ascontiguousarray(h)
    return h.shape, hashlib.sha1(h.tobytes()).hexdigest()


def frozen(x):
    """x with every array in it (itself, its items, its attributes) read-only: what a cache hands out stays what it computed"""
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, (tuple, list)):
        for v in x:
            frozen(v)
    elif isinstance(x, dict) or hasattr(x, "__dict__"):
        for v in (x if isinstance(x, dict) else vars(x)).values():
            frozen(v)
    return x


def assert_field(got, want, what):
    """two float32 vertex fields of one shape, equal bit for bit (so -0 is not +0, and a NaN equals only its own payload)"""
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32, (what, got.shape, got.dtype, want.shape, want.dtype)
    d = bits(got) != bits(want)
    assert not d.any(), f"{what}: {int(d.sum())} vertices differ, first at {np.argwhere(d)[:4].tolist()}: {got[d][:4]} against {want[d][:4]}"


def assert_frame(got, want, what):
    """two (H, W, 4) frames, equal byte for byte"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = (got != want).any(axis=2)
    assert not d.any(), f"{what}: {int(d.sum())} pixels differ, first at {np.argwhere(d)[:4].tolist()}: {got[d][:2].tolist()} against {want[d][:2].tolist()}"


def uniforms(W, H, cam="default", *, exag=None, spacing=None, sun=None, cameras=None):
    """the scene's float32 uniform block of 44 for one of overlay_scenes' cameras (or of `cameras`)"""
    import oracle
    if cameras is None:
        from overlay_scenes import CAMERAS as cameras
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *cameras[cam]), np.float32).reshape(44)
    if exag is not None:
        u[38] = exag
    if spacing is not None:
        u[36] = spacing
    if sun is not None:
        u[32:35] = sun
    return u


def terrain(W, H, grid, h, lut=None):
    from vulkan_forge_amd import cabi as m
    t = m.Terrain(W, H, grid, np.zeros(1024, np.uint8) if lut is None else lut)
    t.set_height(h)
    return t


def viridis():
    """the 256 sRGB texels of the scenes' default colormap (an extension of vulkan_forge_amd, not of the drop-in module)"""
    import vulkan_forge_amd
    return vulkan_forge_amd.colormap_rgba8("viridis")


_oracle = {}


def oracle_key(u, W, H, grid, h, mode="reference"):
    return (np.asarray(u, np.float32).tobytes(), W, H, grid, digest(h), mode)


def oracle_frame(u, W, H, grid, h, mode="reference"):
    """the oracle's (H, W, 4) frame and its visibility plane under viridis: computed once per case and process, handed out read-only"""
    import oracle
    key = oracle_key(u, W, H, grid, h, mode)
    if key not in _oracle:
        rgba, vis = oracle.render_terrain(u, W, H, grid, h, viridis(), want_vis=True, nthreads=8,
                                          shade_mode=oracle.SHADE_SPEC_T32 if mode == "spec_t32" else oracle.SHADE_REFERENCE)
        _oracle[key] = frozen((rgba.reshape(H, W, 4), vis))
    return _oracle[key]


def run_check(script, marker, timeout=300, args=(), env=None):
    """run a check script of this directory in a child process: it must exit 0 and print its marker"""
    r = subprocess.run([sys.executable, os.path.join(HERE, script), *args], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0 and marker in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r


def smooth(n, seed=1):
    """a smooth n x n float32 height field: four seeded sine waves"""
    rng = np.random.default_rng(seed)
    x = np.linspace(0, 1, n, dtype=np.float64)
    X, Z = np.meshgrid(x, x)
    h = sum(rng.normal() * 0.2 / f * np.sin(2 * np.pi * f * (X * np.cos(a) + Z * np.sin(a)) + p)
            for f, a, p in zip((1, 2, 3, 5), rng.uniform(0, 6.3, 4), rng.uniform(0, 6.3, 4)))
    return h.astype(np.float32)


def ridge(shape=(64, 64)):
    """a wall 1.5 high across the terrain at z = 0 (texture rows map to z)"""
    z = np.linspace(-1.5, 1.5, shape[0])
    return np.broadcast_to((1.5 * np.exp(-(z / 0.25) ** 2))[:, None], shape).astype(np.float32)

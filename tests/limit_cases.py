"""Case descriptions at the size limits the C ABI accepts (include/vf_hip.h): frames of 16384 pixels, 256 tile columns and stripes,
height textures of 32768 texels, ambient reach 1024 and 64 directions, 65536 contour levels.  Shared by tests/test_gpu_limits.py (the
GPU against the oracle and the models) and tests/test_limit_cases.py (the oracle and the models alone show that every case reaches the
edge it is named for).  Pure numpy: a case holds the frame, grid, camera, texture shape and seed; nothing here needs a GPU."""
import math

import numpy as np

f32 = np.float32
MAX_FRAME, MAX_TEXTURE, MAX_STRIPES, MAX_LEVELS, MAX_REACH, MAX_DIRECTIONS = 16384, 32768, 256, 65536, 1024, 64
TILE, BIN = 64, 16
HALF = 1.5                                                    # the terrain spans +-1.5 spacing in x and z


def noise(seed, shape, amp=0.5):
    """white noise heights in +-amp / 2, float32, as conftest.heightmap draws them"""
    return (np.random.default_rng(seed).random(shape, dtype=f32) - f32(0.5)) * f32(amp)


def top_down(W, H, height=6.0, fill=0.5):
    """A camera above the centre looking down, up = -z: x runs along the frame's width and z down its height.  The reference's
    projection puts 1.5 depth - znear into w, so a frame whose plain half extent is `fill` * 1.5 at height 0 shows the terrain's edge at
    about 0.8 / fill of the frame's LONGER half side: the terrain overfills that side also where its surface is lowest (-0.75), and the
    other side of an extreme aspect sees a strip a few cells wide."""
    aspect = W / H
    t = fill * HALF / height / max(aspect, 1.0)               # tan(fovy / 2)
    return ((0.0, height, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 2.0 * math.degrees(math.atan(t)), 0.1, 100.0)


def grazing(W, H, fill=0.9, znear=1.3):
    """A low camera on the -x side looking across the terrain at its centre; z runs along the frame's long side (up = +y for a wide
    frame, -z for a tall one).  The near plane stands in the terrain (the reference's projection puts it at a depth of about 2 znear):
    the hills nearest to the camera, highest around z = 0, are cut through, and the ends of the long side are not."""
    aspect = W / H
    eye = (-2.6, 0.45, 0.0)
    t = fill * HALF / math.hypot(*eye) / max(aspect, 1.0)
    return (eye, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0) if aspect >= 1.0 else (0.0, 0.0, -1.0), 2.0 * math.degrees(math.atan(t)), znear, 100.0)


def uncut(camera):
    """the same camera with the near plane in front of the terrain"""
    return camera[:4] + (0.1, camera[5])


def _case(name, W, H, grid, tex, seed, camera, frames=1, cmap="viridis", amp=0.5):
    return dict(name=name, W=W, H=H, grid=grid, tex=tex, seed=seed, camera=camera, frames=frames, cmap=cmap, amp=amp)


def _aspects():
    out = []
    #        W      H      grid  texture (rows, columns)
    for W, H, G, tex in ((16384, 1, 129, (31, 129)), (16384, 24, 1025, (64, 1025)), (16383, 130, 1025, (77, 300)), (1, 16384, 257, (257, 19)),
                         (24, 16384, 1025, (1025, 64)), (130, 16383, 1025, (300, 77)), (4097, 257, 300, (150, 301))):
        for kind, cam in (("down", top_down(W, H)), ("grazing", grazing(W, H))):
            # three frames on one handle (the last one planned from feedback) on one wide and one tall case
            frames = 3 if (W, H, kind) in ((16384, 24, "down"), (24, 16384, "down")) else 1
            out.append(_case(f"{W}x{H}_{kind}", W, H, G, tex, 7000 + len(out), cam, frames))
    return out


ASPECT_CASES = _aspects()

# the whole 16384 x 16384 frame: bands of 64 rows dealt to 128 ranks, of which the first, one in the middle and the last are compared
FULL = _case("16384x16384_down", MAX_FRAME, MAX_FRAME, 2049, (512, 512), 7100, top_down(MAX_FRAME, MAX_FRAME), frames=2)
FULL_RANKS, FULL_NRANKS, FULL_BAND = (0, 77, 127), 128, 64

# shards at the limit: 256 tile columns dealt to 8 ranks, and 256 tile rows in bands
SHARD_WIDE = _case("16384x128_shards", MAX_FRAME, 128, 513, (40, 513), 7200, top_down(MAX_FRAME, 128))
SHARD_TALL = _case("128x16384_bands", 128, MAX_FRAME, 513, (513, 40), 7201, top_down(128, MAX_FRAME))
SHARD_RANKS = 8


def stripe_owners(nstripes=MAX_STRIPES, nranks=SHARD_RANKS, seed=7210):
    """an uneven owner table: rank r owns about (r + 1) shares of the stripes, shuffled, so every rank owns non-adjacent stripes"""
    rng = np.random.default_rng(seed)
    w = np.arange(1, nranks + 1, dtype=np.float64)
    owner = rng.choice(nranks, size=nstripes, p=w / w.sum()).astype(np.uint8)
    owner[:nranks] = np.arange(nranks)                        # (no rank without a stripe)
    return owner


def rows_of(rank, nranks, band, H):
    return np.flatnonzero(((np.arange(H) // band) % nranks) == rank)


def uniforms(c, oracle):
    return oracle.look_at_uniforms(1, c["W"], c["H"], *c["camera"])


def heights(c):
    return noise(c["seed"], c["tex"], c["amp"])


# height textures at 32768 texels a side: (rows, columns); a NaN texel in the last column
TEXTURE_SHAPES = ((1, MAX_TEXTURE), (MAX_TEXTURE, 1), (3, MAX_TEXTURE))
TEXTURE_FRAME = (200, 150, 257)


def big_texture(shape, seed=7300):
    h = noise(seed + shape[0], shape, amp=1.0)
    h[shape[0] // 2, shape[1] - 1] = np.nan
    return h


# contours at 65536 levels: a small grid, so that millions of segments fall into one block of the extraction; at grid 33 round joins
# need more records than the 2^24 a handle may hold
DEFAULT_CAMERA = ((3.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0)
CONTOURS = _case("contours_65536_levels", 96, 64, 9, (5, 7), 7500, DEFAULT_CAMERA, amp=1.0)
CONTOURS_REFUSED_GRID = 33
RECORD_BUDGET = 1 << 24


def contour_levels(bounds, n=MAX_LEVELS):
    """n distinct ascending float32 levels over the height bounds (lo, hi) of the surface"""
    return np.linspace(bounds[0], bounds[1], n).astype(f32)

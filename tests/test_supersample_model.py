"""The CPU model of supersampled frames (tests/supersample_model): the resolve's contract on hand-built blocks -- the
identity at f = 1, uniform blocks of every byte, the mean in linear light, alpha half up, the summation order -- and, on an oracle
frame with a ridge against the background, that the resolved frame has intermediate pixels along the silhouette where the 1x frame
has none."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
import support  # noqa: F401  (the repository root and the model directories on sys.path)
import supersample_model as ssm

F32 = np.float32


def block(f, values, alpha=255):
    """one output pixel's f x f samples, row-major `values` in all three colour channels"""
    s = np.empty((f, f, 4), np.uint8)
    s[..., :3] = np.asarray(values, np.uint8).reshape(f, f, 1)
    s[..., 3] = np.asarray(alpha, np.uint8).reshape(-1, 1).reshape(f, f) if np.ndim(alpha) else alpha
    return s


def test_the_tables_are_the_ones_the_tint_models_use():
    import oracle
    import overlay_model as om
    dec, thr = ssm.tables()
    assert [F32(om.decode(k)) for k in range(256)] == list(dec)
    # the encode at every threshold, one step below it, and at 1500 seeded values
    probe = np.concatenate([thr[1:], np.nextafter(thr[1:], F32(-1)), np.random.default_rng(4).random(1500, dtype=F32), [F32(0), F32(1)]]).astype(F32)
    got = ssm.encode(probe)
    assert np.array_equal(got, oracle.srgb_encode(probe))
    assert [int(v) for v in got] == [om.encode(c) for c in probe]


def test_factor_one_is_the_identity():
    x = np.random.default_rng(0).integers(0, 256, (5, 7, 4), dtype=np.uint8)
    assert np.array_equal(ssm.resolve(x, 1), x)


@pytest.mark.parametrize("f", [2, 3, 4])
def test_a_uniform_block_of_every_byte_resolves_to_that_byte(f):
    # 256 output pixels in a column, pixel v made of f x f samples (v, v, v, v)
    s = np.repeat(np.repeat(np.arange(256, dtype=np.uint8).reshape(256, 1, 1), f, axis=0), f, axis=1)
    s = np.repeat(s, 4, axis=2)
    out = ssm.resolve(s, f)
    assert out.shape == (256, 1, 4)
    bad = [(v, out[v, 0].tolist()) for v in range(256) if (out[v, 0] != v).any()]
    assert not bad, bad


def test_the_mean_is_taken_in_linear_light():
    import oracle
    dec, _ = ssm.tables()
    assert ssm.resolve(block(2, [0, 255, 255, 0]), 2)[0, 0].tolist() == [188, 188, 188, 255]
    assert ssm.resolve(block(2, [0, 0, 255, 255]), 2)[0, 0, 0] == 188
    for f, white in ((3, 4), (3, 5), (4, 8), (4, 3)):
        v = [255] * white + [0] * (f * f - white)
        exact = np.float64(white) * np.float64(dec[255]) / (f * f)          # dec[0] = 0, dec[255] = 1: the exact linear mean
        want = int(oracle.srgb_encode(np.array([exact], F32))[0])
        got = ssm.resolve(block(f, v), f)[0, 0]
        assert got[0] == want and want not in (0, 255) and got[3] == 255
        assert want > round(255 * white / (f * f))                          # (not the mean of the bytes: linear light is brighter)


def test_alpha_is_the_integer_mean_rounded_half_up():
    a2 = lambda al: int(ssm.resolve(block(2, [9] * 4, alpha=np.array(al)), 2)[0, 0, 3])      # noqa: E731
    assert a2([0, 0, 1, 1]) == 1          # 2 / 4 = 0.5 -> 1
    assert a2([0, 0, 0, 1]) == 0          # 0.25 -> 0
    assert a2([255, 255, 255, 254]) == 255 and a2([255, 254, 254, 254]) == 254 and a2([255, 255, 254, 254]) == 255
    a3 = lambda al: int(ssm.resolve(block(3, [9] * 9, alpha=np.array(al)), 3)[0, 0, 3])      # noqa: E731
    assert a3([1, 1, 1, 1, 0, 0, 0, 0, 0]) == 0 and a3([1, 1, 1, 1, 1, 0, 0, 0, 0]) == 1     # 4 / 9 -> 0, 5 / 9 -> 1
    a4 = lambda al: int(ssm.resolve(block(4, [9] * 16, alpha=np.array(al)), 4)[0, 0, 3])     # noqa: E731
    assert a4([1] * 8 + [0] * 8) == 1 and a4([1] * 7 + [0] * 9) == 0


def test_the_summation_order_is_rows_outer_columns_inner_from_the_first_sample():
    """The 2 x 2 block (205, 143 / 93, 118): ((205 + 143) + 93) + 118 in binary32 lands below the threshold of 148, the column-major
    and the reversed sums on it."""
    s = block(2, [205, 143, 93, 118])
    assert ssm.resolve(s, 2)[0, 0, 0] == 147
    assert ssm.resolve(s, 2, order=[(0, 0), (1, 0), (0, 1), (1, 1)])[0, 0, 0] == 148
    assert ssm.resolve(s, 2, order=[(1, 1), (1, 0), (0, 1), (0, 0)])[0, 0, 0] == 148
    # ... and starting from 0 is no different from starting from the first sample (0 + x is x): the contract's wording fixes the count of additions
    dec, _ = ssm.tables()
    l = dec[[205, 143, 93, 118]]
    assert ssm.encode(np.array([F32(F32(F32(l[0] + l[1]) + l[2]) + l[3]) * F32(0.25)], F32))[0] == 147


def test_representative():
    p = np.arange(12 * 8).reshape(12, 8)
    assert np.array_equal(ssm.representative(p, 1), p)
    assert ssm.representative(p, 2)[1, 2] == p[3, 5] and ssm.representative(p, 4)[2, 1] == p[10, 6] and ssm.representative(p, 3).shape == (4, 3)
    assert ssm.representative(np.arange(36).reshape(6, 6), 3)[1, 1] == 4 * 6 + 4


# ---- a ridge against the background ----

W, H, GRID = 64, 48, 32
RIDGE_CAMERA = ((0.0, 0.45, 3.4), (0.0, 0.25, 0.0), (0.0, 1.0, 0.0), 40.0, 0.1, 100.0)      # grazing: the ridge stands against the background


def ridge_heights():
    x = np.linspace(-1.0, 1.0, 33, dtype=F32)
    z = np.linspace(-1.0, 1.0, 33, dtype=F32)
    return (0.9 * np.exp(-(z[:, None] / 0.25) ** 2) * (0.6 + 0.4 * np.cos(3.0 * x[None, :]))).astype(F32)


@pytest.fixture(scope="module")
def ridge():
    import oracle
    lut = np.load(os.path.join(HERE, "golden", "colormaps_rgba8.npz"))["viridis"]
    u = oracle.look_at_uniforms(1, W, H, *RIDGE_CAMERA)
    h = ridge_heights()
    plain, vis1 = oracle.render_terrain(u, W, H, GRID, h, lut, want_vis=True)
    return dict(u=u, h=h, lut=lut, plain=plain.reshape(H, W, 4), vis1=vis1)


@pytest.mark.parametrize("f", [2, 4])
def test_a_silhouette_gets_intermediate_pixels_the_1x_frame_lacks(ridge, f):
    r = ssm.frame(W, H, f, ridge["u"], ridge["h"], GRID, ridge["lut"])
    s, vis, out = r["samples"], r["vis"], r["frame"]
    assert s.shape == (f * H, f * W, 4) and vis.shape == (f * H, f * W) and out.shape == (H, W, 4)
    assert np.array_equal(out, ssm.resolve(s, f))                 # (no overlays)
    covered = (vis != 0).reshape(H, f, W, f)
    n = covered.sum(axis=(1, 3))
    mixed = (n > 0) & (n < f * f)                                 # the silhouette: pixels with samples of both sides
    assert mixed.sum() >= 20 and (n == 0).any() and (n == f * f).any()
    bg = s[vis == 0]
    assert (bg == bg[0]).all()                                    # one background colour
    B = bg[0, :3].astype(int)
    # a channel in which every terrain sample, of the samples and of the 1x frame, lies clearly on one side of the background
    terr = np.concatenate([s[vis != 0][:, :3], ridge["plain"][ridge["vis1"] != 0][:, :3]]).astype(int)
    gap = np.maximum(terr.min(axis=0) - B, B - terr.max(axis=0))
    ch = int(np.argmax(gap))
    assert gap[ch] >= 8, gap
    lo, hi = sorted((int(B[ch]), int(terr.min(axis=0)[ch] if terr.min(axis=0)[ch] > B[ch] else terr.max(axis=0)[ch])))
    between = lambda img: (img[..., ch].astype(int) > lo) & (img[..., ch].astype(int) < hi)      # noqa: E731
    assert not between(ridge["plain"]).any()                      # 1x: every pixel is one side's colour
    got = between(out)
    assert got.sum() >= 10 and not (got & ~mixed).any()           # resolved: strictly between, and only along the silhouette
    # a pixel whose samples all lie on one side keeps that side: the background stays the background
    assert (out[n == 0] == np.append(B, bg[0, 3])).all()

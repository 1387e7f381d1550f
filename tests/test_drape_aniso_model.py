"""The CPU model of anisotropic filtering of the drape's mip sampling (tests/drape_aniso_model) against what anisotropic
filtering must do: the largest anisotropy 1 is the mip model bit for bit, the plan equals a numpy restatement on hand-worked
footprints, a constant image gives the isotropic frame, the level of detail never rises, the tap count is the footprint's ratio on the
surface, the frame comes closer to a supersampled reference, and the cases the GPU tests draw reach every branch."""

import numpy as np
import pytest

import support  # noqa: F401  (first: the repository root and the model directories on sys.path)
import drape_aniso_model as dam
from support import uniforms
from test_drape_model import VIRIDIS, constant_lut, plain
from overlay_scenes import GRID, heights

dmm = dam.dmm
drm = dmm.drm
import gbuffer_model as gbm

f32 = np.float32
AS = (2, 4, 8, 16)


@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_anisotropy_1_is_the_mip_model(cam):
    W, H = 257, 131
    u, rgba, vis = plain(W, H, cam)
    img = dmm.case_image()
    for filt in ("linear", "nearest"):
        for bias in (-1.0, 0.0, 1.5):
            kw = dict(extent=dam.CASE_EXTENT[cam], filter=filt, bias=bias, opacity=0.37)
            want, want_again, ws = dmm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, want_sample=True, **kw)
            got, again, s = dam.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, max_anisotropy=1, want_sample=True, **kw)
            assert want_again.any() and np.array_equal(again, want_again) and np.array_equal(got, want), (filt, bias)
            assert np.array_equal(s[..., :7].view(np.uint32), ws.view(np.uint32)) and (s[..., 7][again] == 1).all()


# ---- the plan (items 1 - 4) and the tap offsets (item 5) restated in numpy binary32 ----

def np_lod(rho2, bias):
    bits = int(np.array(rho2, f32).view(np.uint32))
    E, M = (bits >> 23) & 255, bits & 0x7FFFFF
    if bits >> 31 or E == 0 or (E == 255 and M):
        return f32(-np.inf)
    if E == 255:
        return f32(np.inf)
    return f32(f32(0.5) * f32(f32(E - 127) + f32(f32(M) * f32(2.0 ** -23))) + f32(bias))


def np_plan(ax, ay, A, bias=0.0):
    ax, ay = f32(ax), f32(ay)
    ym = bool(ay > ax)
    amax, amin = (ay, ax) if ym else (ax, ay)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if not amax > f32(f32(1.5625) * amin):
            return ym, np_lod(amax, bias), 1
        t = f32(amax * f32(1.0 / (A * A)))
        m2 = amin if amin > t else t
        n = next((k for k in range(1, A + 1) if amax <= f32(f32(k * k) * m2)), A)
    return ym, np_lod(m2, bias), n


def same_plan(a, b):
    return a[0] == b[0] and np.array(a[1], f32).view(np.uint32) == np.array(b[1], f32).view(np.uint32) and a[2] == b[2]


def test_the_plan_on_hand_worked_footprints():
    """the squared lengths (amin, amax) = (4, 4 r^2): 0.5 log2(4) = 1, so lod = 1 while the ratio r fits in A taps and
    1 + log2(r / A) beyond (exact where r / A is a power of two)"""
    amin = f32(4.0)
    for A in (1,) + AS:
        for r, n_want in ((1.0, 1), (1.25, 1), (2.0, 2), (2.5, 3), (16.0, 16), (17.0, 17), (1000.0, 1000)):
            amax = f32(amin * f32(r * r))                      # (exact: r^2 has few bits)
            for ym, (ax, ay) in ((False, (amax, amin)), (True, (amin, amax))):
                got = dam.plan(ax, ay, A)
                assert same_plan(got, np_plan(ax, ay, A)), (A, r, ym)
                if r <= 1.25 or A == 1:                       # item 2 (or A = 1): 4k's pixel, lod from the longer axis
                    assert got[2] == 1 and got[1] == np_lod(amax, 0.0), (A, r)
                    assert got[0] == (ym and r > 1.0)
                else:
                    assert got[0] == ym and got[2] == min(A, n_want), (A, r, got)
                    if r <= A:
                        assert got[1] == f32(1.0), (A, r, got)
                    elif r == 16.0:
                        assert got[1] == f32(1.0 + np.log2(16.0 / A)), (A, r, got)
                    else:
                        assert got[1] > f32(1.0) and got[1] <= np_lod(amax, 0.0), (A, r, got)
        # just above 1.25: the first ratio that takes more than one tap
        above = np.nextafter(f32(1.5625) * amin, f32(np.inf))
        got = dam.plan(above, amin, A, bias=0.5)
        assert same_plan(got, np_plan(above, amin, A, bias=0.5)) and got[2] == (2 if A > 1 else 1)
        assert got[1] == (f32(1.5) if A > 1 else np_lod(above, 0.5))
        # zero, denormal, infinite and NaN components
        den, inf, nan = f32(1e-42), f32(np.inf), f32(np.nan)
        for ax, ay in ((0.0, 0.0), (0.0, 4.0), (4.0, 0.0), (den, den), (den, 0.0), (den, 4.0), (f32(3e-45), f32(1e-44)), (inf, 4.0), (4.0, inf),
                       (inf, inf), (nan, 4.0), (4.0, nan), (nan, nan), (inf, nan), (inf, 0.0), (f32(3e38), f32(1e-38))):
            got = dam.plan(ax, ay, A, bias=0.25)
            assert same_plan(got, np_plan(ax, ay, A, bias=0.25)), (A, ax, ay, got)
            assert 1 <= got[2] <= A
        assert dam.plan(0.0, 0.0, A) == (False, f32(-np.inf), 1)                  # 4k's routes: level 0 ...
        assert dam.plan(nan, 4.0, A)[1:] == (f32(-np.inf), 1) and dam.plan(4.0, nan, A)[1:] == (f32(1.0), 1)    # ... a NaN axis as 4k takes it
        assert dam.plan(inf, inf, A)[1:] == (f32(np.inf), 1)                    # ... the top level
        assert dam.plan(inf, 4.0, A)[1:] == (f32(np.inf), 1)                    # an infinite longer axis: one tap at the top level
        assert dam.plan(4.0, 0.0, A)[2] == A and dam.plan(4.0, 0.0, A)[1] == f32(1.0 - np.log2(A))     # a zero shorter axis: A taps


def test_the_tap_offsets():
    for n in range(1, 17):
        w = f32(1.0) / f32(n)
        o = np.array([dam.offset(n, i) for i in range(n)], f32)
        want = np.array([f32(f32(f32(i) + f32(0.5)) * w) - f32(0.5) for i in range(n)], f32)
        assert np.array_equal(o.view(np.uint32), want.view(np.uint32)), n
        assert (np.diff(o) > 0).all() and o[0] >= -0.5 and o[-1] <= 0.5
        assert f32(f32(n) * w) == 1.0                          # the mean of N equal values is the value (N <= 16)
        if n & 1:
            assert o[n // 2] == 0.0, n                        # the middle tap of an odd N is the pixel's own sample point
    for n in (2, 3, 16):
        o = np.array([dam.offset(n, i) for i in range(n)], f32)
        print(f"N = {n}: offsets {o.tolist()}")
        if n != 3:
            assert np.array_equal(o, -o[::-1]), n             # 1 / N is exact: symmetric to the bit
        # fl(1 / 3) is not a third: each offset carries two roundings of values below 1 (the product, at most 2^-25, and the difference,
        # at most 2^-26) and the error of w itself scaled by (i + 0.5) <= 2.5 (2.5 * 2^-26): a pair's sum is within 2^-22 of zero
        assert np.abs(o + o[::-1]).max() <= 2.0 ** -22, n
    assert [float(dam.offset(2, i)) for i in range(2)] == [-0.25, 0.25]
    assert [float(dam.offset(16, i)) for i in range(16)] == [(i + 0.5) / 16 - 0.5 for i in range(16)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cam", ["default", "near"])
def test_a_constant_image_gives_the_isotropic_frame(cam, mode):
    """premultiplied values 0 and 1 are exact in binary16 and N fl(1 / N) = 1 for N <= 16: every tap returns the colour and so does the mean"""
    W, H = 96, 64
    colour = (255, 0, 255)
    u, rgba, vis = plain(W, H, cam, VIRIDIS, mode)
    taps = set()
    for size in ((1, 1), (37, 53), (300, 7)):
        img = np.zeros((size[1], size[0], 4), np.uint8)
        img[:] = (*colour, 255)
        for filt in ("linear", "nearest"):
            flat, flat_again = drm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, extent=drm.EXTENT, filter=filt, shade_mode=mode)
            for bias in (-16.0, -1.0, 0.0, 1.5, 16.0):
                want, want_again = dmm.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, extent=drm.EXTENT, filter=filt, bias=bias, shade_mode=mode)
                assert np.array_equal(want, flat) and np.array_equal(want_again, flat_again)
                for A in AS:
                    frame, again, s = dam.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, extent=drm.EXTENT, filter=filt, bias=bias, shade_mode=mode,
                                                max_anisotropy=A, want_sample=True)
                    assert np.array_equal(again, want_again) and np.array_equal(frame, want), (size, filt, bias, A)
                    taps |= set(s[..., 7][again].astype(int).tolist())
    assert {1, 2, 3, 16} <= taps, taps                        # one tap, even, odd and the largest count took part


@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_the_level_of_detail_never_rises(cam):
    W, H = 257, 131
    u, rgba, vis = plain(W, H, cam)
    img = dmm.case_image()
    kw = dict(extent=dam.CASE_EXTENT[cam], bias=0.5, want_sample=True)
    _, again1, s1 = dam.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, max_anisotropy=1, **kw)
    for A in AS:
        _, again, s = dam.frame(rgba, vis, u, heights(), GRID, VIRIDIS, img, max_anisotropy=A, **kw)
        both = again & again1
        assert both.sum() > 0.9 * again1.sum()
        lod, lod1, n = s[..., 6][both], s1[..., 6][both], s[..., 7][both]
        assert (lod <= lod1).all(), (cam, A)
        one = n == 1
        assert one.any() and np.array_equal(lod[one], lod1[one])
        assert (lod[~one] < lod1[~one]).mean() > 0.9          # (the piecewise-linear logarithm is monotone, and nearly always strictly)


@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_the_tap_count_is_the_footprints_ratio(cam):
    """N against min(A, ceil(sqrt(amax / amin))) in binary64 from the geometry-buffer model's world positions of the pixel, its right and
    its lower neighbour, where the three carry one visibility id; a ratio within a relative 1e-3 of an integer or of 1.25 may fall
    either way in binary32 and is exempt, and those are few"""
    import oracle
    W, H, grid = 257, 131, 24                                 # (a coarse grid: at the scenes' 1024 no primitive spans two pixels)
    u = uniforms(W, H, cam)
    rgba, vis = oracle.render_terrain(u, W, H, grid, heights(), VIRIDIS, want_vis=True, nthreads=8, shade_mode=oracle.SHADE_REFERENCE)
    rgba = rgba.reshape(H, W, 4)
    iw, ih = dmm.CASE_SIZE
    ext = np.array(dam.CASE_EXTENT[cam], f32)
    _, pos, _ = gbm.planes(vis, u, heights(), grid)
    x, z = pos[..., 0].astype(np.float64) / float(u[36]), pos[..., 2].astype(np.float64) / float(u[36])
    same = np.zeros((H, W), bool)
    same[:-1, :-1] = (vis[:-1, :-1] == vis[:-1, 1:]) & (vis[:-1, :-1] == vis[1:, :-1])
    sx, sz = float(f32(iw) / (ext[2] - ext[0])), float(f32(ih) / (ext[3] - ext[1]))
    ax, ay = np.zeros((H, W)), np.zeros((H, W))
    ax[:-1, :-1] = ((x[:-1, 1:] - x[:-1, :-1]) * sx) ** 2 + ((z[:-1, 1:] - z[:-1, :-1]) * sz) ** 2
    ay[:-1, :-1] = ((x[1:, :-1] - x[:-1, :-1]) * sx) ** 2 + ((z[1:, :-1] - z[:-1, :-1]) * sz) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.sqrt(np.maximum(ax, ay) / np.minimum(ax, ay))
    for A in AS:
        _, again, s = dam.frame(rgba, vis, u, heights(), grid, VIRIDIS, dmm.case_image(), extent=ext, max_anisotropy=A, want_sample=True)
        pick = same & again & np.isfinite(ratio)
        assert pick.sum() > 0.3 * again.sum()
        r, n, ym = ratio[pick], s[..., 7][pick].astype(np.int64), s[..., 8][pick]
        near = (np.abs(r - np.round(r)) <= 1e-3 * r) | (np.abs(r - 1.25) <= 1e-3 * 1.25)
        want = np.where(r <= 1.25, 1, np.minimum(A, np.ceil(r))).astype(np.int64)
        wrong = (n != want) & ~near
        print(f"{cam} A = {A}: {pick.sum()} pixels, ratio {r.min():.3f} ... {r.max():.3f}, mean N {n.mean():.2f}, {near.sum()} exempt, {wrong.sum()} wrong")
        assert not wrong.any(), (cam, A, r[wrong][:5], n[wrong][:5], want[wrong][:5])
        assert near.mean() <= 0.02, near.mean()
        many = n > 1
        assert np.array_equal(ym[many] == 1, (ay > ax)[pick][many])       # the major axis is the longer one


# the ratio rms(A = 8) / rms(A = 1) the model measures in the test below (printed there); the bound asserted lies halfway to 1
QUALITY_RATIO = 0.858


def test_quality_against_a_supersampled_reference():
    """On a flat height field with a constant colormap the terrain is one colour and the frame's detail is the image's alone.  The
    reference integrates the image over each pixel: the unmipped `nearest` drape on the oracle's frame at (8 W, 8 H), decoded to linear
    light and box-averaged 8 x 8.  The model's (W, H) frames are compared with it in linear light over their rewritten pixels."""
    import oracle
    W, H, F, grid = 96, 64, 8, 64
    lut = constant_lut((200, 180, 90))
    h = np.zeros((16, 16), f32)
    img = dmm.case_image()
    decode = oracle.srgb_tables()[0].astype(np.float64)

    def base(w, hh):
        u = uniforms(w, hh, "default")
        rgba, vis = oracle.render_terrain(u, w, hh, grid, h, lut, want_vis=True, nthreads=8, shade_mode=oracle.SHADE_REFERENCE)
        return u, rgba.reshape(hh, w, 4), vis

    u8, rgba8, vis8 = base(F * W, F * H)
    fine, _ = drm.frame(rgba8, vis8, u8, h, grid, lut, img, filter="nearest")
    ref = decode[fine[..., :3]].reshape(H, F, W, F, 3).mean(axis=(1, 3))
    u, rgba, vis = base(W, H)
    rms, masks = {}, {}
    for A in (1, 8):
        frame, again = dam.frame(rgba, vis, u, h, grid, lut, img, filter="linear", bias=0.0, max_anisotropy=A)
        masks[A] = again
        rms[A] = frame
    both = masks[1] & masks[8]
    assert both.sum() > 0.9 * masks[1].sum() and both.sum() > 0.05 * W * H      # (the camera sees the grid in a part of the frame)
    for A in (1, 8):
        rms[A] = float(np.sqrt(((decode[rms[A][..., :3]] - ref)[both] ** 2).mean()))
    ratio = rms[8] / rms[1]
    print(f"rms error in linear light over {both.sum()} pixels: A = 1 {rms[1]:.5f}, A = 8 {rms[8]:.5f}, ratio {ratio:.3f}")
    assert rms[8] < rms[1]
    assert ratio < 0.5 * (1.0 + QUALITY_RATIO)


def case_shares(cam, A, W=257, H=131):
    u, rgba, vis = plain(W, H, cam)
    _, again, s = dam.frame(rgba, vis, u, heights(), GRID, VIRIDIS, dmm.case_image(), extent=dam.CASE_EXTENT[cam], bias=0.0, max_anisotropy=A,
                            want_sample=True)
    return u, vis, again, s


def test_the_gpu_tests_case_reaches_the_code():
    W, H = 257, 131
    levels = len(dmm.sizes(*dmm.CASE_SIZE))
    xmajor = ymajor = total = 0
    for cam in ("default", "fill", "near"):
        u, vis, again, s = case_shares(cam, 16)
        n, lod, ym = s[..., 7][again], s[..., 6][again], s[..., 8][again]
        many = n > 1
        sh = {"N = 1": (n == 1).mean(), "N = 16": (n == 16).mean(), "1 < N < 16": (many & (n < 16)).mean(), "level 0": (many & ~(lod > 0)).mean(),
              "blend": (many & (lod > 0) & (lod < levels - 1) & (lod != np.floor(lod))).mean()}
        for A in (2, 4, 8):
            _, _, againA, sA = case_shares(cam, A)
            sh[f"N = {A}"] = (sA[..., 7][againA] == A).mean()
        print(f"{cam}: {again.sum()} rewritten, mean N {n.mean():.2f}; " + ", ".join(f"{k} {v:.3f}" for k, v in sh.items())
              + f"; x-major {(many & (ym == 0)).mean():.3f}, y-major {(many & (ym == 1)).mean():.3f}")
        assert again.sum() > 0.1 * (vis != 0).sum()
        assert sh["N = 1"] >= 0.02
        for A in AS:
            assert sh[f"N = {A}"] >= 0.02, (cam, A)
        assert sh["1 < N < 16"] >= 0.05 and sh["level 0"] >= 0.05 and sh["blend"] >= 0.05
        xmajor += (many & (ym == 0)).sum(); ymajor += (many & (ym == 1)).sum(); total += again.sum()
        if cam == "near":
            cut = dam.clipped_mask(vis, u, heights(), GRID) & again
            print(f"near: {cut.sum()} rewritten pixels show a primitive cut by the near or far plane, {(s[..., 7][cut] > 1).sum()} of them with N > 1")
            assert (s[..., 7][cut] > 1).any()
    assert xmajor >= 0.02 * total and ymajor >= 0.02 * total
    # an extent inside the grid: taps near its edge leave the image rectangle and are clamped
    u, rgba, vis = plain(W, H, "fill")
    _, again, s = dam.frame(rgba, vis, u, heights(), GRID, VIRIDIS, dmm.case_image(), extent=dam.INTERIOR_EXTENT, max_anisotropy=16, want_sample=True)
    print(f"interior extent: {int(s[..., 9][again].sum())} of {again.sum()} rewritten pixels have a clamped tap")
    assert s[..., 9][again].sum() > 0

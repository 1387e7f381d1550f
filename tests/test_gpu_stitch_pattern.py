"""k_stitch_tiles and k_stitch_bands on gather buffers in which every 32-bit word says where it lies:
    tiles:  rank << 24 | local_tile << 12 | y_in_tile << 6 | x_in_tile        bands:  rank << 24 | local_row << 12 | x
and every slot that no tile owns holds a poison word.  The expected image is built here from the rule include/vf_hip.h prints
(tile owner ((tx >> stripe_log2) + skew * ty) % nranks, or owner[tx >> stripe_log2] of a registered map; local tiles dense and
row-major by (ty, tx); row y belongs to rank (y / band_h) % nranks, owned rows dense in band order) -- not from vf_tile_layout, which
is checked against the same rule on the side.  A misplaced tile, row or 16-byte group cannot hide in such a frame."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 64
POISON, UNWRITTEN = 0xFFFFFFFF, 0xEEEEEEEE


class Device:
    """a context of the library plus raw device buffers of the HIP runtime it already loaded (as tests/test_gpu_c5.py does)"""

    def __init__(self):
        from vulkan_forge_amd import cabi
        self.cabi, self.lib = cabi, cabi.load()
        self.ctx = C.c_void_p()
        assert self.lib.vf_ctx_create(0, C.byref(self.ctx)) == cabi.VF_OK, self.lib.vf_last_error()
        di = cabi.DeviceInfo()
        assert self.lib.vf_ctx_device_info(self.ctx, C.byref(di)) == cabi.VF_OK
        # vf_stitch_tiles_device launches min(tiles, cap) workgroups: one per compute unit unless VF_STITCH_WGS says otherwise
        self.block_cap = max(1, int(os.environ.get("VF_STITCH_WGS") or di.compute_units))
        hip = self.hip = C.CDLL("libamdhip64.so.7")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def close(self):
        self.lib.vf_ctx_destroy(self.ctx)

    def upload(self, a, pad=0):
        """device copy of `a` (+ pad bytes behind it)"""
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), a.nbytes + pad) == 0
        assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0                  # hipMemcpyHostToDevice
        return p.value

    def download(self, ptr, shape):
        out = np.empty(shape, np.uint32)
        assert self.hip.hipDeviceSynchronize() == 0
        assert self.hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0            # hipMemcpyDeviceToHost
        return out

    def free(self, *ptrs):
        for p in ptrs:
            assert self.hip.hipFree(p) == 0


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


# ---- the rule, in numpy -----------------------------------------------------------------------------------------------------------
def tile_owner(ntx, nty, nranks, skew, stripe_log2, owner_map=None):
    tx, ty = np.meshgrid(np.arange(ntx), np.arange(nty))
    if owner_map is not None:
        return np.asarray(owner_map)[tx >> stripe_log2].astype(np.int64)
    return ((tx >> stripe_log2) + skew * ty) % nranks


def tile_case(W, H, nranks, skew, stripe_log2, extra_stride, owner_map=None):
    """(gather buffer [nranks][stride][64][64], expected image (H, W), stride, owner grid)"""
    ntx, nty = -(-W // T), -(-H // T)
    own = tile_owner(ntx, nty, nranks, skew, stripe_log2, owner_map)
    local = np.zeros_like(own)
    counts = []
    for r in range(nranks):
        m = own == r
        local[m] = np.arange(m.sum())                                                  # row-major by (ty, tx)
        counts.append(int(m.sum()))
    stride = max(counts) + extra_stride
    assert nranks <= 255 and stride < 4096
    inner = (np.arange(T)[:, None] << 6 | np.arange(T)[None, :]).astype(np.uint32)
    gathered = np.full((nranks, stride, T, T), POISON, np.uint32)
    for r in range(nranks):
        gathered[r, :counts[r]] = np.uint32(r << 24) | (np.arange(counts[r], dtype=np.uint32) << 12)[:, None, None] | inner
    head = (own << 24 | local << 12).astype(np.uint32)
    y, x = np.arange(H), np.arange(W)
    image = head[(y // T)[:, None], (x // T)[None, :]] | inner[(y % T)[:, None], (x % T)[None, :]]
    return gathered, image, stride, own


def run_tiles(dev, W, H, nranks, layout, gathered, stride, offset_words=0):
    d_g = dev.upload(gathered)
    d_i = dev.upload(np.full(H * W + offset_words, UNWRITTEN, np.uint32), pad=16)
    try:
        rc = dev.lib.vf_stitch_tiles_device(dev.ctx, C.c_void_p(d_g), C.c_void_p(d_i + 4 * offset_words), W, H, nranks, layout, stride, None)
        assert rc == dev.cabi.VF_OK, dev.lib.vf_last_error()
        out = dev.download(d_i, (H * W + offset_words,))
    finally:
        dev.hip.hipDeviceSynchronize()
        dev.free(d_g, d_i)
    assert (out[:offset_words] == UNWRITTEN).all()
    return out[offset_words:].reshape(H, W)


def check_image(got, want, what):
    assert not (got == POISON).any() and not (got == UNWRITTEN).any(), what
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), [(int(y), int(x), hex(got[y, x]), hex(want[y, x])) for y, x in np.argwhere(bad)[:4]])


def check_layout(dev, W, H, nranks, layout, own):
    """vf_tile_layout (host arithmetic) lists the same tiles in the same order"""
    for r in range(nranks):
        ty, tx = np.nonzero(own == r)
        assert np.array_equal(dev.cabi.tile_layout(W, H, r, nranks, layout, lib=dev.lib), np.stack([tx, ty], axis=1)), (W, H, r, nranks, hex(layout))


FRAMES = [(64, 64), (128, 64), (130, 70), (131, 129), (200, 65), (1, 1), (1, 130), (1000, 520)]


@pytest.mark.parametrize("W,H", FRAMES, ids=lambda v: str(v))
def test_tiles_every_layout(dev, W, H):
    """ranks 1, 2, 3, 4, 8 x skew 0, 1, 3 x stripes of 1, 2, 4 tiles; the stride of the largest shard and a larger one in turn"""
    k = 0
    for nranks in (1, 2, 3, 4, 8):
        for skew in (0, 1, 3):
            for stripe_log2 in (0, 1, 2):
                gathered, want, stride, own = tile_case(W, H, nranks, skew, stripe_log2, extra_stride=(0, 3)[k % 2])
                layout = skew | stripe_log2 << 16
                check_image(run_tiles(dev, W, H, nranks, layout, gathered, stride), want, (W, H, nranks, skew, stripe_log2, stride))
                if (W, H) in ((130, 70), (1000, 520)):
                    check_layout(dev, W, H, nranks, layout, own)
                k += 1


def test_tiles_more_tiles_than_workgroups(dev):
    """the smallest frame of two tile rows with more tiles than the launch has workgroups: the tile loop takes a second trip"""
    ntx = dev.block_cap // 2 + 1
    W, H = T * (ntx - 1) + 1, T + 1
    assert 2 * ntx > dev.block_cap >= 2 * (ntx - 1) and 2 * ntx < 4096
    for nranks, skew, stripe_log2 in ((1, 0, 0), (3, 1, 1), (8, 3, 0)):
        gathered, want, stride, own = tile_case(W, H, nranks, skew, stripe_log2, extra_stride=1)
        check_image(run_tiles(dev, W, H, nranks, skew | stripe_log2 << 16, gathered, stride), want, (W, H, nranks, skew, stripe_log2))


@pytest.mark.parametrize("wgs", [1, 3, 7])
def test_tiles_loop_wraps_under_a_forced_workgroup_count(dev, monkeypatch, wgs):
    """VF_STITCH_WGS (read at every call) forces 1, 3 or 7 workgroups: 144 tiles then take up to 144 trips of the tile loop whatever
    the device's compute-unit count is, so the wrap stays tested if the default cap moves"""
    monkeypatch.setenv("VF_STITCH_WGS", str(wgs))
    for W, H, nranks, skew, stripe_log2 in ((1000, 520, 3, 1, 1), (200, 65, 2, 3, 0)):
        gathered, want, stride, _ = tile_case(W, H, nranks, skew, stripe_log2, extra_stride=1)
        check_image(run_tiles(dev, W, H, nranks, skew | stripe_log2 << 16, gathered, stride), want, (wgs, W, H))


@pytest.mark.parametrize("W,H", [(64, 64), (128, 64), (1000, 520)], ids=lambda v: str(v))
def test_tiles_image_base_off_by_four_bytes(dev, W, H):
    """W % 4 == 0 and an image pointer that is not 16-byte aligned: the kernel has to store word by word"""
    for nranks, skew, stripe_log2 in ((1, 0, 0), (2, 1, 0), (4, 0, 1)):
        gathered, want, stride, _ = tile_case(W, H, nranks, skew, stripe_log2, extra_stride=0)
        check_image(run_tiles(dev, W, H, nranks, skew | stripe_log2 << 16, gathered, stride, offset_words=1), want, (W, H, nranks, skew, stripe_log2))


def test_tiles_registered_owner_maps(dev):
    """vf_balance_stripes' deal of eight stripes of two tile columns, and a table written by hand"""
    W, H, shift = 1000, 520, 1                                                        # 16 x 9 tiles, 8 stripes
    ms = np.random.default_rng(4).uniform(0.1, 3.0, 8).astype(np.float32)
    for nranks, owner in ((2, None), (4, None), (3, np.array([2, 0, 0, 1, 2, 2, 1, 0], np.uint8))):
        if owner is None:
            owner = dev.cabi.balance_stripes(ms, nranks, lib=dev.lib)
            assert np.array_equal(np.bincount(owner, minlength=nranks), np.full(nranks, 8 // nranks))
        layout = dev.cabi.register_stripe_map(owner, shift, nranks, lib=dev.lib)
        gathered, want, stride, own = tile_case(W, H, nranks, 0, shift, extra_stride=2, owner_map=owner)
        check_image(run_tiles(dev, W, H, nranks, layout, gathered, stride), want, (nranks, owner.tolist()))
        check_layout(dev, W, H, nranks, layout, own)
        gathered, want, stride, _ = tile_case(130, 70, nranks, 0, shift, extra_stride=0, owner_map=owner)     # the same map, word by word
        check_image(run_tiles(dev, 130, 70, nranks, layout, gathered, stride), want, ("130x70", nranks, owner.tolist()))


def test_tiles_refuse_a_stride_below_the_largest_shard(dev):
    gathered, _, stride, _ = tile_case(200, 65, 2, 1, 0, extra_stride=0)
    d_g, d_i = dev.upload(gathered), dev.upload(np.full(200 * 65, UNWRITTEN, np.uint32))
    try:
        assert dev.lib.vf_stitch_tiles_device(dev.ctx, C.c_void_p(d_g), C.c_void_p(d_i), 200, 65, 2, 1, stride - 1, None) == dev.cabi.VF_ERR_INVALID
        assert (dev.download(d_i, (200 * 65,)) == UNWRITTEN).all()
    finally:
        dev.free(d_g, d_i)


# ---- bands ------------------------------------------------------------------------------------------------------------------------
def band_case(W, H, nranks, band_h):
    rows = H // nranks
    assert rows < 4096 and W < 4096
    gathered = (np.arange(nranks, dtype=np.uint32)[:, None, None] << 24 | np.arange(rows, dtype=np.uint32)[None, :, None] << 12
                | np.arange(W, dtype=np.uint32)[None, None, :])
    y = np.arange(H)
    b = y // band_h
    r, ly = b % nranks, (b // nranks) * band_h + y % band_h
    image = (r << 24 | ly << 12).astype(np.uint32)[:, None] | np.arange(W, dtype=np.uint32)[None, :]
    return np.ascontiguousarray(gathered), image


@pytest.mark.parametrize("band_h", [1, 2, 64])
@pytest.mark.parametrize("nranks", [1, 2, 3])
def test_bands(dev, band_h, nranks):
    for W in (4, 132):
        for reps in (1, 3):
            H = band_h * nranks * reps
            gathered, want = band_case(W, H, nranks, band_h)
            d_g, d_i = dev.upload(gathered), dev.upload(np.full(H * W, UNWRITTEN, np.uint32))
            try:
                rc = dev.lib.vf_stitch_bands_device(dev.ctx, C.c_void_p(d_g), C.c_void_p(d_i), W, H, nranks, band_h, None)
                assert rc == dev.cabi.VF_OK, dev.lib.vf_last_error()
                got = dev.download(d_i, (H, W))
            finally:
                dev.hip.hipDeviceSynchronize()
                dev.free(d_g, d_i)
            check_image(got, want, (W, H, nranks, band_h))


@pytest.mark.parametrize("W,H,nranks,band_h,why", [(6, 8, 2, 2, "width"), (8, 10, 2, 2, "height"), (8, 12, 2, 3, "band_h"), (8, 8, 0, 2, "nranks")])
def test_bands_refusals_launch_nothing(dev, W, H, nranks, band_h, why):
    d_g, d_i = dev.upload(np.zeros(H * W, np.uint32)), dev.upload(np.full(H * W, UNWRITTEN, np.uint32))
    try:
        assert dev.lib.vf_stitch_bands_device(dev.ctx, C.c_void_p(d_g), C.c_void_p(d_i), W, H, nranks, band_h, None) == dev.cabi.VF_ERR_INVALID, why
        assert (dev.download(d_i, (H * W,)) == UNWRITTEN).all()
    finally:
        dev.free(d_g, d_i)

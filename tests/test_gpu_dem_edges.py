"""The DEM kernels (k_dem_ingest, k_dem_minmaxsum, k_dem_sqdev, k_dem_normalize, k_dem_sample) against tests/dem_model.py at the
sizes and values where a reduction, a grid stride or a conversion goes wrong -- through cabi.Dem, the C-ABI itself.

What is compared how:
  ingest, the texture round trip, min / max, the percentile range, normalisation given the reported statistics: equality
      (bit for bit; min / max and every NaN numerically: -0 == +0, NaN == NaN);
  mean: within one f32 step of the f64 mean rounded to f32 -- the library adds in f64, only the last rounding can differ;
  std:  within one f32 step of the model's arithmetic (f32 deviations from the reported f32 mean, squared in f32, added in f64) --
        the two differ in the order of an f64 sum alone.
The planted +-1000 among noise in [-1, 1] make a dropped tail, a dropped block or a dropped second trip of the grid stride show in an
extreme AND in the mean (2000 / n or 1000 / n, thousands of f32 steps of a mean near 0 even at the largest size)."""
import numpy as np
import pytest

import dem_model as dm

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS = 1e-8                                                    # normalize_terrain's default
BIG_EPS = 4096.0                                              # above the spread (2000) and the std of the planted maps


@pytest.fixture()
def dem():
    from vulkan_forge_amd import cabi
    d = cabi.Dem()
    yield d
    d.close()


def texture(d):
    d.upload()
    return d.read_patch()


def close_f32(got, want):
    """equal, both NaN, or finite and at most one f32 step apart"""
    got, want = F32(got), F32(want)
    if not (np.isfinite(got) and np.isfinite(want)):
        return dm.same(got, want)
    return dm.ulp_distance(got, want) <= 1


def check_stats(d, h):
    """h: the ingested map (float32).  Returns the reported statistics."""
    st = d.stats()
    mn, mx, m64, _ = dm.stats(h)
    with np.errstate(over="ignore"):
        want_mean = F32(m64)
    want_std = dm.std_of(h, st[2])
    print(f"n={h.size} min {st[0]!r} / {mn!r}  max {st[1]!r} / {mx!r}  mean {st[2]!r} / {want_mean!r}  std {st[3]!r} / {want_std!r}")
    assert dm.same(st[0], mn) and dm.same(st[1], mx), (st, mn, mx)
    assert close_f32(st[2], want_mean), (st[2], want_mean)
    assert close_f32(st[3], want_std), (st[3], want_std)
    return st


# ---- planted extremes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hi_at,lo_at", dm.planted_cases())
def test_planted_extremes(dem, n, hi_at, lo_at):
    h = dm.planted_map(n, hi_at, lo_at)
    dem.set_heights(h)
    st = check_stats(dem, h)
    assert st[1] == (1000.0 if hi_at is not None else h.max()) and st[0] == (-1000.0 if lo_at is not None else h.min())
    assert np.array_equal(texture(dem).view(np.uint32), h.view(np.uint32))


@pytest.mark.parametrize("n", [64, 868, 524289 + 300])
def test_every_sample_counts_in_the_sums(dem, n):
    """h[k] = k + 1: integers whose f64 sum is exact, so the mean is (n + 1) / 2 rounded once whichever lanes, waves, blocks and trips
    added it; half a wave, a wave of a block or a trip left out moves it by a quarter of itself"""
    h = np.arange(1, n + 1, dtype=F32).reshape(1, n)
    dem.set_heights(h)
    st = check_stats(dem, h)
    assert st[0] == 1.0 and st[1] == n and st[2] == F32((n + 1) / 2)


@pytest.mark.parametrize("n", dm.STATS_WRAP_SIZES[2:] + dm.INGEST_WRAP_SIZES)
def test_std_sees_the_later_trips_of_the_grid_stride(dem, n):
    """zeros up to sample 524 288, +-3 in turn from there on: every deviation that counts lies beyond the first trip of the stride loop,
    and a sum of squares that stopped after it would be 0"""
    h = np.zeros((1, n), F32)
    h[0, dm.STATS_GRID:] = np.where(np.arange(n - dm.STATS_GRID) % 2 == 0, F32(3.0), F32(-3.0))
    dem.set_heights(h)
    st = check_stats(dem, h)
    assert st[3] > 0 and abs(float(st[3]) - 3.0 * np.sqrt((n - dm.STATS_GRID) / n)) < 1e-5


# ---- values ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dm.VALUE_MAP_NAMES)
@pytest.mark.parametrize("n", [1000, 524289])
def test_values(dem, oracle, n, name):
    src = dm.value_maps(n)[name]
    h = dm.ingest(src, 1.0)
    dem.set_heights(src)
    assert dm.same_bits(texture(dem), h)                                           # the ingest (f64 -> f32 conversions included)
    st = check_stats(dem, h)
    if name in ("nan_first", "all_nan"):
        assert np.isnan(st[0]) and np.isnan(st[1])
    elif name in ("nan_middle", "nan_last"):
        assert st[0] == np.nanmin(h) and st[1] == np.nanmax(h) and np.isnan(st[2]) and np.isnan(st[3])
    elif name == "inf":
        assert st[1] == np.inf and st[2] == np.inf and np.isnan(st[3])
    elif name == "constant":
        assert st == (3.25, 3.25, 3.25, 0.0)
    elif name == "everest":
        assert abs(float(st[3]) - float(h.astype(np.float64).std())) < 1e-6          # a one-pass f32 E[x^2] - E[x]^2 is off by ~1 here
    elif name.startswith("zeros"):
        assert st[0] == 0.0 and st[1] == 0.0 and st[2] == 0.0 and st[3] == 0.0
    for mode, lo, hi in (("minmax", -2.0, 7.0), ("zscore", 0.0, 1.0)):
        dem.set_heights(src)
        dem.normalize(mode, lo, hi, EPS)
        got = texture(dem)
        assert dm.same_bits(got, dm.normalize(h, mode, lo, hi, EPS, st)), (name, mode)
        if mode == "minmax":
            assert dm.same_bits(got, oracle.dem_normalize(h, "minmax", eps=EPS, out_range=(lo, hi))), name
            if name in ("nan_first", "all_nan"):
                assert np.isnan(got).all()
            elif name == "nan_middle":
                assert np.isnan(got).sum() == 1
        elif name == "constant":
            assert (got == 0.0).all()                                              # (v - mean) / max(0, eps)


@pytest.mark.parametrize("n", dm.INGEST_WRAP_SIZES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ingest_past_its_grid_stride(dem, n, dtype):
    src = np.random.default_rng(n).uniform(-3.0, 3.0, (1, n)).astype(dtype)
    src[0, -1], src[0, 4096 * 256 - 2] = 1234.5, -77.25                             # the last sample and one of the last block of the first trip
    dem.set_heights(src, 2.5)
    assert np.array_equal(texture(dem).view(np.uint32), dm.ingest(src, 2.5).view(np.uint32))


# ---- normalize -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1000,) + dm.INGEST_WRAP_SIZES)
@pytest.mark.parametrize("mode", ["minmax", "zscore"])
@pytest.mark.parametrize("eps", [EPS, BIG_EPS])
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-2.0, 7.0), (5.0, 5.0)])
def test_normalize_is_the_formula_bit_for_bit(dem, oracle, n, mode, eps, lo, hi):
    h = dm.planted_map(n, 0, (n - 1) // 256 * 256)
    h[0, 1:n - 1:7] *= F32(0.001)                                                   # quotients and products of every size
    dem.set_heights(h)
    st = dem.stats()
    dem.normalize(mode, lo, hi, eps)
    got = texture(dem)
    want = dm.normalize(h, mode, lo, hi, eps, st)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])
    if mode == "minmax":
        assert np.array_equal(got.view(np.uint32), oracle.dem_normalize(h, "minmax", eps=eps, out_range=(lo, hi)).view(np.uint32))
        if lo == hi:
            assert (got == lo).all()
    elif eps == BIG_EPS:
        assert st[3] < BIG_EPS and np.array_equal(got, (h - st[2]) / F32(BIG_EPS))      # the divisor is eps


def test_minmax_after_a_nan_first_map_is_all_nan(dem):
    h = dm.value_maps(257)["nan_first"]
    dem.set_heights(h)
    st = dem.stats()
    assert np.isnan(st[0]) and np.isnan(st[1])
    dem.normalize("minmax", 0.0, 1.0, EPS)
    assert np.isnan(texture(dem)).all()


# ---- percentile range ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 1000)] + list(dm.PERCENTILE_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_percentile_range(dem, oracle, shape):
    h = dm.permutation_map(shape)
    dem.set_heights(h)
    got = dem.percentile_range()
    want = dm.percentile_range(h)
    print(shape, got, want)
    assert got == want and (float(got[0]), float(got[1])) == oracle.dem_percentile_range(h)
    assert np.array_equal(texture(dem), h)                                          # sampling leaves the map alone


@pytest.mark.parametrize("shape", [(1, 1000), (1, 200000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_percentile_range_with_ties(dem, oracle, shape):
    h = dm.tied_map(shape)
    dem.set_heights(h)
    got = dem.percentile_range()
    assert got == dm.percentile_range(h) and (float(got[0]), float(got[1])) == oracle.dem_percentile_range(h)


# ---- one handle, maps of shrinking size ------------------------------------------------------------------------------------------
def test_a_handle_serves_the_current_map_only(dem):
    """300 x 1000 float64, then 7 x 5 float32, then 1 x 1: capacity, staging and partial sums of the larger map stay allocated and
    must not be read.  The percentile range of the first map samples into the staging buffer (step 4)."""
    big = dm.permutation_map((300, 1000)).astype(np.float64) - 150000.0
    small = np.random.default_rng(3).uniform(50.0, 60.0, (7, 5)).astype(F32)          # apart from anything the big map leaves behind
    one = np.array([[42.5]], F32)
    for src in (big, small, one):
        h = dm.ingest(src, 1.0)
        dem.set_heights(src)
        check_stats(dem, h)
        assert dem.percentile_range() == dm.percentile_range(h)
        assert np.array_equal(texture(dem), h) and dem.texture_size() == (h.shape[1], h.shape[0])
        st = dem.stats()
        dem.normalize("zscore", 0.0, 1.0, EPS)
        assert dm.same_bits(texture(dem), dm.normalize(h, "zscore", 0.0, 1.0, EPS, st))
        dem.set_heights(src)
        dem.normalize("minmax", -2.0, 7.0, EPS)
        assert dm.same_bits(texture(dem), dm.normalize(h, "minmax", -2.0, 7.0, EPS, st))
    # the texture keeps its own size when a smaller map arrives after the upload
    dem.set_heights(small)
    dem.upload()
    dem.set_heights(one)
    assert dem.texture_size() == (5, 7)
    assert np.array_equal(dem.read_patch(), small) and np.array_equal(dem.read_patch(1, 2, 3, 4), small[2:6, 1:4])
    from vulkan_forge_amd import cabi
    with pytest.raises(cabi.VfError, match="exceeds texture bounds in x"):
        dem.read_patch(3, 0, 3, 1)
    assert dem.stats() == (42.5, 42.5, 42.5, 0.0)

"""tests/dem_model.py (numpy, written from the header and the reference's Rust) against the oracle's dem_* functions (C, the reference's
sequential f32 loops), on the CPU.  Where the two must agree exactly they do: the ingest, min / max -- a NaN first sample included --,
normalisation given the same statistics, the percentile range.  The mean and the std agree exactly on maps whose sequential f32
sums are exact, which is where a sequential f32 sum and an f64 sum say the same.

The NaN-first rule: the reference starts min and max at heights[0], so a NaN there stays (min = max = NaN, and minmax-normalising the
map gives all NaN).  Model and oracle agree on it here; the library passed every NaN over and reported the finite extremes until
tests/test_gpu_dem_edges.py asked."""
import ctypes as C

import numpy as np
import pytest

import dem_model as dm

F32 = np.float32


def oracle_normalize(oracle, h, mode, lo, hi, eps, st):
    """vfo_dem_normalize with the statistics handed in (oracle.dem_normalize computes its own)"""
    out = np.array(h, dtype=F32, order="C")
    stv = np.array(st, F32)
    f32p = C.POINTER(C.c_float)
    oracle.lib().vfo_dem_normalize(out.ctypes.data_as(f32p), out.size, 1 if mode == "zscore" else 0, eps, lo, hi, stv.ctypes.data_as(f32p))
    return out


@pytest.mark.parametrize("name", dm.VALUE_MAP_NAMES)
@pytest.mark.parametrize("ex", [1.0, 2.5])
def test_ingest_is_the_oracles_bit_for_bit(oracle, name, ex):
    src = dm.value_maps(1000)[name]
    assert dm.same_bits(dm.ingest(src, ex), oracle.dem_ingest(src, ex))


def test_ingest_of_float64_rounds_overflows_and_denormalises():
    """the model's own conversions, stated as numbers"""
    src = np.array([[1e39, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, 1e-40]], np.float64)
    got = dm.ingest(src, 1.0)[0]
    assert got[0] == np.inf and got[1] == 1.0 and got[2] == F32(1.0) + F32(2.0 ** -22)
    assert got[3].view(np.uint32) == 1 and got[4] == 0.0 and got[5].view(np.uint32) == 2 and 0 < got[6] < 2.0 ** -126


@pytest.mark.parametrize("name", dm.VALUE_MAP_NAMES)
def test_min_max_are_the_oracles(oracle, name):
    h = dm.ingest(dm.value_maps(1000)[name], 1.0)
    mn, mx = dm.min_max(h)
    ost = oracle.dem_stats(h)
    assert dm.same(mn, F32(ost[0])) and dm.same(mx, F32(ost[1])), (mn, mx, ost)


def test_nan_first_gives_nan_min_and_max_and_an_all_nan_minmax(oracle):
    h = dm.value_maps(1000)["nan_first"]
    assert np.isnan(h[0, 0]) and np.isfinite(h[0, 1:]).all()
    for st in (oracle.dem_stats(h), dm.stats(h)):
        assert np.isnan(st[0]) and np.isnan(st[1])
    assert np.isnan(oracle.dem_normalize(h, "minmax", out_range=(-2.0, 7.0))).all()
    mn, mx, m64, sd = dm.stats(h)
    assert np.isnan(dm.normalize(h, "minmax", -2.0, 7.0, 1e-8, (mn, mx, F32(m64), sd))).all()
    for other in ("nan_middle", "nan_last"):                  # a NaN anywhere else is passed over
        o = dm.value_maps(1000)[other]
        st = oracle.dem_stats(o)
        assert st[0] == np.nanmin(o) and st[1] == np.nanmax(o) and dm.same(dm.min_max(o), (F32(st[0]), F32(st[1])))


@pytest.mark.parametrize("name", dm.VALUE_MAP_NAMES)
@pytest.mark.parametrize("mode", ["minmax", "zscore"])
@pytest.mark.parametrize("eps", [1e-8, 10.0])
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-2.0, 7.0), (5.0, 5.0)])
def test_normalize_is_the_oracles_given_the_same_statistics(oracle, name, mode, eps, lo, hi):
    h = dm.ingest(dm.value_maps(1000)[name], 1.0)
    st = np.array(oracle.dem_stats(h), F32)
    assert dm.same_bits(dm.normalize(h, mode, lo, hi, eps, st), oracle_normalize(oracle, h, mode, lo, hi, eps, st))


PERCENTILE_CASES = [(1, n) for n in dm.EDGE_SIZES + dm.STATS_WRAP_SIZES + dm.INGEST_WRAP_SIZES] + list(dm.PERCENTILE_SHAPES)


@pytest.mark.parametrize("shape", PERCENTILE_CASES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_percentile_range_is_the_oracles(oracle, shape):
    for h in (dm.permutation_map(shape), dm.tied_map(shape)):
        want = oracle.dem_percentile_range(h)
        got = dm.percentile_range(h)
        assert (float(got[0]), float(got[1])) == want, (shape, got, want)


def test_percentile_sample_counts():
    """step = n // 65536 above 65536 samples, m = ceil(n / step); 131073 samples its last element"""
    for n, step, m in ((65536, 1, 65536), (65537, 1, 65537), (131071, 1, 131071), (131072, 2, 65536), (131073, 2, 65537), (200000, 3, 66667),
                       (300000, 4, 75000)):
        s = dm.percentile_sample(np.arange(n, dtype=F32))
        assert s.size == m and s[1] == step and s[-1] == (m - 1) * step, n
    assert dm.percentile_sample(np.arange(131073, dtype=F32))[-1] == 131072


@pytest.mark.parametrize("n", [1, 63, 257, 1000, 4096])
def test_mean_and_std_are_the_oracles_where_the_f32_sums_are_exact(oracle, n):
    """Integers below 2^24 / n whose sum is a multiple of n: the sum, the mean, every deviation, every square and the sum of the squares
    (< 64^2 n < 2^24) are exact in f32 in any order, so the oracle's sequential f32 loops and the model's f64 sums are the same numbers
    and one rounding of the quotient remains (f64 then f32 rounds a quotient of f32 values like f32 alone: 53 >= 2 * 24 + 2)."""
    rng = np.random.default_rng(n)
    v = rng.integers(1, 64, n)
    v[: int(v.sum() % n)] -= 1
    assert v.sum() % n == 0 and v.min() >= 0
    h = v.astype(F32).reshape(1, n)
    mn, mx, m64, sd = dm.stats(h)
    ost = oracle.dem_stats(h)
    assert (float(mn), float(mx), float(F32(m64)), float(sd)) == ost
    assert m64 == v.sum() // n and sd == F32(np.sqrt(F32(((v - v.sum() // n) ** 2).sum() / n)))


def test_std_follows_the_mean_it_is_given():
    """the two-pass form: deviations from the f32 mean handed in, not from a mean of its own"""
    h = dm.value_maps(1000)["everest"]
    m = F32(dm.mean64(h))
    assert dm.std_of(h, m) == dm.stats(h)[3] == dm.stats(h, m)[3]
    assert dm.std_of(h, np.nextafter(m, F32(np.inf))) != dm.std_of(h, F32(0.0))
    assert abs(float(dm.std_of(h, m)) - float(h.astype(np.float64).std())) < 1e-6


def test_planted_cases_cover_what_they_claim():
    cases = dm.planted_cases()
    assert {c[0] for c in cases} == set(dm.EDGE_SIZES + dm.STATS_WRAP_SIZES + dm.INGEST_WRAP_SIZES)
    assert (1, 0, None) in cases and (1, None, 0) in cases
    for n, hi, lo in cases:
        for p in (hi, lo):
            assert p is None or 0 <= p < n
        assert hi != lo
    at = {n: {c[1] for c in cases if c[0] == n} for n in (1000, 524288, 524289, 1048575, 1048577)}
    assert at[1000] == {0, 999, 960, 768} and at[524288] == {0, 524287, 524224, 524032} and at[524289] == {0, 524288, 524287}
    assert at[1048575] == {0, 524287, 524288, 1048320, 1048512, 1048574} and at[1048577] == {0, 524287, 524288, 1048576}
    h = dm.planted_map(1000, 960, 999)
    assert h.shape == (1, 1000) and h[0, 960] == 1000 and h[0, 999] == -1000 and np.abs(np.delete(h[0], [960, 999])).max() <= 1

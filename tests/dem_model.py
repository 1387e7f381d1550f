"""A plain numpy statement of the Renderer DEM path, written from the contract in include/vf_hip.h and the reference's Rust
(src/lib.rs:351-388, 905-951; src/terrain_stats.rs:11-35) -- nothing here comes from the library or the oracle, which are both
compared against it (tests/test_dem_model.py on the CPU, tests/test_gpu_dem_edges.py on the GPU)."""
import numpy as np

F32 = np.float32
SAMPLE = 65536


def ingest(src, exaggeration):
    """add_terrain: heights = (f32)src * exaggeration, the product in f32."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(src).astype(F32) * F32(exaggeration)


def min_max(h):
    """The reference starts min and max at heights[0] and replaces them by `<` / `>`: a NaN first sample stays, any other NaN is
    passed over.  (Among zeros of both signs the reference keeps the first it meets; compare these numerically, not by bits.)"""
    h = np.asarray(h, F32).ravel()
    if np.isnan(h[0]):
        return F32(np.nan), F32(np.nan)
    ok = h[~np.isnan(h)]
    return ok.min(), ok.max()


def mean64(h):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(h, F32).ravel().astype(np.float64).sum() / np.float64(np.asarray(h).size)


def std_of(h, mean_f32):
    """d = h - mean and d * d in f32, summed in f64, divided by n, rounded to f32, sqrt in f32."""
    h = np.asarray(h, F32).ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        d = h - F32(mean_f32)
        sq = d * d
        assert d.dtype == F32 and sq.dtype == F32
        return np.sqrt(F32(sq.astype(np.float64).sum() / np.float64(h.size)))


def stats(h, mean_f32=None):
    """(min, max, mean64, std_of(mean_f32)); mean_f32 defaults to mean64 rounded to f32."""
    mn, mx = min_max(h)
    m64 = mean64(h)
    with np.errstate(over="ignore"):
        m32 = F32(m64) if mean_f32 is None else F32(mean_f32)
    return mn, mx, m64, std_of(h, m32)


def normalize(h, mode, lo, hi, eps, st):
    """normalize_in_place with st = (min, max, mean, std) as f32; f32::max / fmaxf pass a NaN operand over, as np.fmax does."""
    h = np.asarray(h, F32)
    mn, mx, mean, std = (F32(v) for v in st)
    lo, hi, eps = F32(lo), F32(hi), F32(eps)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if mode == "minmax":
            denom = np.fmax(np.abs(mx - mn), eps)
            scale = (hi - lo) / denom
            out = (h - mn) * scale + lo
        elif mode == "zscore":
            denom = np.fmax(std, eps)
            out = (h - mean) / denom
        else:
            raise ValueError(mode)
    assert out.dtype == F32
    return out


def percentile_sample(h):
    flat = np.asarray(h, F32).ravel()
    n = flat.size
    step = n // SAMPLE if n > SAMPLE else 1
    return flat[::step]


def percentile_range(h):
    """terrain_stats::min_max(clamp = true); NaN among the samples is out of scope (the reference's sort is unspecified there)."""
    s = np.sort(percentile_sample(h), kind="stable")
    m = F32(s.size)
    return s[int(m * F32(0.01))], s[int(m * F32(0.99))]


def same(a, b):
    """numerically equal, NaN equal to NaN (so -0 == +0)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def same_bits(a, b, nan_any=True):
    """bit for bit; with nan_any every NaN equals every NaN (sign and payload of a produced NaN are not part of the contract)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    eq = a.view(np.uint32) == b.view(np.uint32)
    if nan_any:
        eq |= np.isnan(a) & np.isnan(b)
    return bool(eq.all())


def ulp_distance(a, b):
    """distance in f32 steps between two finite f32 values (0 when equal, -0 == +0)"""
    def key(v):
        u = int(np.array(v, F32).view(np.uint32))
        return -(u & 0x7FFFFFFF) if u >> 31 else u
    return abs(key(a) - key(b))


# ---- the cases both test files use (sizes: the smallest at which each bound of the kernels is exercised) ----------------------
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)                 # wavefront (64) and block (256) edges
STATS_WRAP_SIZES = (524287, 524288, 524289)                       # the statistics kernels' grid stride: 2048 blocks x 256
INGEST_WRAP_SIZES = (1048575, 1048577)                            # ingest / normalize: 4096 blocks x 256
PERCENTILE_SHAPES = ((1, 65536), (1, 65537), (1, 131071),         # step 1: the whole map
                     (1, 131072), (1, 131073),                    # step 2; 131073: m = 65537, the last sample is the last element
                     (1, 200000),                                 # step 3, n % step != 0
                     (300, 1000))                                 # step 4
STATS_GRID = 2048 * 256


def planted_positions(n):
    """0, n - 1, the last multiple of 64 and of 256 below n, and both sides of the statistics kernels' first stride"""
    pos = {0, n - 1, (n - 1) // 64 * 64, (n - 1) // 256 * 256}
    if n > STATS_GRID:
        pos |= {STATS_GRID - 1, STATS_GRID}
    return sorted(pos)


def planted_cases():
    """(n, index of +1000 or None, index of -1000 or None): every position holds each extreme once, the other one sits at the
    next position of the list (a map of one sample holds one of them at a time)"""
    out = []
    for n in EDGE_SIZES + STATS_WRAP_SIZES + INGEST_WRAP_SIZES:
        pos = planted_positions(n)
        if len(pos) == 1:
            out += [(n, pos[0], None), (n, None, pos[0])]
            continue
        for k, p in enumerate(pos):
            out.append((n, p, pos[(k + 1) % len(pos)]))
    return out


def planted_map(n, hi_at, lo_at):
    h = np.random.default_rng(n).uniform(-1.0, 1.0, n).astype(F32)
    if hi_at is not None:
        h[hi_at] = 1000.0
    if lo_at is not None:
        h[lo_at] = -1000.0
    return h.reshape(1, n)


def permutation_map(shape, seed=5):
    """a seeded permutation of 0 .. n-1 (exact in f32 below 2^24): p1 and p99 name the very elements that were sampled"""
    n = shape[0] * shape[1]
    assert n < 1 << 24
    return np.random.default_rng(seed).permutation(n).astype(F32).reshape(shape)


def tied_map(shape, seed=6):
    """many ties: 37 distinct values"""
    return np.random.default_rng(seed).integers(0, 37, shape).astype(F32)


def value_maps(n):
    """name -> (1, n) map of the values a reduction or a conversion can get wrong; float32 unless the name says f64"""
    rng = np.random.default_rng(n + 1)
    noise = rng.uniform(-1.0, 1.0, n).astype(F32)

    def put(at, v):
        h = noise.copy()
        h[at] = v
        return h

    f64_special = np.array([
        1e39, -1e39, 3.4028235677973366e38, 3.4028235e38, -3.5e38,                     # beyond f32: +-inf; the last finite one
        1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50,        # ties: to even down, to even up; just above a tie
        -(1.0 + 2.0 ** -24), 16777217.0, 16777219.0, 0.1,
        1e-40, -1e-40, 2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -40), 3 * 2.0 ** -150,   # f32 subnormals and their ties
        2.0 ** -126 * (1 - 2.0 ** -25), 1e-46, -1e-46, 0.0, -0.0], np.float64)
    f64 = rng.uniform(-1.0, 1.0, n)
    f64[::3] = np.resize(f64_special, f64[::3].size)
    maps = {
        "nan_first": put(0, np.nan),
        "nan_middle": put(n // 2, np.nan),
        "nan_last": put(n - 1, np.nan),
        "all_nan": np.full(n, np.nan, F32),
        "inf": put(n // 3, np.inf),
        "constant": np.full(n, 3.25, F32),
        "everest": (F32(8848.0) + rng.uniform(-0.5, 0.5, n).astype(F32)).astype(F32),
        "zeros_minus_first": np.where(np.arange(n) % 3 == 0, F32(-0.0), F32(0.0)).astype(F32),
        "zeros_plus_first": np.where(np.arange(n) % 3 == 1, F32(-0.0), F32(0.0)).astype(F32),
        "f64_edges": f64,
    }
    return {k: v.reshape(1, n) for k, v in maps.items()}


VALUE_MAP_NAMES = tuple(value_maps(8))

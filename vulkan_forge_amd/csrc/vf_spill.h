// vf_spill.h -- spill analysis: the lowest level the water must reach at the sources before a vertex gets wet (the minimax path
// height), and the sink depth spill - h.
//
//   the keys             key(x) = bits ^ (sign ? 0xFFFFFFFF : 0x80000000) as uint32: the float order on finite values, -0 below +0, and
//                        one answer in bits for min and max.  The kernels work on keys and decode at the end.
//   the tiles            a wave64 holds a 64 x 64 tile of keys in registers, lane = row, register = column.  `hk` (the keys of h, the
//                        key of +inf where h is not finite and beyond the grid) and `w` (the keys of the current spill) are tile-major
//                        and column-major inside a tile: element (tile 64 + b) 64 + r is column b, row r of tile ty ntx + tx;
//                        ntx = ceil(n / 64).  Register b of a wave is one coalesced 256-byte load.
//   k_spill_init         hk from the height cache; w = hk on the border of the grid (EDGES) or the key of +inf; every tile active
//   k_spill_seed         w = hk at a passable seed (the feature's one atomic on the field: a 32-bit atomicMin on the key)
//   k_spill_pass         one wave per tile: the facing column and row of the four neighbours enter, then the tile runs to its own
//                        fixpoint -- a sweep along the registers in both directions and one step across the lanes by shuffles, until no
//                        lane changes.  The host repeats the launch until one changes nothing (SeededFill::fixpoint, vf_hip.hip).  Activity
//                        flags, one word per tile and pass parity: a tile whose neighbours stored nothing in the last pass leaves at once
//   k_spill_out          spill (decoded) and sd = spill - h per vertex, row-major, and the two counts
//   k_spill_tint         blends a shallow and a deep colour over the covered pixels of a frame from its stored visibility, flat: the
//                        flood's tint with another pixel rule (tint_visible and vs_depth_tint, vf_viewshed.h)
//
// Launched only for a handle that asked for the spill: the frame path is not touched.  Every device loop has a fixed trip bound, no
// workgroup waits for another, there is no LDS in the field kernels, and values of `w` only ever fall: a wave that reads a neighbour's
// words while that neighbour stores them sees, per 32-bit word, the old or the new value, both upper bounds of the truth, and the
// next launch sees the new one (the neighbour flags this tile), so every order of evaluation ends in the same greatest fixpoint.
// The state is indexed by compile-time constants only (fully unrolled loops): nothing goes to scratch.  All kernels are templates: the
// library's non-template kernels keep their places.
#pragma once
#include "vf_flood.h"

namespace vf {

constexpr uint32_t kSpillTile = 64;                            // vertices per side of a tile: the registers of the state, the lanes of a wave
constexpr uint32_t kSpillTileWords = kSpillTile * kSpillTile;
constexpr uint32_t kSpillTrips = 4096;                         // k trips settle every in-tile path of k edges, and a tile has 4096 vertices
constexpr uint32_t kSpillInf = 0xFF800000u;                    // key(+inf): no key of a passable vertex reaches it

__device__ __forceinline__ uint32_t spill_key(float x)
{
    const uint32_t b = __float_as_uint(x);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float spill_unkey(uint32_t k) { return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }

// where vertex (i, j) lives in hk and w
__device__ __forceinline__ size_t spill_index(uint32_t ntx, uint32_t i, uint32_t j)
{
    return (((size_t)(j >> 6) * ntx + (i >> 6)) * kSpillTile + (i & 63u)) * kSpillTile + (j & 63u);
}

// blockIdx.x: the tile; blockIdx.y * 4 + wave: the column b of it; lane: the row.  Stores are coalesced, the height cache is gathered.
template <bool EDGES>
__global__ __launch_bounds__(256) void k_spill_init(uint32_t n, uint32_t nb, uint32_t ntx, uint32_t tiles, const float *__restrict__ hblk,
                                                    uint32_t *__restrict__ hk, uint32_t *__restrict__ w, uint32_t *__restrict__ act)
{
    const uint32_t tile = blockIdx.x;
    if (tile >= tiles) return;
    const uint32_t lane = threadIdx.x & 63u, b = blockIdx.y * 4u + (threadIdx.x >> 6);
    const uint32_t ty = tile / ntx, tx = tile - ty * ntx;
    const uint32_t i = tx * kSpillTile + b, j = ty * kSpillTile + lane;
    uint32_t k = kSpillInf;
    if (i < n && j < n) {
        const float h = cached_height(hblk, nb, i, j);
        if (isfinite(h)) k = spill_key(h);
    }
    const bool border = EDGES && i < n && j < n && (i == 0u || j == 0u || i == n - 1u || j == n - 1u);
    const size_t o = ((size_t)tile * kSpillTile + b) * kSpillTile + lane;
    hk[o] = k;
    w[o] = border ? k : kSpillInf;
    if (blockIdx.y == 0u && threadIdx.x == 0u) { act[tile] = 0u; act[tiles + tile] = 1u; }   // (pass 1 reads the second array)
}

// One thread per seed: vertex (ij[2 k], ij[2 k + 1]).  A seed that is not passable is none.
template <int UNUSED>
__global__ __launch_bounds__(256) void k_spill_seed(uint32_t n, uint32_t ntx, const uint32_t *__restrict__ ij, uint32_t count,
                                                    const uint32_t *__restrict__ hk, uint32_t *__restrict__ w)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= count) return;
    const uint32_t i = ij[2u * k], j = ij[2u * k + 1u];
    if (i >= n || j >= n) return;
    const size_t o = spill_index(ntx, i, j);
    const uint32_t key = hk[o];
    if (key != kSpillInf) atomicMin(&w[o], key);
}

// w = max(h, min(w, x)), and the bits it changed into c
#define VF_SPILL_RELAX(h_, w_, x_, c_) do { const uint32_t nv_ = max((h_), min((w_), (x_))); (c_) |= nv_ ^ (w_); (w_) = nv_; } while (0)

// One wave per tile (blockIdx.x = ty ntx + tx), lane = row, register = column.  *changed = 1 when the tile's `w` fell.  act_cur: this
// pass's activity words (read and cleared by the owner only), act_next: the next pass's (only ever set to 1 here).  all != 0: the
// flags are ignored (diagnostics).  `w` is read and written in the same launch by different waves on purpose (see the head of the
// file): no __restrict__ on it.
template <int UNUSED>
__global__ __launch_bounds__(64) void k_spill_pass(uint32_t ntx, uint32_t nty, uint32_t all, const uint32_t *__restrict__ hk, uint32_t *w,
                                                   uint32_t *act_cur, uint32_t *act_next, uint32_t *__restrict__ changed, uint32_t *__restrict__ runs)
{
    const uint32_t lane = threadIdx.x, tile = blockIdx.x;
    if (tile >= ntx * nty) return;
    uint32_t active = 0u;
    if (lane == 0u) { active = act_cur[tile]; act_cur[tile] = 0u; }
    active = __builtin_amdgcn_readfirstlane(active);
    if (!(active | all)) return;                               // (wave-uniform)
    if (lane == 0u) atomicAdd(runs, 1u);
    const uint32_t ty = tile / ntx, tx = tile - ty * ntx;
    const size_t base = (size_t)tile * kSpillTileWords;
    uint32_t h[kSpillTile], v[kSpillTile];
#pragma unroll
    for (uint32_t b = 0; b < kSpillTile; ++b) {
        h[b] = hk[base + b * kSpillTile + lane];
        v[b] = w[base + b * kSpillTile + lane];
    }
    uint32_t fell = 0u;
    // the halos: column 63 of the left tile, column 0 of the right one (one coalesced load each); row 63 of the tile above and row 0
    // of the tile below (lane b holds column b's element, handed to register b of lane 0 / lane 63)
    if (tx > 0u) { const uint32_t x = w[base - kSpillTileWords + 63u * kSpillTile + lane]; VF_SPILL_RELAX(h[0], v[0], x, fell); }
    if (tx + 1u < ntx) { const uint32_t x = w[base + kSpillTileWords + lane]; VF_SPILL_RELAX(h[63], v[63], x, fell); }
    uint32_t above = kSpillInf, below = kSpillInf;
    if (ty > 0u) above = w[base - (size_t)ntx * kSpillTileWords + lane * kSpillTile + 63u];
    if (ty + 1u < nty) below = w[base + (size_t)ntx * kSpillTileWords + lane * kSpillTile];
#pragma unroll
    for (uint32_t b = 0; b < kSpillTile; ++b) {
        const uint32_t xa = __builtin_amdgcn_readlane(above, b), xb = __builtin_amdgcn_readlane(below, b);
        const uint32_t x = lane == 0u ? xa : lane == 63u ? xb : kSpillInf;
        VF_SPILL_RELAX(h[b], v[b], x, fell);
    }
    bool open = true;                                          // the trip bound ended the loop: the tile is not at its fixpoint yet
    for (uint32_t trip = 0; trip < kSpillTrips; ++trip) {
        uint32_t c = 0u;
#pragma unroll
        for (uint32_t b = 1; b < kSpillTile; ++b) VF_SPILL_RELAX(h[b], v[b], v[b - 1u], c);
#pragma unroll
        for (uint32_t b = kSpillTile - 1u; b-- > 0u;) VF_SPILL_RELAX(h[b], v[b], v[b + 1u], c);
#pragma unroll
        for (uint32_t b = 0; b < kSpillTile; ++b) {            // (lane 0 / lane 63 get their own value back: no change)
            const uint32_t x = min(__shfl_up(v[b], 1u), __shfl_down(v[b], 1u));
            VF_SPILL_RELAX(h[b], v[b], x, c);
        }
        fell |= c;
        if (!__any(c != 0u)) { open = false; break; }
    }
    if (!__any(fell != 0u) && !open) return;
#pragma unroll
    for (uint32_t b = 0; b < kSpillTile; ++b) w[base + b * kSpillTile + lane] = v[b];
    if (lane == 0u) {
        *changed = 1u;
        if (tx > 0u) act_next[tile - 1u] = 1u;
        if (tx + 1u < ntx) act_next[tile + 1u] = 1u;
        if (ty > 0u) act_next[tile - ntx] = 1u;
        if (ty + 1u < nty) act_next[tile + ntx] = 1u;
        if (open) act_next[tile] = 1u;
    }
}

// A wave takes 64 consecutive vertices of one row (blockIdx.x: the tile column, blockIdx.y * 4 + wave: the row): spill decoded, sd =
// spill - h, and counts += reached | sinks << 32 (one atomic add per wave; n x n stays below 2^32: spill_field refuses anything else)
template <int UNUSED>
__global__ __launch_bounds__(256) void k_spill_out(uint32_t n, uint32_t nb, uint32_t ntx, const float *__restrict__ hblk, const uint32_t *__restrict__ w,
                                                   float *__restrict__ spill, float *__restrict__ sd, unsigned long long *__restrict__ counts)
{
    const uint32_t lane = threadIdx.x & 63u, tx = blockIdx.x, j = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (j >= n) return;                                        // (wave-uniform)
    const uint32_t i = tx * kSpillTile + lane;
    bool reached = false, sink = false;
    if (i < n) {
        const uint32_t k = w[spill_index(ntx, i, j)];
        const float sp = spill_unkey(k), d = sp - cached_height(hblk, nb, i, j);
        const size_t o = (size_t)j * n + i;
        spill[o] = sp;
        sd[o] = d;
        reached = k != kSpillInf;
        sink = d > 0.0f && isfinite(d);
    }
    const uint64_t r = __ballot(reached), k = __ballot(sink);
    if (lane == 0u && r != 0ull) atomicAdd(counts, (unsigned long long)__popcll(r) | ((unsigned long long)__popcll(k) << 32));
}

// ---- the tint pass (contract item 6) ----

struct SpillTint {
    const float *sd;            // spill - h, n x n
    const float *decode;        // 256 sRGB8 -> linear
    uint32_t shallow_rgba, deep_rgba;
    float depth_full;
};

// Pixel (px, py) with visibility id `id` and colour `rgba`: false when the pass leaves it as the frame drew it
template <bool CLIPPED>
__device__ __forceinline__ bool spill_pixel(const FrameParams &P, const SetupView &V, const SpillTint &T, const float *dec, const float *thr,
                                            uint32_t id, int32_t px, int32_t py, uint32_t &rgba)
{
    const uint32_t prim = id - 1u;
    const VisibleSite s = visible_site<CLIPPED>(P, V, prim);
    const float w0 = T.sd[site_vertex(P, s, 0)], w1 = T.sd[site_vertex(P, s, 1)], w2 = T.sd[site_vertex(P, s, 2)];
    if (!(isfinite(w0) && isfinite(w1) && isfinite(w2))) return false;
    if (w0 == 0.0f && w1 == 0.0f && w2 == 0.0f) return false;  // no sink here: the usual case
    const VisiblePoint<CLIPPED> p = visible_point<CLIPPED>(P, V, s, prim, px, py);
    const float d = point_scalar(P, p, px, py, w0, w1, w2);
    if (!(d > 0.0f)) return false;
    return vs_depth_tint(dec, thr, d, T.depth_full, T.shallow_rgba, T.deep_rgba, rgba);
}

// The covered pixels of a frame's colour buffer over a sink (tint_visible, vf_viewshed.h)
template <bool CLIPPED>
__global__ __launch_bounds__(256) void k_spill_tint(FrameParams P, SetupView V, const float *__restrict__ thresh, const uint32_t *__restrict__ vis,
                                                    SpillTint T, const uint32_t *__restrict__ redo, uint32_t *__restrict__ rgba)
{
    tint_visible<CLIPPED>(P, thresh, T.decode, vis, redo, rgba, [&](const float *dec, const float *thr, uint32_t id, int32_t px, int32_t py, uint32_t &c) {
        return spill_pixel<CLIPPED>(P, V, T, dec, thr, id, px, py, c);
    });
}

} // namespace vf

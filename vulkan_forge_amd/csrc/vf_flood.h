// vf_flood.h -- flood analysis: what lies under water at a level, and which of that ground the water can reach.
//
//   the masks            a wave64 holds a 64 x 64 tile of vertices as one 64-bit row mask per lane.  `wet` (h is finite and below the
//                        level) and `fl` (flooded) are tile-major: word (ty ntx + tx) 64 + r is row r of tile (tx, ty), bit b of it the
//                        vertex (64 tx + b, 64 ty + r); ntx = ceil(n / 64); bits and rows beyond the grid are 0 in `wet`, so in `fl`
//   k_flood_wet          the masks' words from the height cache by a wave ballot, and wd = level - h per vertex
//   k_flood_seed         the sources' bits into `fl` where `wet` has them (the feature's one atomic: an OR on a 32-bit half)
//   k_flood_pass         one wave per tile: the halo bits of the four neighbours enter, then the tile runs to its own fixpoint -- a
//                        Kogge-Stone occluded fill along the rows, one step across them by lane shuffles, until no lane changes.  The
//                        host repeats the launch until one changes nothing (SeededFill::fixpoint, vf_hip.hip: the spill's loop too)
//   k_flood_depth        depth = flooded ? wd : 0 per vertex, and the two counts
//   k_flood_tint         blends a shallow and a deep colour over the covered pixels of a frame from its stored visibility, flat: the
//                        tint body (tint_visible) and the blend (vs_depth_tint) are vf_viewshed.h's, shared with k_spill_tint
//
// Launched only for a handle that asked for a flood or for the field: the frame path is not touched.  Every device loop has a fixed
// trip bound, no workgroup waits for another, and bits of `fl` are only ever set: a wave that reads a neighbour's words while that
// neighbour stores them sees a subset of the truth and the next launch sees all of it, so every order of evaluation ends in the same
// least fixpoint.  64-bit shifts take constant amounts only (vf_device.h: the MI355X fault of a shift by the last allocated
// register); a bit is tested or set through the 32-bit half that holds it.  All kernels are templates: the library's non-template
// kernels keep their places.
#pragma once
#include "vf_viewshed.h"

namespace vf {

constexpr uint32_t kFloodTile = 64;                            // vertices per side of a tile: the bits of a word, the lanes of a wave
constexpr uint32_t kFloodTrips = 4096;                         // a tile has 4096 bits and every trip of k_flood_pass but its last sets one

// where vertex (i, j) lives in the masks: the 32-bit half (of the words seen as pairs, low half first) and the bit in it
__device__ __forceinline__ size_t flood_half(uint32_t ntx, uint32_t i, uint32_t j)
{
    const size_t word = ((size_t)(j >> 6) * ntx + (i >> 6)) * kFloodTile + (j & 63u);
    return word * 2u + ((i >> 5) & 1u);
}
__device__ __forceinline__ bool flood_bit(const uint32_t *__restrict__ mask, uint32_t ntx, uint32_t i, uint32_t j)
{
    return (mask[flood_half(ntx, i, j)] >> (i & 31u)) & 1u;
}

// A wave takes 64 consecutive vertices of one row (blockIdx.x: the tile column, blockIdx.y * 4 + wave: the row, up to the last row of
// the last tile): the row's word of `wet` by a ballot, `fl` = the same word (EVERYWHERE: the plain bathtub) or 0, and wd.
template <bool EVERYWHERE>
__global__ __launch_bounds__(256) void k_flood_wet(uint32_t n, uint32_t nb, uint32_t ntx, uint32_t rows, float level, const float *__restrict__ hblk,
                                                   uint64_t *__restrict__ wet, uint64_t *__restrict__ fl, float *__restrict__ wd)
{
    const uint32_t lane = threadIdx.x & 63u, tx = blockIdx.x, j = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (j >= rows) return;                                     // (wave-uniform)
    const uint32_t i = tx * kFloodTile + lane;
    const bool inside = i < n && j < n;
    bool w = false;
    if (inside) {
        const float h = cached_height(hblk, nb, i, j);
        w = isfinite(h) && h < level;
        wd[(size_t)j * n + i] = level - h;
    }
    const uint64_t word = __ballot(w);
    if (lane == 0u) {
        const size_t o = ((size_t)(j >> 6) * ntx + tx) * kFloodTile + (j & 63u);
        wet[o] = word;
        fl[o] = EVERYWHERE ? word : 0ull;
    }
}

// One thread per source: vertex (ij[2 k], ij[2 k + 1]) of a seed list (EDGES = false, count of them), or the k-th of the 4 n border
// vertices (EDGES = true; a corner comes twice).  A source that is not wet-able is none.
template <bool EDGES>
__global__ __launch_bounds__(256) void k_flood_seed(uint32_t n, uint32_t ntx, const uint32_t *__restrict__ ij, uint32_t count,
                                                    const uint32_t *__restrict__ wet, uint32_t *__restrict__ fl)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= count) return;
    uint32_t i, j;
    if constexpr (EDGES) {
        const uint32_t side = k / n, a = k - side * n;
        i = side == 2u ? 0u : side == 3u ? n - 1u : a;
        j = side == 0u ? 0u : side == 1u ? n - 1u : a;
    } else {
        i = ij[2u * k]; j = ij[2u * k + 1u];
    }
    if (i >= n || j >= n) return;
    const size_t o = flood_half(ntx, i, j);
    const uint32_t m = 1u << (i & 31u);
    if (wet[o] & m) atomicOr(&fl[o], m);
}

// occluded fills along a row: every bit of w that a run of w bits joins to a bit of g, towards the higher / the lower bits
__device__ __forceinline__ uint64_t flood_fill_up(uint64_t g, uint64_t p)
{
    g |= p & (g << 1); p &= p << 1;
    g |= p & (g << 2); p &= p << 2;
    g |= p & (g << 4); p &= p << 4;
    g |= p & (g << 8); p &= p << 8;
    g |= p & (g << 16); p &= p << 16;
    g |= p & (g << 32);
    return g;
}
__device__ __forceinline__ uint64_t flood_fill_down(uint64_t g, uint64_t p)
{
    g |= p & (g >> 1); p &= p >> 1;
    g |= p & (g >> 2); p &= p >> 2;
    g |= p & (g >> 4); p &= p >> 4;
    g |= p & (g >> 8); p &= p >> 8;
    g |= p & (g >> 16); p &= p >> 16;
    g |= p & (g >> 32);
    return g;
}

// the words of the rows above and below this lane's (0 beyond the tile), by shuffles of the two halves
__device__ __forceinline__ uint64_t flood_rows_beside(uint64_t f, uint32_t lane)
{
    const uint32_t lo = (uint32_t)f, hi = (uint32_t)(f >> 32);
    const uint32_t ulo = __shfl_up(lo, 1u), uhi = __shfl_up(hi, 1u), dlo = __shfl_down(lo, 1u), dhi = __shfl_down(hi, 1u);
    const uint64_t up = lane ? ((uint64_t)uhi << 32) | ulo : 0ull, down = lane < 63u ? ((uint64_t)dhi << 32) | dlo : 0ull;
    return up | down;
}

// One wave per tile (blockIdx.x = ty ntx + tx), lane = row.  *changed = 1 when the tile's `fl` grew.  `fl` is read and written in the
// same launch by different waves on purpose (see the head of the file): no __restrict__ on it.
template <int UNUSED>
__global__ __launch_bounds__(64) void k_flood_pass(uint32_t ntx, uint32_t nty, const uint64_t *__restrict__ wet, uint64_t *fl, uint32_t *__restrict__ changed)
{
    const uint32_t lane = threadIdx.x, tile = blockIdx.x;
    if (tile >= ntx * nty) return;
    const uint32_t ty = tile / ntx, tx = tile - ty * ntx;
    const size_t base = (size_t)tile * kFloodTile;
    const uint64_t w = wet[base + lane], f0 = fl[base + lane];
    if (!__any(w != 0ull) || !__any(f0 != w)) return;          // nothing to wet, or nothing left to wet
    uint64_t halo = 0ull;
    if (tx > 0u) halo |= fl[base - kFloodTile + lane] >> 63;
    if (tx + 1u < ntx) halo |= fl[base + kFloodTile + lane] << 63;
    if (ty > 0u) {                                             // (wave-uniform loads)
        const uint64_t above = fl[base - (size_t)ntx * kFloodTile + 63u];
        if (lane == 0u) halo |= above;
    }
    if (ty + 1u < nty) {
        const uint64_t below = fl[base + (size_t)ntx * kFloodTile];
        if (lane == 63u) halo |= below;
    }
    uint64_t f = f0 | (w & halo);
    for (uint32_t trip = 0; trip < kFloodTrips; ++trip) {
        const uint64_t before = f;
        f = flood_fill_up(f, w);
        f = flood_fill_down(f, w);
        f |= w & flood_rows_beside(f, lane);
        if (!__any(f != before)) break;
    }
    if (!__any(f != f0)) return;
    fl[base + lane] = f;
    if (lane == 0u) *changed = 1u;
}

// A wave takes 64 consecutive vertices of one row, as k_flood_wet does: depth = flooded ? wd : 0, and counts += flooded | wet-able << 32
// (one atomic add per wave; n x n stays below 2^32: the grid is at most 8192, and flood_field refuses anything else)
template <int UNUSED>
__global__ __launch_bounds__(256) void k_flood_depth(uint32_t n, uint32_t ntx, const uint64_t *__restrict__ wet, const uint64_t *__restrict__ fl,
                                                     const float *__restrict__ wd, float *__restrict__ depth, unsigned long long *__restrict__ counts)
{
    const uint32_t lane = threadIdx.x & 63u, tx = blockIdx.x, j = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (j >= n) return;                                        // (wave-uniform)
    const size_t o = ((size_t)(j >> 6) * ntx + tx) * kFloodTile + (j & 63u);
    const uint64_t f = fl[o], w = wet[o];
    const uint32_t half = lane < 32u ? (uint32_t)f : (uint32_t)(f >> 32);
    const uint32_t i = tx * kFloodTile + lane;
    if (i < n) {
        const size_t v = (size_t)j * n + i;
        depth[v] = ((half >> (lane & 31u)) & 1u) ? wd[v] : 0.0f;
    }
    if (lane == 0u && w != 0ull) atomicAdd(counts, (unsigned long long)__popcll(f) | ((unsigned long long)__popcll(w) << 32));
}

// ---- the tint pass (contract item 5) ----

struct FloodTint {
    const uint32_t *fl;         // the flooded mask, as 32-bit halves
    const float *wd;            // level - h, n x n
    const float *decode;        // 256 sRGB8 -> linear
    uint32_t ntx;
    uint32_t shallow_rgba, deep_rgba;
    float depth_full;
};

// Pixel (px, py) with visibility id `id` and colour `rgba`: false when the pass leaves it as the frame drew it
template <bool CLIPPED>
__device__ __forceinline__ bool flood_pixel(const FrameParams &P, const SetupView &V, const FloodTint &T, const float *dec, const float *thr,
                                            uint32_t id, int32_t px, int32_t py, uint32_t &rgba)
{
    const uint32_t prim = id - 1u;
    const VisibleSite s = visible_site<CLIPPED>(P, V, prim);
    // vertex 0 = (i + odd, j), vertex 1 = (i, j + 1), vertex 2 = (i + 1, j + odd) (site_vertex)
    if (!(flood_bit(T.fl, T.ntx, s.i + s.odd, s.j) || flood_bit(T.fl, T.ntx, s.i, s.j + 1u) || flood_bit(T.fl, T.ntx, s.i + 1u, s.j + s.odd))) return false;
    const float w0 = T.wd[site_vertex(P, s, 0)], w1 = T.wd[site_vertex(P, s, 1)], w2 = T.wd[site_vertex(P, s, 2)];
    if (!(isfinite(w0) && isfinite(w1) && isfinite(w2))) return false;
    const VisiblePoint<CLIPPED> p = visible_point<CLIPPED>(P, V, s, prim, px, py);
    const float d = point_scalar(P, p, px, py, w0, w1, w2);
    if (!(d > 0.0f)) return false;
    return vs_depth_tint(dec, thr, d, T.depth_full, T.shallow_rgba, T.deep_rgba, rgba);
}

// The covered pixels of a frame's colour buffer under water (tint_visible, vf_viewshed.h)
template <bool CLIPPED>
__global__ __launch_bounds__(256) void k_flood_tint(FrameParams P, SetupView V, const float *__restrict__ thresh, const uint32_t *__restrict__ vis,
                                                    FloodTint T, const uint32_t *__restrict__ redo, uint32_t *__restrict__ rgba)
{
    tint_visible<CLIPPED>(P, thresh, T.decode, vis, redo, rgba, [&](const float *dec, const float *thr, uint32_t id, int32_t px, int32_t py, uint32_t &c) {
        return flood_pixel<CLIPPED>(P, V, T, dec, thr, id, px, py, c);
    });
}

} // namespace vf

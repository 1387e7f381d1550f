// vf_contour.h -- contour lines (isolines) of the rendered surface, extracted on the GPU from the displaced-height cache straight
// into overlay records (vf_terrain_add_contours).  Add time, not frame time: the records are drawn by the overlay
// passes of vf_overlay.h like those of a line layer.
//
//   k_ct_count    one wave per 8x8-cell block, one cell (two triangles) per lane: segments per block
//   k_ct_scan     one workgroup: block counts -> exclusive offsets (in place) and the total
//   k_ct_emit     the walk of k_ct_count again; a wave prefix sum gives each lane its slots behind the block's offset
//   k_ct_bounds   vf_terrain_height_bounds: min / max of the finite heights, from the per-block bounds
//
// The contract (bit for bit; tests/contour_model is its CPU statement).  Triangles are the renderer's: cell (i, j), a = (i, j),
// b = (i + 1, j), c = (i, j + 1), d = (i + 1, j + 1), even triangle (a, c, b), odd triangle (b, c, d).  A vertex is above level L
// iff h >= L; a triangle with a non-finite vertex height emits nothing; L crosses a triangle iff its vertices are not all on one
// side, and then one vertex s is alone on its side.  s above: p0 on edge s-next(s), p1 on s-prev(s); s below: the other way round
// (the triangle's vertex order).  A crossing point is formed from the edge's below vertex P to its above vertex Q:
// t = (L - hP) / (hQ - hP), x = fma(t, xQ - xP, xP), z likewise -- both triangles on an edge get the same bits.  Records: blocks
// row-major, cells row-major in a block, even before odd, levels ascending; the segment, then (round joins) a disc at p0.
#pragma once
#include "vf_device.h"
// (included by vf_overlay.h, behind its record types OvIn / kOv*)

namespace vf {

constexpr uint32_t kCtMaxLevels = 65536u;       // levels of one contour layer

struct CtGrid {
    uint32_t nm1, nb;               // cells / blocks per side
    float step, spacing;            // x_i = (-1.5 + i step) spacing, as the vertex stage forms it
    const float *hblk;              // displaced-height cache (k_height_blocks)
    const float2 *bounds;           // per block min / max (-inf / inf: a non-finite height in the block)
    const float *levels;            // ascending
    uint32_t nlevels;
};

struct CtStyle {
    float hw, lift;
    uint32_t rgba, feature, base;   // base: kOvDrape [| kOvOcclude]
    uint32_t kb_bits;               // pad[0] (bits of kb when occluding, else 0)
    uint32_t round;                 // a disc at every segment's p0
};

// first index k in [lo, hi) with lv[k] > v, hi when there is none
__device__ __forceinline__ uint32_t ct_upper(const float *__restrict__ lv, uint32_t lo, uint32_t hi, float v)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (lv[mid] <= v) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// the levels that cross a triangle: indices [lo, hi) of the sorted list, min h < L <= max h (within the block's range [k0, k1))
__device__ __forceinline__ void ct_range(const float *__restrict__ lv, uint32_t k0, uint32_t k1, float h0, float h1, float h2,
                                         uint32_t &lo, uint32_t &hi)
{
    lo = hi = k0;
    if (!(isfinite(h0) && isfinite(h1) && isfinite(h2))) return;
    lo = ct_upper(lv, k0, k1, fminf(h0, fminf(h1, h2)));
    hi = ct_upper(lv, lo, k1, fmaxf(h0, fmaxf(h1, h2)));
}

// the crossing of level L with the edge from its below vertex P to its above vertex Q
__device__ __forceinline__ void ct_cross(float L, float hP, float xP, float zP, float hQ, float xQ, float zQ, float &x, float &z)
{
    const float t = (L - hP) / (hQ - hP);
    x = fmaf(t, xQ - xP, xP);
    z = fmaf(t, zQ - zP, zP);
}

// the segment of level L in triangle (v0, v1, v2), which L crosses
__device__ __forceinline__ void ct_segment(float L, float h0, float x0, float z0, float h1, float x1, float z1, float h2, float x2, float z2,
                                           float &ax, float &az, float &bx, float &bz)
{
    const bool a0 = h0 >= L, a1 = h1 >= L, a2 = h2 >= L;
    const bool one = ((int)a0 + (int)a1 + (int)a2) == 1;               // one vertex above: it is the lone one; else the one below
    const int s = (a0 == one) ? 0 : (a1 == one) ? 1 : 2;
    // rotate: s, next(s), prev(s)
    const float hs = s == 0 ? h0 : s == 1 ? h1 : h2, xs = s == 0 ? x0 : s == 1 ? x1 : x2, zs = s == 0 ? z0 : s == 1 ? z1 : z2;
    const float hn = s == 0 ? h1 : s == 1 ? h2 : h0, xn = s == 0 ? x1 : s == 1 ? x2 : x0, zn = s == 0 ? z1 : s == 1 ? z2 : z0;
    const float hp = s == 0 ? h2 : s == 1 ? h0 : h1, xp = s == 0 ? x2 : s == 1 ? x0 : x1, zp = s == 0 ? z2 : s == 1 ? z0 : z1;
    if (one) {                                                          // s above: p0 on s-next, p1 on s-prev
        ct_cross(L, hn, xn, zn, hs, xs, zs, ax, az);
        ct_cross(L, hp, xp, zp, hs, xs, zs, bx, bz);
    } else {                                                            // s below: p0 on s-prev, p1 on s-next
        ct_cross(L, hs, xs, zs, hp, xp, zp, ax, az);
        ct_cross(L, hs, xs, zs, hn, xn, zn, bx, bz);
    }
}

// A lane's cell of its wave's block: the four vertex heights from the block's 81 staged heights, whether the cell exists, and the level
// ranges of its two triangles.  false (for the whole wave): no level lies in the block's height interval.
struct CtCell { float ha, hb, hc, hd; uint32_t i, j, e0, e1, o0, o1; };

__device__ __forceinline__ bool ct_cell(const CtGrid &G, float *s_h, CtCell &c)
{
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    const float2 bd = G.bounds[b];
    const uint32_t k0 = ct_upper(G.levels, 0u, G.nlevels, bd.x), k1 = ct_upper(G.levels, k0, G.nlevels, bd.y);
    if (k0 >= k1) return false;                                         // (wave-uniform)
    const float *src = G.hblk + (size_t)b * kBlockStride;
    s_h[lane] = src[lane];
    if (lane + 64u < (uint32_t)kBlockStride) s_h[lane + 64u] = src[lane + 64u];
    __syncthreads();
    const uint32_t li = lane & 7u, lj = lane >> 3;
    c.i = (b % G.nb) * kBlockCells + li; c.j = (b / G.nb) * kBlockCells + lj;
    c.ha = s_h[lj * 9u + li]; c.hb = s_h[lj * 9u + li + 1u]; c.hc = s_h[(lj + 1u) * 9u + li]; c.hd = s_h[(lj + 1u) * 9u + li + 1u];
    c.e0 = c.e1 = c.o0 = c.o1 = k0;
    if (c.i < G.nm1 && c.j < G.nm1) {                                   // (border blocks: cells beyond the grid hold nothing)
        ct_range(G.levels, k0, k1, c.ha, c.hc, c.hb, c.e0, c.e1);
        ct_range(G.levels, k0, k1, c.hb, c.hc, c.hd, c.o0, c.o1);
    }
    return true;
}

__global__ __launch_bounds__(64) void k_ct_count(CtGrid G, uint32_t *__restrict__ count)
{
    __shared__ float s_h[kBlockStride];
    CtCell c;
    uint32_t n = 0;
    if (ct_cell(G, s_h, c)) n = (c.e1 - c.e0) + (c.o1 - c.o0);
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if (threadIdx.x == 0) count[blockIdx.x] = n;                        // (at most 128 * kCtMaxLevels = 2^23)
}

// block counts -> exclusive offsets in place (modulo 2^32: only used when the total fits the primitive budget), total[0] = their sum
__global__ __launch_bounds__(1024) void k_ct_scan(uint32_t nblocks, uint32_t *__restrict__ cnt, unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long part[1024], carry;                   // (a chunk's sum can reach 1024 * 2^23)
    const uint32_t tid = threadIdx.x;
    if (tid == 0) carry = 0ull;
    __syncthreads();
    for (uint32_t base = 0; base < nblocks; base += 1024u) {
        const uint32_t k = base + tid;
        const uint32_t v = k < nblocks ? cnt[k] : 0u;
        part[tid] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 1024u; d <<= 1) {                     // inclusive Hillis-Steele scan
            const unsigned long long add = tid >= d ? part[tid - d] : 0ull;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        const unsigned long long c = carry;
        if (k < nblocks) cnt[k] = (uint32_t)(c + part[tid] - v);
        __syncthreads();
        if (tid == 1023u) carry = c + part[1023];
        __syncthreads();
    }
    if (tid == 0) total[0] = carry;
}

__device__ __forceinline__ void ct_store(OvIn *__restrict__ out, uint32_t idx, float ax, float az, float bx, float bz, uint32_t kind, const CtStyle &S)
{
    uint4 *q = reinterpret_cast<uint4 *>(out + idx);                   // (48-byte records in a 256-byte aligned array)
    q[0] = make_uint4(__float_as_uint(ax), __float_as_uint(S.lift), __float_as_uint(az), __float_as_uint(bx));
    q[1] = make_uint4(__float_as_uint(S.lift), __float_as_uint(bz), __float_as_uint(S.hw), kind | S.base);
    q[2] = make_uint4(S.rgba, S.feature, S.kb_bits, 0u);
}

__device__ __forceinline__ uint32_t ct_emit_tri(const CtGrid &G, const CtStyle &S, OvIn *__restrict__ out, uint32_t slot, uint32_t k0, uint32_t k1,
                                                float h0, float x0, float z0, float h1, float x1, float z1, float h2, float x2, float z2)
{
    for (uint32_t k = k0; k < k1; ++k, ++slot) {
        float ax, az, bx, bz;
        ct_segment(G.levels[k], h0, x0, z0, h1, x1, z1, h2, x2, z2, ax, az, bx, bz);
        const uint32_t idx = S.round ? 2u * slot : slot;
        ct_store(out, idx, ax, az, bx, bz, kOvSegment, S);
        if (S.round) ct_store(out, idx + 1u, ax, az, ax, az, kOvCircle, S);
    }
    return slot;
}

// offset: k_ct_scan's exclusive block offsets (segments); out: the layer's first record
__global__ __launch_bounds__(64) void k_ct_emit(CtGrid G, CtStyle S, const uint32_t *__restrict__ offset, OvIn *__restrict__ out)
{
    __shared__ float s_h[kBlockStride];
    CtCell c;
    if (!ct_cell(G, s_h, c)) return;
    const uint32_t n = (c.e1 - c.e0) + (c.o1 - c.o0);
    uint32_t incl = n;                                                  // inclusive prefix sum over the wave's lanes
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if ((int)threadIdx.x >= o) incl += up;
    }
    if (!n) return;
    uint32_t slot = offset[blockIdx.x] + incl - n;
    const float xa = (-1.5f + (float)c.i * G.step) * G.spacing, xb = (-1.5f + (float)(c.i + 1u) * G.step) * G.spacing;
    const float za = (-1.5f + (float)c.j * G.step) * G.spacing, zc = (-1.5f + (float)(c.j + 1u) * G.step) * G.spacing;
    slot = ct_emit_tri(G, S, out, slot, c.e0, c.e1, c.ha, xa, za, c.hc, xa, zc, c.hb, xb, za);     // even: (a, c, b)
    ct_emit_tri(G, S, out, slot, c.o0, c.o1, c.hb, xb, za, c.hc, xa, zc, c.hd, xb, zc);            // odd: (b, c, d)
}

// min / max of the surface's finite heights -> out[0]: the per-block bounds, and for a block that holds a non-finite height (bounds
// -inf / inf) its heights again.  One workgroup.
__global__ __launch_bounds__(1024) void k_ct_bounds(uint32_t n, uint32_t nb, const float2 *__restrict__ bounds, const float *__restrict__ hblk,
                                                    float2 *__restrict__ out)
{
    __shared__ float s_lo[16], s_hi[16];
    float lo = INFINITY, hi = -INFINITY;
    for (uint32_t b = threadIdx.x; b < nb * nb; b += 1024u) {
        const float2 bd = bounds[b];
        if (isfinite(bd.x) && isfinite(bd.y)) { lo = fminf(lo, bd.x); hi = fmaxf(hi, bd.y); continue; }
        const uint32_t i0 = (b % nb) * kBlockCells, j0 = (b / nb) * kBlockCells;
        for (uint32_t v = 0; v < (uint32_t)kBlockStride; ++v) {
            const float h = hblk[(size_t)b * kBlockStride + v];
            if (i0 + v % 9u < n && j0 + v / 9u < n && isfinite(h)) { lo = fminf(lo, h); hi = fmaxf(hi, h); }
        }
    }
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
    if ((threadIdx.x & 63u) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) { lo = fminf(lo, s_lo[w]); hi = fmaxf(hi, s_hi[w]); }
        out[0] = make_float2(lo, hi);
    }
}

} // namespace vf

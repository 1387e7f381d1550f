// vf_shadow.h -- cast sun shadows on the terrain.
//
//   the shadow field   one float per grid vertex, lit in [0, 1], from the displaced-height cache and the sun: a prefix maximum along
//                      sheared grid lines, as a decoupled scan -- k_shadow_chunk_max (the maximum of every 64-step chunk of every
//                      line), k_shadow_carry (their exclusive running maximum along each line), k_shadow_lit (the scan inside a chunk
//                      by DPP, seeded with the chunk's carry, and the horizon test)
//   the shade pass     k_shadow_shade walks the frame's stored visibility (for_each_visible, vf_visible.h) and writes again, through
//                      the exact fragment function, the pixels whose interpolated lit is below 1 (the lookup, the weights and the
//                      clipped walk are that header's)
//
// Launched only for a handle that asked for shadows or for the field: the frame path is not touched.  The arithmetic is the
// contract's, bit for bit (tests/shadow_model/shadow_model.c is its CPU statement): max is exact and associative, so the scan gives
// the sequential walk's bits however a line is cut; every term is formed from its step number alone.  All kernels are templates:
// the library's non-template kernels keep their places.
#pragma once
#include "vf_visible.h"

namespace vf {

constexpr uint32_t kShChunk = 64;                         // steps of a line per chunk = lanes of a wave
constexpr uint32_t kShLines = 64;                         // lines per workgroup
constexpr uint32_t kShPitch = kShChunk + 1;               // LDS row pitch of the z-major transposition: conflict-free both ways

// The frame of reference of one field (the host fills it: shadow_plan in vf_hip.hip).  Step k = 0, 1, ... of a line counts grid
// vertices along the major axis from the sun-side edge; line l holds the vertices whose minor index is c_lo + l - s * r(k),
// r(k) = rint((float)k * a).
struct ShadowPlan {
    uint32_t n, nb;
    uint32_t zmajor;            // the major axis: 0 = x (i), 1 = z (j)
    uint32_t from_high;         // the sun stands on the major axis' positive side: step k is major index n - 1 - k
    int32_t s;                  // +1: the sun's minor component is >= 0 (a line drifts towards lower minor indices), -1 otherwise
    int32_t c_lo;               // intercept of line 0
    uint32_t nlines, nchunks;   // n + r(n - 1) lines, ceil(n / 64) chunks
    float a;                    // |minor| / |major| component of the sun, in [0, 1]
    float d;                    // rise of the ray per step, world height units (0 when the sun is at or below the horizon)
    float exag, strength, softness, bias;
};

__device__ __forceinline__ bool sh_vertex(const ShadowPlan &S, uint32_t line, uint32_t k, uint32_t &i, uint32_t &j)
{
    if (line >= S.nlines || k >= S.n) return false;
    const int32_t minor = S.c_lo + (int32_t)line - S.s * (int32_t)rintf((float)k * S.a);
    if (minor < 0 || minor >= (int32_t)S.n) return false;
    const uint32_t major = S.from_high ? S.n - 1u - k : k;
    i = S.zmajor ? (uint32_t)minor : major;
    j = S.zmajor ? major : (uint32_t)minor;
    return true;
}

// y = h * exag of step k of a line; NaN where the line has no vertex (a non-finite y occludes nothing and is lit)
__device__ __forceinline__ float sh_height(const ShadowPlan &S, const float *__restrict__ hblk, uint32_t line, uint32_t k)
{
    uint32_t i, j;
    if (!sh_vertex(S, line, k, i, j)) return __builtin_nanf("");
    return cached_height(hblk, S.nb, i, j) * S.exag;
}

__device__ __forceinline__ float sh_term(const ShadowPlan &S, float y, uint32_t k) { return isfinite(y) ? y + (float)k * S.d : -INFINITY; }

// lit of step k: y its height, M the maximum of the terms of the steps before it (-inf: none)
__device__ __forceinline__ float sh_lit(const ShadowPlan &S, float y, float M, uint32_t k)
{
    if (!isfinite(y)) return 1.0f;
    const float e = (M - (float)k * S.d) - y;
    const float c = fminf(fmaxf((e - S.bias) / S.softness, 0.0f), 1.0f);
    return 1.0f - S.strength * c;
}

// Chunk (blockIdx.x) of 64 lines (blockIdx.y): the maximum of each line's 64 terms -> cmax[chunk][line].
// ZMAJOR = false: memory runs along the steps -- lane = step, a wave reduces one line at a time.
// ZMAJOR = true: memory runs across the lines -- lane = line, each wave walks a quarter of the steps, the quarters meet in LDS.
template <bool ZMAJOR>
__global__ __launch_bounds__(256) void k_shadow_chunk_max(ShadowPlan S, const float *__restrict__ hblk, float *__restrict__ cmax)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t k0 = blockIdx.x * kShChunk, l0 = blockIdx.y * kShLines;
    if constexpr (ZMAJOR) {
        __shared__ float part[4][kShLines];
        float m = -INFINITY;
        for (uint32_t kk = wave; kk < kShChunk; kk += 4u) m = fmaxf(m, sh_term(S, sh_height(S, hblk, l0 + lane, k0 + kk), k0 + kk));
        part[wave][lane] = m;
        __syncthreads();
        if (wave == 0u && l0 + lane < S.nlines)
            cmax[(size_t)blockIdx.x * S.nlines + l0 + lane] = fmaxf(fmaxf(part[0][lane], part[1][lane]), fmaxf(part[2][lane], part[3][lane]));
    } else {
        for (uint32_t g = wave; g < kShLines; g += 4u) {
            const uint32_t line = l0 + g;
            if (line >= S.nlines) break;                       // (wave-uniform)
            float m = sh_term(S, sh_height(S, hblk, line, k0 + lane), k0 + lane);
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            if (lane == 0u) cmax[(size_t)blockIdx.x * S.nlines + line] = m;
        }
    }
}

// per line: the chunk maxima -> the maximum of the chunks before each (in place), one thread per line
template <int UNUSED>
__global__ __launch_bounds__(256) void k_shadow_carry(uint32_t nlines, uint32_t nchunks, float *__restrict__ cmax)
{
    const uint32_t line = blockIdx.x * 256u + threadIdx.x;
    if (line >= nlines) return;
    float run = -INFINITY;
    for (uint32_t c = 0; c < nchunks; ++c) {
        const size_t o = (size_t)c * nlines + line;
        const float m = cmax[o];
        cmax[o] = run;
        run = fmaxf(run, m);
    }
}

// float <-> uint32 in the same order (every float but NaN; 0 lies below them all: the identity of the DPP ladder's unsigned max)
__device__ __forceinline__ uint32_t sh_order(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float sh_unorder(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// lane = step k0 + lane of one line: its lit from its height y and the line's carry into the chunk
__device__ __forceinline__ float sh_scan_lit(const ShadowPlan &S, float y, float carry, uint32_t k)
{
    const uint32_t inc = wave_scan_max(sh_order(sh_term(S, y, k)));            // terms of the chunk's steps up to and including this one
    const uint32_t before = __shfl_up(inc, 1u);                                // ... up to the one before
    const float M = (threadIdx.x & 63u) ? fmaxf(sh_unorder(before), carry) : carry;
    return sh_lit(S, y, M, k);
}

template <bool ZMAJOR>
__global__ __launch_bounds__(256) void k_shadow_lit(ShadowPlan S, const float *__restrict__ hblk, const float *__restrict__ carry,
                                                    float *__restrict__ lit)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t k0 = blockIdx.x * kShChunk, l0 = blockIdx.y * kShLines;
    if constexpr (ZMAJOR) {
        // rows of the grid are contiguous across the lines: heights come in and lit goes out with lane = line, the scan runs with
        // lane = step, and the 64 x 64 tile changes hands in LDS
        __shared__ float tile[kShLines * kShPitch];
        for (uint32_t kk = wave; kk < kShChunk; kk += 4u) tile[lane * kShPitch + kk] = sh_height(S, hblk, l0 + lane, k0 + kk);
        __syncthreads();
        for (uint32_t g = wave; g < kShLines; g += 4u) {
            const uint32_t line = l0 + g;
            const float c = line < S.nlines ? carry[(size_t)blockIdx.x * S.nlines + line] : -INFINITY;
            tile[g * kShPitch + lane] = sh_scan_lit(S, tile[g * kShPitch + lane], c, k0 + lane);
        }
        __syncthreads();
        for (uint32_t kk = wave; kk < kShChunk; kk += 4u) {
            uint32_t i, j;
            if (sh_vertex(S, l0 + lane, k0 + kk, i, j)) lit[(size_t)j * S.n + i] = tile[lane * kShPitch + kk];
        }
    } else {
        for (uint32_t g = wave; g < kShLines; g += 4u) {
            const uint32_t line = l0 + g;
            if (line >= S.nlines) break;                       // (wave-uniform)
            const float v = sh_scan_lit(S, sh_height(S, hblk, line, k0 + lane), carry[(size_t)blockIdx.x * S.nlines + line], k0 + lane);
            uint32_t i, j;
            if (sh_vertex(S, line, k0 + lane, i, j)) lit[(size_t)j * S.n + i] = v;
        }
    }
}

// a sun without a horizontal component (or none at all): every vertex is lit
template <int UNUSED>
__global__ __launch_bounds__(256) void k_shadow_fill(size_t count, float *__restrict__ lit)
{
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k < count) lit[k] = 1.0f;
}

// ---- the shade pass ---------------------------------------------------------------------------------------------------------

// Pixel (px, py) with visibility id `id`: its interpolated lit; when that is below 1, its colour again with lambert * lit.
// A primitive whose three vertex values are all 1 is lit without interpolation (x * (1 / x) need not round to 1).
// AMBIENT (k_ambient_shade of vf_ambient.h): amb = 1 - strength (1 - sky) per vertex is interpolated by the same rule
// and the pixel is written again when lit or amb is below 1, with shade * amb; `lit` may be NULL then (no cast shadows: lit = 1).
template <bool CLIPPED, bool AMBIENT>
__device__ __forceinline__ bool sh_pixel(const FrameParams &P, const SetupView &V, const ShadeTables &T, const float *__restrict__ lit,
                                         const float *__restrict__ sky, float amb_strength, uint32_t id, int32_t px, int32_t py, uint32_t &rgba)
{
    const uint32_t prim = id - 1u;
    const VisibleSite s = visible_site<CLIPPED>(P, V, prim);
    const uint32_t i = s.i, j = s.j, odd = s.odd;
    // vertex 0 = (i + odd, j), vertex 1 = (i, j + 1), vertex 2 = (i + 1, j + odd)
    const bool have_lit = !AMBIENT || lit != nullptr;
    const float l0 = have_lit ? lit[(size_t)j * P.n + i + odd] : 1.0f, l1 = have_lit ? lit[(size_t)(j + 1u) * P.n + i] : 1.0f, l2 = have_lit ? lit[(size_t)(j + odd) * P.n + i + 1u] : 1.0f;
    float a0 = 1.0f, a1 = 1.0f, a2 = 1.0f;
    if constexpr (AMBIENT) {
        a0 = 1.0f - amb_strength * (1.0f - sky[(size_t)j * P.n + i + odd]);
        a1 = 1.0f - amb_strength * (1.0f - sky[(size_t)(j + 1u) * P.n + i]);
        a2 = 1.0f - amb_strength * (1.0f - sky[(size_t)(j + odd) * P.n + i + 1u]);
    }
    const bool plain_l = l0 == 1.0f && l1 == 1.0f && l2 == 1.0f, plain_a = a0 == 1.0f && a1 == 1.0f && a2 == 1.0f;
    if (plain_l && plain_a) return false;
    float attr[3] = { 0.0f, 0.0f, 0.0f }, v = 1.0f, w = 1.0f;
    if constexpr (CLIPPED) {
        if (s.generic) {
            GVert g[3];
            load_prim(P, V.hblk, prim, g[0], g[1], g[2]);
            (void)clipped_weights(g, P.hw, P.hh, P.W, P.H, px, py, attr);
            // lit rides through the clipper in the place of the height varying: the same crossings, the same piece
            float la[3];
            if (!AMBIENT || !plain_l) {
                g[0].a[0] = l0; g[1].a[0] = l1; g[2].a[0] = l2;
                (void)clipped_weights(g, P.hw, P.hh, P.W, P.H, px, py, la);
                v = la[0];
            }
            if constexpr (AMBIENT) {
                if (!plain_a) {
                    g[0].a[0] = a0; g[1].a[0] = a1; g[2].a[0] = a2;
                    (void)clipped_weights(g, P.hw, P.hh, P.W, P.H, px, py, la);
                    w = la[0];
                }
            }
        }
    }
    if (!s.generic) {
        const VertexRec r0 = V.vtx[s.r0], r1 = V.vtx[s.r1], r2 = V.vtx[s.r2];
        float q0, q1, q2;
        record_weights(r0, r1, r2, px, py, q0, q1, q2);
        const float rQ = 1.0f / ((q0 + q1) + q2);
        if (!AMBIENT || !plain_l) v = fmaf(q2, l2, fmaf(q1, l1, q0 * l0)) * rQ;
        if constexpr (AMBIENT) { if (!plain_a) w = fmaf(q2, a2, fmaf(q1, a1, q0 * a0)) * rQ; }
        if (!(v < 1.0f) && !(AMBIENT && w < 1.0f)) return false;
        const float x0 = grid_coord(P, i + odd), x1 = grid_coord(P, i), x2 = grid_coord(P, i + 1u);
        const float z0 = grid_coord(P, j), z1 = grid_coord(P, j + 1u), z2 = grid_coord(P, j + odd);
        attr[0] = fmaf(q2, r2.h, fmaf(q1, r1.h, q0 * r0.h)) * rQ;
        attr[1] = fmaf(q2, x2, fmaf(q1, x1, q0 * x0)) * rQ;
        attr[2] = fmaf(q2, z2, fmaf(q1, z1, q0 * z0)) * rQ;
    }
    if (!(v < 1.0f) && !(AMBIENT && w < 1.0f)) return false;
    // (an interpolated value an ulp above 1 shades as 1; without AMBIENT v is below 1 here)
    rgba = AMBIENT ? fragment_shader_lit(P, T, attr, fminf(v, 1.0f), fminf(w, 1.0f)) : fragment_shader_lit(P, T, attr, v, 1.0f);
    return true;
}

// The frame's visibility (H, W) -> the shadowed pixels of its colour buffer, in the walk of for_each_visible (vf_visible.h).  `redo`
// is the frame's count of work items that met a clipped or oversized primitive: both instantiations are launched behind a frame and
// the one the frame does not call for leaves at once (no host round trip between the frame and its shadows).
template <bool CLIPPED>
__global__ __launch_bounds__(256) void k_shadow_shade(FrameParams P, SetupView V, const float *__restrict__ lut_linear, const float *__restrict__ thresh,
                                                      const uint32_t *__restrict__ vis, const float *__restrict__ lit, const uint32_t *__restrict__ redo,
                                                      uint32_t *__restrict__ rgba)
{
    if ((*redo != 0u) != CLIPPED) return;
    __shared__ __attribute__((aligned(16))) float s_lut[kLutFloats];
    __shared__ float s_thr[256];
    for (int k = threadIdx.x; k < kLutFloats; k += 256) s_lut[k] = lut_linear[k];
    s_thr[threadIdx.x] = thresh[threadIdx.x];
    __syncthreads();
    const ShadeTables T = { s_lut, s_thr };
    for_each_visible(P, vis, [&](uint32_t id, uint32_t px, uint32_t py) {
        uint32_t c;
        if (id != 0u && sh_pixel<CLIPPED, false>(P, V, T, lit, nullptr, 0.0f, id, (int32_t)px, (int32_t)py, c)) rgba[(size_t)py * P.W + px] = c;
    });
}

} // namespace vf

// vf_shadow.h -- cast sun shadows on the terrain.
//
//   the shadow field   one float per grid vertex, lit in [0, 1], from the displaced-height cache and the sun: a prefix maximum along
//                      sheared grid lines, as a decoupled scan -- k_shadow_chunk_max (the maximum of every 64-step chunk of every
//                      line), k_shadow_carry (their exclusive running maximum along each line), k_shadow_lit (the scan inside a chunk
//                      by DPP, seeded with the chunk's carry, and the horizon test)
//   the shade pass     k_relight<., kShadow> (vf_relight.h) writes again, through the exact fragment function, the
//                      pixels whose interpolated lit is below 1
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

// ---- the three stages of the scan, stated once ----
// Their bodies serve the single field's kernels below and the batched ones of vf_sun_exposure.h, which wrap them: a wrapper finds its
// plan, passes the base of *that plan's* carries (of this chunk, where a stage works on one) and, for the last stage, a sink that
// takes every value.  S comes by reference: a by-value kernel argument or a record in device memory.

// Chunk (blockIdx.x) of 64 lines (blockIdx.y): the maximum of each line's 64 terms -> out[line], out = cmax[chunk].
// ZMAJOR = false: memory runs along the steps -- lane = step, a wave reduces one line at a time.
// ZMAJOR = true: memory runs across the lines -- lane = line, each wave walks a quarter of the steps, the quarters meet in LDS.
template <bool ZMAJOR>
__device__ __forceinline__ void sh_stage_chunk_max(const ShadowPlan &S, const float *__restrict__ hblk, float *__restrict__ out)
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
            out[l0 + lane] = fmaxf(fmaxf(part[0][lane], part[1][lane]), fmaxf(part[2][lane], part[3][lane]));
    } else {
        for (uint32_t g = wave; g < kShLines; g += 4u) {
            const uint32_t line = l0 + g;
            if (line >= S.nlines) break;                       // (wave-uniform)
            float m = sh_term(S, sh_height(S, hblk, line, k0 + lane), k0 + lane);
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            if (lane == 0u) out[line] = m;
        }
    }
}

template <bool ZMAJOR>
__global__ __launch_bounds__(256) void k_shadow_chunk_max(ShadowPlan S, const float *__restrict__ hblk, float *__restrict__ cmax)
{
    sh_stage_chunk_max<ZMAJOR>(S, hblk, cmax + (size_t)blockIdx.x * S.nlines);
}

// per line: the chunk maxima -> the maximum of the chunks before each (in place, c = the plan's cmax), one thread per line.  Of the
// plan this stage needs two numbers, and k_shadow_carry is handed no more than them: they come as they are.
__device__ __forceinline__ void sh_stage_carry(uint32_t nlines, uint32_t nchunks, float *__restrict__ c)
{
    const uint32_t line = blockIdx.x * 256u + threadIdx.x;
    if (line >= nlines) return;
    float run = -INFINITY;
    for (uint32_t k = 0; k < nchunks; ++k) {
        const size_t o = (size_t)k * nlines + line;
        const float m = c[o];
        c[o] = run;
        run = fmaxf(run, m);
    }
}

template <int UNUSED>
__global__ __launch_bounds__(256) void k_shadow_carry(uint32_t nlines, uint32_t nchunks, float *__restrict__ cmax)
{
    sh_stage_carry(nlines, nchunks, cmax);
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

// The scan inside chunk (blockIdx.x) of 64 lines (blockIdx.y), seeded with in[line], in = carry[chunk]: sink(line, k, lit) for every
// step, those without a vertex among them (the sink asks sh_vertex)
template <bool ZMAJOR, class Sink>
__device__ __forceinline__ void sh_stage_lit(const ShadowPlan &S, const float *__restrict__ hblk, const float *__restrict__ in, Sink sink)
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
            const float c = line < S.nlines ? in[line] : -INFINITY;
            tile[g * kShPitch + lane] = sh_scan_lit(S, tile[g * kShPitch + lane], c, k0 + lane);
        }
        __syncthreads();
        for (uint32_t kk = wave; kk < kShChunk; kk += 4u) sink(l0 + lane, k0 + kk, tile[lane * kShPitch + kk]);
    } else {
        for (uint32_t g = wave; g < kShLines; g += 4u) {
            const uint32_t line = l0 + g;
            if (line >= S.nlines) break;                       // (wave-uniform)
            sink(line, k0 + lane, sh_scan_lit(S, sh_height(S, hblk, line, k0 + lane), in[line], k0 + lane));
        }
    }
}

template <bool ZMAJOR>
__global__ __launch_bounds__(256) void k_shadow_lit(ShadowPlan S, const float *__restrict__ hblk, const float *__restrict__ carry,
                                                    float *__restrict__ lit)
{
    sh_stage_lit<ZMAJOR>(S, hblk, carry + (size_t)blockIdx.x * S.nlines, [&](uint32_t line, uint32_t k, float v) {
        uint32_t i, j;
        if (sh_vertex(S, line, k, i, j)) lit[(size_t)j * S.n + i] = v;
    });
}

// a sun without a horizontal component (or none at all): every vertex is lit
template <int UNUSED>
__global__ __launch_bounds__(256) void k_shadow_fill(size_t count, float *__restrict__ lit)
{
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k < count) lit[k] = 1.0f;
}

} // namespace vf

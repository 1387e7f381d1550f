// vf_ambient.h -- ambient occlusion from a sky-view scan of the height field.
//
//   the sky-view field  one float per grid vertex, sky in [0, 1] (1 = open sky), from the displaced-height cache and D horizontal
//                       directions: k_ambient_dir, one launch per direction over the sheared lines of the shadow scan (ShadowPlan,
//                       sh_vertex), forms every vertex's horizon slope over its R predecessors on its line and adds the occlusion
//                       to the field; the last launch turns the sum into sky
//   the shade pass      k_relight<., kAmbient> (vf_relight.h): one pass serves cast shadows and ambient occlusion
//                       together
//
// Launched only for a handle that asked for ambient occlusion or for the field.  The arithmetic is the contract's, bit for bit
// (tests/ambient_model/ambient_model.c is its CPU statement): the horizon is a maximum, exact in any order, of terms formed from the
// two heights and the distance in steps alone.  All kernels are templates.
#pragma once
#include "vf_shadow.h"

namespace vf {

constexpr uint32_t kAmMaxReach = 1024;                                     // steps a vertex looks back at most (VF_AMBIENT_REACH_MAX cells)
constexpr uint32_t kAmTable = kShChunk * (kAmMaxReach / kShChunk + 2u);    // inverse distances of m = -64 ... 64 ceil(R / 64) + 63

// One direction of a field (the host fills it: ambient_plan in vf_hip.hip).  S is the frame of reference of the direction's lines
// (its d, strength, softness and bias are not used); a vertex at step k looks towards the steps k - m, m = 1 ... R.
struct AmbientPlan {
    ShadowPlan S;
    uint32_t R;                 // max(1, floor(reach / g)), g = sqrt(a^2 + 1) the length of a step in cells
    uint32_t first, last;       // the first direction stores its occlusion, the others add theirs; the last one stores sky
    float ell;                  // the length of a step, world units
    float count;                // (float)D
};

// y of step k of a line; -inf where the line has no vertex or the height is not finite (neither takes part in a horizon)
__device__ __forceinline__ float am_height(const ShadowPlan &S, const float *__restrict__ hblk, uint32_t line, uint32_t k)
{
    const float y = sh_height(S, hblk, line, k);
    return isfinite(y) ? y : -INFINITY;
}

// the occlusion of one direction at a vertex joins the field (every vertex lies on one line of a direction: no other thread of the
// launch touches it, and the launches follow each other on one stream -- the sum runs in the order of the directions)
__device__ __forceinline__ void am_store(const AmbientPlan &A, float *__restrict__ sky, size_t o, float y, float T)
{
    const float occ = y > -INFINITY ? 1.0f - 1.0f / (1.0f + T * T) : 0.0f;
    const float acc = A.first ? occ : sky[o] + occ;
    sky[o] = A.last ? fmaxf(1.0f - acc / A.count, 0.0f) : acc;
}

// Chunk (blockIdx.x) of 64 lines (blockIdx.y), 64 x 64 vertices: the chunk's own tile of heights and the ceil(R / 64) tiles before it
// on the lines pass through LDS one after the other, as tile[line][step] (pitch 65: conflict-free whichever way it is filled;
// ZMAJOR = false fills it with lane = step, ZMAJOR = true with lane = line, as memory runs).  A wave then holds one line of the tile
// in a register, lane = step, takes step j of it from lane j as a scalar and meets it with the vertex's own height and 1 / (m ell)
// from a table in LDS, m = the distance of the lane's vertex to step j; the table holds 0 where m is not in 1 ... R (a product of
// +-0 or NaN leaves the maximum, which starts at 0, as it is).  Each thread carries 16 vertices: lines wave, wave + 4, ...
template <bool ZMAJOR>
__global__ __launch_bounds__(256) void k_ambient_dir(AmbientPlan A, const float *__restrict__ hblk, float *__restrict__ sky)
{
    const ShadowPlan &S = A.S;
    __shared__ float tile[kShLines * kShPitch];
    __shared__ float tab[kAmTable];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x, k0 = c * kShChunk, l0 = blockIdx.y * kShLines;
    const uint32_t Q = (A.R + kShChunk - 1u) / kShChunk;
    for (uint32_t e = threadIdx.x; e < kShChunk * (Q + 2u) && e < kAmTable; e += 256u) {
        const int32_t m = (int32_t)e - (int32_t)kShChunk;
        tab[e] = (m >= 1 && m <= (int32_t)A.R) ? 1.0f / ((float)m * A.ell) : 0.0f;
    }
    float T[kShLines / 4u], y[kShLines / 4u];
#pragma unroll
    for (uint32_t gi = 0; gi < kShLines / 4u; ++gi) { T[gi] = 0.0f; y[gi] = -INFINITY; }
    for (uint32_t q = 0; q <= Q && q <= c; ++q) {
        const uint32_t kt = (c - q) * kShChunk;
        if (q) __syncthreads();
        if constexpr (ZMAJOR) {
            for (uint32_t kk = wave; kk < kShChunk; kk += 4u) tile[lane * kShPitch + kk] = am_height(S, hblk, l0 + lane, kt + kk);
        } else {
            for (uint32_t g = wave; g < kShLines; g += 4u) tile[g * kShPitch + lane] = am_height(S, hblk, l0 + g, kt + lane);
        }
        __syncthreads();
        // the steps j of this tile that some lane reaches: 1 <= 64 q + lane - j <= R
        const uint32_t jlo = q * kShChunk > A.R ? q * kShChunk - A.R : 0u, jhi = q ? kShChunk - 1u : kShChunk - 2u;
        const float *inv = tab + kShChunk + q * kShChunk + lane;               // inv[-j]: 1 / (m ell), m = 64 q + lane - j
#pragma unroll
        for (uint32_t gi = 0; gi < kShLines / 4u; ++gi) {
            const float row = tile[(wave + 4u * gi) * kShPitch + lane];
            if (q == 0u) y[gi] = row;
            float t = T[gi];
            const float own = y[gi];
            for (uint32_t j = jlo; j <= jhi; ++j) {
                const float yj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(row), (int)j));
                t = fmaxf(t, (yj - own) * inv[-(int32_t)j]);
            }
            T[gi] = t;
        }
    }
    if constexpr (ZMAJOR) {
        // the horizons change hands in LDS: out with lane = line, as the field's rows run
        __syncthreads();
#pragma unroll
        for (uint32_t gi = 0; gi < kShLines / 4u; ++gi) tile[(wave + 4u * gi) * kShPitch + lane] = y[gi] > -INFINITY ? T[gi] : -INFINITY;
        __syncthreads();
        for (uint32_t kk = wave; kk < kShChunk; kk += 4u) {
            uint32_t i, j;
            if (!sh_vertex(S, l0 + lane, k0 + kk, i, j)) continue;
            const float t = tile[lane * kShPitch + kk];
            am_store(A, sky, (size_t)j * S.n + i, t, t > -INFINITY ? t : 0.0f);
        }
    } else {
#pragma unroll
        for (uint32_t gi = 0; gi < kShLines / 4u; ++gi) {
            uint32_t i, j;
            if (sh_vertex(S, l0 + wave + 4u * gi, k0 + lane, i, j)) am_store(A, sky, (size_t)j * S.n + i, y[gi], T[gi]);
        }
    }
}

} // namespace vf

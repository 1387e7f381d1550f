// vf_cumulative_viewshed.h -- cumulative viewsheds: how many of N observers see each vertex.
//
// The scan of vf_viewshed.h over a batch of observers at once: the same three stages, with the observer's index in blockIdx.z and its
// ViewshedPlan read from a device array, so that a batch costs five launches however many observers it holds.  Every observer has
// its own carries (cmax[observer][quadrant][chunk][line]).  The last stage does not store seen: it adds q = rint(seen * 65536) to a
// field of 32-bit sums with a relaxed device-scope atomic.  One observer has one writer per vertex (vs_owner), so the atomics meet only
// between observers, and integer addition commutes: the sums do not depend on batching or on the order of arrival.
//
// The range limit is in the plans the host fills: steps[] and nchunks are cut at ceil(Rc), so a line has no vertex beyond it
// (vs_vertex), chunks beyond it are neither launched nor walked, and the in-range vertices keep the bits of the full scan -- the
// terms before a step do not depend on what comes after it.  RR = Rc * Rc decides which of the walked vertices count.
// All kernels are templates: the library's non-template kernels keep their places.
#pragma once
#include "vf_viewshed.h"

namespace vf {

// k_viewshed_chunk_max for observer blockIdx.z / 2, quadrant 2 ZMAJOR + (blockIdx.z & 1)
template <bool ZMAJOR>
__global__ __launch_bounds__(256) void k_cumulative_chunk_max(const ViewshedPlan *__restrict__ plans, const float *__restrict__ hblk, float *__restrict__ cmax)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t b = blockIdx.z >> 1, q = (ZMAJOR ? 2u : 0u) + (blockIdx.z & 1u);
    const ViewshedPlan &V = plans[b];
    const uint32_t k0 = blockIdx.x * kShChunk + 1u, l0 = blockIdx.y * kShLines;
    if (!vs_group_live(V, q, l0, k0)) return;
    const float y_eye = vs_eye(V, hblk);
    float *out = cmax + (((size_t)b * 4u + q) * V.nchunks + blockIdx.x) * V.nlines;
    if constexpr (ZMAJOR) {
        __shared__ float part[4][kShLines];
        float m = -INFINITY;
        for (uint32_t kk = wave; kk < kShChunk; kk += 4u) {
            float D;
            const float y = vs_height(V, hblk, q, l0 + lane, k0 + kk, D);
            m = fmaxf(m, vs_term(y, y_eye, D));
        }
        part[wave][lane] = m;
        __syncthreads();
        if (wave == 0u && l0 + lane < V.nlines)
            out[l0 + lane] = fmaxf(fmaxf(part[0][lane], part[1][lane]), fmaxf(part[2][lane], part[3][lane]));
    } else {
        for (uint32_t g = wave; g < kShLines; g += 4u) {
            const uint32_t line = l0 + g;
            if (line >= V.nlines) break;                       // (wave-uniform)
            if (!vs_live(V, q, line, k0)) continue;            // (wave-uniform)
            float D;
            const float y = vs_height(V, hblk, q, line, k0 + lane, D);
            float m = vs_term(y, y_eye, D);
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            if (lane == 0u) out[line] = m;
        }
    }
}

// k_viewshed_carry for observer blockIdx.y / 4, quadrant blockIdx.y & 3
template <int UNUSED>
__global__ __launch_bounds__(256) void k_cumulative_carry(const ViewshedPlan *__restrict__ plans, float *__restrict__ cmax)
{
    const uint32_t b = blockIdx.y >> 2, q = blockIdx.y & 3u;
    const ViewshedPlan &V = plans[b];
    const uint32_t line = blockIdx.x * 256u + threadIdx.x;
    if (line >= V.nlines) return;
    float run = -INFINITY;
    for (uint32_t c = 0; c < V.nchunks; ++c) {
        if (!vs_live(V, q, line, c * kShChunk + 1u)) break;
        const size_t o = (((size_t)b * 4u + q) * V.nchunks + c) * V.nlines + line;
        const float m = cmax[o];
        cmax[o] = run;
        run = fmaxf(run, m);
    }
}

// The add of step k of a line: by the line that owns the vertex, as vs_store stores; only inside the range, and only a q that is not 0
__device__ __forceinline__ void cv_add(const ViewshedPlan &V, uint32_t q, uint32_t line, uint32_t k, float v, float RR, uint32_t ranged,
                                       uint32_t *__restrict__ sum)
{
    uint32_t i, j;
    int32_t r;
    if (!vs_vertex(V, q, line, k, i, j, r)) return;
    if (q >= 2u && (uint32_t)(r < 0 ? -r : r) >= k) return;
    if (vs_owner(V, k, r) != line) return;
    if (ranged && !((float)(k * k + (uint32_t)(r * r)) <= RR)) return;
    const uint32_t qv = (uint32_t)rintf(v * 65536.0f);          // v in [0, 1]: the product is exact, rintf rounds half to even
    if (qv) (void)__hip_atomic_fetch_add(sum + (size_t)j * V.n + i, qv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// k_viewshed_seen for observer blockIdx.z / 2, quadrant 2 ZMAJOR + (blockIdx.z & 1): the adds are shaped as its stores are -- lane =
// step along a row in the x-major quadrants, lane = line behind the LDS hand-over in the z-major ones
template <bool ZMAJOR>
__global__ __launch_bounds__(256) void k_cumulative_seen(const ViewshedPlan *__restrict__ plans, const float *__restrict__ hblk,
                                                         const float *__restrict__ carry, float RR, uint32_t ranged, uint32_t *__restrict__ sum)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t b = blockIdx.z >> 1, q = (ZMAJOR ? 2u : 0u) + (blockIdx.z & 1u);
    const ViewshedPlan &V = plans[b];
    const uint32_t k0 = blockIdx.x * kShChunk + 1u, l0 = blockIdx.y * kShLines;
    if (!ZMAJOR && blockIdx.x == 0u && blockIdx.y == 0u && (blockIdx.z & 1u) == 0u && threadIdx.x == 0u)     // the observer's own vertex: 1
        (void)__hip_atomic_fetch_add(sum + (size_t)V.jo * V.n + V.io, 65536u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!vs_group_live(V, q, l0, k0)) return;
    const float y_obs = cached_height(hblk, V.nb, V.io, V.jo) * V.exag;
    const float y_eye = y_obs + V.eye_height;
    const bool blind = !isfinite(y_obs);                       // an observer without a height: 1 everywhere in range
    const float *in = carry + (((size_t)b * 4u + q) * V.nchunks + blockIdx.x) * V.nlines;
    if constexpr (ZMAJOR) {
        __shared__ float tile[kShLines * kShPitch];
        for (uint32_t kk = wave; kk < kShChunk; kk += 4u) {
            float D;
            tile[lane * kShPitch + kk] = vs_height(V, hblk, q, l0 + lane, k0 + kk, D);
        }
        __syncthreads();
        for (uint32_t g = wave; g < kShLines; g += 4u) {
            const uint32_t line = l0 + g;
            const float c = vs_live(V, q, line, k0) ? in[line] : -INFINITY;
            const int32_t r = vs_minor(V, min(line, V.nlines - 1u), k0 + lane);
            const float D = sqrtf((float)((k0 + lane) * (k0 + lane) + (uint32_t)(r * r)));
            const float v = vs_scan_seen(V, tile[g * kShPitch + lane], y_eye, D, c);
            tile[g * kShPitch + lane] = blind ? 1.0f : v;
        }
        __syncthreads();
        for (uint32_t kk = wave; kk < kShChunk; kk += 4u) cv_add(V, q, l0 + lane, k0 + kk, tile[lane * kShPitch + kk], RR, ranged, sum);
    } else {
        for (uint32_t g = wave; g < kShLines; g += 4u) {
            const uint32_t line = l0 + g;
            if (line >= V.nlines) break;                       // (wave-uniform)
            if (!vs_live(V, q, line, k0)) continue;            // (wave-uniform)
            float D;
            const float y = vs_height(V, hblk, q, line, k0 + lane, D);
            const float v = vs_scan_seen(V, y, y_eye, D, in[line]);
            cv_add(V, q, line, k0 + lane, blind ? 1.0f : v, RR, ranged, sum);
        }
    }
}

// sum -> count = (float)sum / 65536 (the conversion rounds to nearest even, the scaling is exact) and f = count / N, the field the
// tint pass reads
template <int UNUSED>
__global__ __launch_bounds__(256) void k_cumulative_finish(const uint32_t *__restrict__ sum, uint32_t nv, float observers, float *__restrict__ count,
                                                           float *__restrict__ frac)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    const float c = (float)sum[v] * (1.0f / 65536.0f);
    count[v] = c;
    frac[v] = c / observers;
}

} // namespace vf

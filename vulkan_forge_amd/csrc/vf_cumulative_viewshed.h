// vf_cumulative_viewshed.h -- cumulative viewsheds: how many of N observers see each vertex.
//
// The scan of vf_viewshed.h over a batch of observers at once: its three stage bodies (vs_stage_*), wrapped with the observer's index in
// blockIdx.z and its ViewshedPlan read from a device array, so that a batch costs five launches however many observers it holds.
// Every observer has its own carries (cmax[observer][quadrant][chunk][line]).  The last stage does not store seen: it adds
// q = rint(seen * 65536) to a field of 32-bit sums with a relaxed device-scope atomic.  One observer has one writer per vertex
// (vs_owned), so the atomics meet only between observers, and integer addition commutes: the sums do not depend on batching or on the
// order of arrival.  k_sum_finish (vf_sun_exposure.h) turns the sums into the count and count / N.
//
// The range limit is in the plans the host fills: steps[] and nchunks are cut at ceil(Rc), so a line has no vertex beyond it
// (vs_vertex), chunks beyond it are neither launched nor walked, and the in-range vertices keep the bits of the full scan -- the
// terms before a step do not depend on what comes after it.  RR = Rc * Rc decides which of the walked vertices count.
// All kernels are templates: the library's non-template kernels keep their places.
#pragma once
#include "vf_viewshed.h"

namespace vf {

// the carries of observer b of a batch: every plan of a computation has the same nchunks and nlines
__device__ __forceinline__ size_t cv_carries(const ViewshedPlan &V, uint32_t b) { return (size_t)b * 4u * V.nchunks * V.nlines; }

// k_viewshed_chunk_max for observer blockIdx.z / 2, quadrant 2 ZMAJOR + (blockIdx.z & 1)
template <bool ZMAJOR>
__global__ __launch_bounds__(256) void k_cumulative_chunk_max(const ViewshedPlan *__restrict__ plans, const float *__restrict__ hblk, float *__restrict__ cmax)
{
    const uint32_t b = blockIdx.z >> 1, q = (ZMAJOR ? 2u : 0u) + (blockIdx.z & 1u);
    const ViewshedPlan &V = plans[b];
    vs_stage_chunk_max<ZMAJOR>(V, q, hblk, cmax + cv_carries(V, b) + vs_carries(V, q, blockIdx.x));
}

// k_viewshed_carry for observer blockIdx.y / 4, quadrant blockIdx.y & 3
template <int UNUSED>
__global__ __launch_bounds__(256) void k_cumulative_carry(const ViewshedPlan *__restrict__ plans, float *__restrict__ cmax)
{
    const uint32_t b = blockIdx.y >> 2, q = blockIdx.y & 3u;
    const ViewshedPlan &V = plans[b];
    vs_stage_carry(V, q, cmax + cv_carries(V, b) + vs_carries(V, q, 0u));
}

// The add of step k of a line: by the line that owns the vertex, as vs_store stores; only inside the range, and only a q that is not 0
__device__ __forceinline__ void cv_add(const ViewshedPlan &V, uint32_t q, uint32_t line, uint32_t k, float v, float RR, uint32_t ranged,
                                       uint32_t *__restrict__ sum)
{
    uint32_t i, j;
    int32_t r;
    if (!vs_owned(V, q, line, k, i, j, r)) return;
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
    const uint32_t b = blockIdx.z >> 1, q = (ZMAJOR ? 2u : 0u) + (blockIdx.z & 1u);
    const ViewshedPlan &V = plans[b];
    if (vs_writes_observer<ZMAJOR>(q))                         // the observer's own vertex: 1
        (void)__hip_atomic_fetch_add(sum + (size_t)V.jo * V.n + V.io, 65536u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    vs_stage_seen<ZMAJOR>(V, q, hblk, carry + cv_carries(V, b) + vs_carries(V, q, blockIdx.x),
                          [&](uint32_t q_, uint32_t line, uint32_t k, float v) { cv_add(V, q_, line, k, v, RR, ranged, sum); });
}

} // namespace vf

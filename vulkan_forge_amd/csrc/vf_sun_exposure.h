// vf_sun_exposure.h -- sun exposure: the sum of the shadow fields of N suns, weighted, with an optional incidence cosine.
//
// The scan of vf_shadow.h over a batch of suns at once: its three stage bodies (sh_stage_*), wrapped with the sun's index in blockIdx.z
// and its ShadowPlan read from a device array of ExposureSun records, so that a batch costs three launches per major axis however many
// suns it holds.
// Every sun of a batch has its own carries (cmax[slot][chunk][line], `stride` floats per slot).  The last stage does not store lit: it
// adds q = rint(((lit * c) * w) * 65536) to a field of 32-bit sums with a relaxed device-scope atomic.  One sun has one writer per
// vertex (a vertex lies on one line of a plan), so the atomics meet only between suns, and integer addition commutes: the sums do not
// depend on batching or on the order of arrival.
//
// Suns differ in major axis and in line count: the host launches <false> over the x-major suns of a batch and <true> over its z-major
// ones, with grid.y sized to the part's largest nlines; a workgroup beyond its own sun's lines retires at once.
// All kernels are templates: the library's non-template kernels keep their places.
#pragma once
#include "vf_shadow.h"

namespace vf {

// One sun of a computation (the host fills it: exposure_field in vf_hip.hip)
struct ExposureSun {
    ShadowPlan S;               // strength = 1, the call's softness and bias (unused by a degenerate sun but for n and nb)
    float sx, sy, sz;           // the sun vector as given
    float sl;                   // sqrtf((sx sx + sy sy) + sz sz)
    float w;                    // its weight
};

// px, pz of a vertex: central differences of y = h * exag inside the grid, one-sided on its edges; px = NaN where
// the vertex's own y is not finite
__device__ __forceinline__ float2 se_slope(const float *__restrict__ hblk, uint32_t n, uint32_t nb, float exag, float cell, uint32_t i, uint32_t j)
{
    const uint32_t ip = min(i + 1u, n - 1u), im = i ? i - 1u : 0u, jp = min(j + 1u, n - 1u), jm = j ? j - 1u : 0u;
    // (a vertex without a height of its own has no slope either: inside the grid the differences do not read it)
    const float px = isfinite(cached_height(hblk, nb, i, j) * exag)
                         ? (cached_height(hblk, nb, ip, j) * exag - cached_height(hblk, nb, im, j) * exag) / (cell * (float)(ip - im)) : __builtin_nanf("");
    const float pz = (cached_height(hblk, nb, i, jp) * exag - cached_height(hblk, nb, i, jm) * exag) / (cell * (float)(jp - jm));
    return make_float2(px, pz);
}

// c of a vertex under a sun: the cosine between the surface normal (-px, 1, -pz) and the sun, clamped to [0, 1]; a NaN gives 0
__device__ __forceinline__ float se_cosine(const ExposureSun &E, float2 p)
{
    const float nn = sqrtf((1.0f + p.x * p.x) + p.y * p.y);
    const float c = (((E.sy - p.x * E.sx) - p.y * E.sz) / nn) / E.sl;
    return c > 0.0f ? fminf(c, 1.0f) : 0.0f;
}

// q of a vertex: lit its shadow value under the sun
template <bool INCIDENCE>
__device__ __forceinline__ uint32_t se_quantum(const ExposureSun &E, float lit, const float2 *__restrict__ slope, size_t vertex)
{
    float v = lit;
    if constexpr (INCIDENCE) v = lit * se_cosine(E, slope[vertex]);
    v = v * E.w;
    return (uint32_t)rintf(v * 65536.0f);                      // v in [0, 1]: the product is exact, rintf rounds half to even
}

// The add of step k of a line; only a q that is not 0
template <bool INCIDENCE>
__device__ __forceinline__ void se_add(const ExposureSun &E, uint32_t line, uint32_t k, float lit, const float2 *__restrict__ slope, uint32_t *__restrict__ sum)
{
    uint32_t i, j;
    if (!sh_vertex(E.S, line, k, i, j)) return;
    const size_t o = (size_t)j * E.S.n + i;
    const uint32_t q = se_quantum<INCIDENCE>(E, lit, slope, o);
    if (q) (void)__hip_atomic_fetch_add(sum + o, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// k_shadow_chunk_max for sun blockIdx.z of the part; its carries begin at cmax + blockIdx.z * stride
template <bool ZMAJOR>
__global__ __launch_bounds__(256) void k_exposure_chunk_max(const ExposureSun *__restrict__ suns, const float *__restrict__ hblk, float *__restrict__ cmax,
                                                            size_t stride)
{
    const ShadowPlan &S = suns[blockIdx.z].S;
    if (blockIdx.y * kShLines >= S.nlines) return;             // (a sun with fewer lines than the part's largest)
    sh_stage_chunk_max<ZMAJOR>(S, hblk, cmax + (size_t)blockIdx.z * stride + (size_t)blockIdx.x * S.nlines);
}

// k_shadow_carry for sun blockIdx.y of the batch
template <int UNUSED>
__global__ __launch_bounds__(256) void k_exposure_carry(const ExposureSun *__restrict__ suns, float *__restrict__ cmax, size_t stride)
{
    const ShadowPlan &S = suns[blockIdx.y].S;
    sh_stage_carry(S.nlines, S.nchunks, cmax + (size_t)blockIdx.y * stride);
}

// k_shadow_lit for sun blockIdx.z of the part: the adds are shaped as its stores are -- lane = step along a row for the x-major suns,
// lane = line behind the LDS hand-over for the z-major ones.  (The sun's index as the fastest grid dimension, so that the suns of a
// batch walk one stretch of the grid together, was measured and not kept: DESIGN.md 4n.)
template <bool ZMAJOR, bool INCIDENCE>
__global__ __launch_bounds__(256) void k_exposure_lit(const ExposureSun *__restrict__ suns, const float *__restrict__ hblk, const float *__restrict__ carry,
                                                      size_t stride, const float2 *__restrict__ slope, uint32_t *__restrict__ sum)
{
    const ExposureSun &E = suns[blockIdx.z];
    if (blockIdx.y * kShLines >= E.S.nlines) return;
    sh_stage_lit<ZMAJOR>(E.S, hblk, carry + (size_t)blockIdx.z * stride + (size_t)blockIdx.x * E.S.nlines,
                         [&](uint32_t line, uint32_t k, float lit) { se_add<INCIDENCE>(E, line, k, lit, slope, sum); });
}

// The degenerate suns (no usable horizontal part: lit = 1 everywhere), all `count` of them: one add per vertex
template <bool INCIDENCE>
__global__ __launch_bounds__(256) void k_exposure_flat(const ExposureSun *__restrict__ suns, uint32_t count, const float2 *__restrict__ slope, uint32_t nv,
                                                       uint32_t *__restrict__ sum)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    uint32_t q = 0;
    for (uint32_t o = 0; o < count; ++o) q += se_quantum<INCIDENCE>(suns[o], 1.0f, slope, v);
    if (q) (void)__hip_atomic_fetch_add(sum + v, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// px, pz of every vertex: they depend on no sun, so a computation with incidence forms them once; a workgroup takes 32 x 8 vertices
template <int UNUSED>
__global__ __launch_bounds__(256) void k_exposure_slopes(const float *__restrict__ hblk, uint32_t n, uint32_t nb, float exag, float cell, float2 *__restrict__ slope)
{
    const uint32_t i = blockIdx.x * 32u + (threadIdx.x & 31u), j = blockIdx.y * 8u + (threadIdx.x >> 5);
    if (i >= n || j >= n) return;
    slope[(size_t)j * n + i] = se_slope(hblk, n, nb, exag, cell, i, j);
}

// The end of a summed field, for this one and for the cumulative viewshed (vf_cumulative_viewshed.h): sum -> value = (float)sum / 65536
// (the conversion rounds to nearest even, the scaling is exact) and frac = min(value / total, 1), the field the tint pass reads (0
// when total is not > 0: no sun's weight counts).
// The cumulative viewshed passes total = (float)N and reads frac as count / N: for it the fminf is the identity and total >= 1.  Every
// observer adds at most 65536 to a vertex, so sum <= N * 65536; with N <= 65535 that bound is a float, and the conversion is monotonic,
// so value <= N and value / N <= 1.
template <int UNUSED>
__global__ __launch_bounds__(256) void k_sum_finish(const uint32_t *__restrict__ sum, uint32_t nv, float total, float *__restrict__ value,
                                                    float *__restrict__ frac)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    const float e = (float)sum[v] * (1.0f / 65536.0f);
    value[v] = e;
    frac[v] = total > 0.0f ? fminf(e / total, 1.0f) : 0.0f;
}

} // namespace vf

// vf_resolve.h -- the resolve of a supersampled frame: the (F H, F W) sample buffer the terrain passes drew -> the
// (H, W) frame the overlays composite onto and the caller reads.  One launch per frame of a handle with F > 1, behind the last tint
// and in front of the overlay pass; a handle with F = 1 never launches it.
//
// The arithmetic is the contract's, bit for bit (tests/supersample_model/supersample_model.py is its CPU statement), per output pixel
// and colour channel:
//   1. lin = decode[byte]                      the context's sRGB8 -> linear table
//   2. acc = the F x F samples added in binary32, rows outer, columns inner, starting from the first sample (not from 0)
//   3. c = acc * inv,  inv = 1.0f / (float)(F F) rounded to binary32          (the library is built without contraction: no fma)
//   4. byte = srgb_encode(c)                   over the threshold table, as every frame store does
//   5. alpha = (sum of the F F alpha bytes + F F / 2) / (F F)                 integer mean, half up
//
// A pure streaming kernel: every sample byte is read once, every output byte written once.  A lane owns PX neighbouring output pixels
// and reads, from each of the F sample rows under them, the F PX contiguous samples -- 16 bytes for F = 2 (PX = 2) and F = 4 (PX = 1),
// 48 bytes for F = 3 (PX = 4) -- so a wave reads whole contiguous row segments.  The loads are 16 bytes wide where the lane's segment is
// whole and 16-byte aligned, dwords otherwise: a sample row starts on a 16-byte boundary only when F W (y F + sy) is a multiple of 4, which
// holds for every row of F = 4 and, for F = 2 and 3, for every row when W is even / a multiple of 4 and every second / fourth row otherwise.
// Rows that end inside a lane's segment take the dword form with a bound per sample; no address outside [0, F H x F W) is formed into a load.
// The kernel is a template: the library's non-template kernels keep their places.
#pragma once
#include "vf_device.h"

namespace vf {

// output pixels per lane
template <int F> struct SsShape { static constexpr int PX = F == 2 ? 2 : (F == 3 ? 4 : 1); };

// N samples of one sample row from column x0 on; sw: samples per row.  Samples at or beyond sw read as 0 (their pixels are not stored).
template <int N>
__device__ __forceinline__ void ss_load_row(const uint32_t *__restrict__ row, uint32_t x0, uint32_t sw, uint32_t v[N])
{
    static_assert(N % 4 == 0, "whole 16-byte words");
    const uint32_t *p = row + x0;
    if (x0 + (uint32_t)N <= sw && (reinterpret_cast<uintptr_t>(p) & 15u) == 0u) {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const uint4 w = reinterpret_cast<const uint4 *>(p)[q];
            v[4 * q] = w.x; v[4 * q + 1] = w.y; v[4 * q + 2] = w.z; v[4 * q + 3] = w.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = x0 + (uint32_t)k < sw ? p[k] : 0u;
    }
}

// samples (F H, F W) RGBA8 words, row-major -> out (H, W).  Persistent: the workgroups walk the lanes' work with a grid stride, so the
// two 1 KB tables are staged once per workgroup, not once per 256 lanes of work.
template <int F>
__global__ __launch_bounds__(256) void k_ss_resolve(const uint32_t *__restrict__ samples, uint32_t W, uint32_t H, const float *__restrict__ decode,
                                                    const float *__restrict__ thresh, uint32_t *__restrict__ out)
{
    constexpr int PX = SsShape<F>::PX, N = F * PX;
    constexpr uint32_t FF = (uint32_t)(F * F);
    __shared__ float s_dec[256];
    __shared__ float s_thr[256];
    s_dec[threadIdx.x] = decode[threadIdx.x];
    s_thr[threadIdx.x] = thresh[threadIdx.x];
    __syncthreads();
    const float inv = 1.0f / (float)FF;
    const uint32_t sw = (uint32_t)F * W;
    const uint32_t lpr = (W + (uint32_t)PX - 1u) / (uint32_t)PX;           // lanes per output row
    const uint32_t total = lpr * H;                                       // (< 2^27: W H <= 16384^2 / F^2)
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const uint32_t y = idx / lpr, x0 = (idx - y * lpr) * (uint32_t)PX;
        uint32_t v[F][N];
#pragma unroll
        for (int sy = 0; sy < F; ++sy) ss_load_row<N>(samples + (size_t)(y * (uint32_t)F + (uint32_t)sy) * sw, x0 * (uint32_t)F, sw, v[sy]);
        uint32_t px[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            uint32_t word = 0u;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float acc = s_dec[(v[0][p * F] >> (8 * ch)) & 255u];
#pragma unroll
                for (int sy = 0; sy < F; ++sy)
#pragma unroll
                    for (int sx = 0; sx < F; ++sx)
                        if (sy || sx) acc = acc + s_dec[(v[sy][p * F + sx] >> (8 * ch)) & 255u];
                word |= srgb_encode(acc * inv, s_thr) << (8 * ch);
            }
            uint32_t a = 0u;
#pragma unroll
            for (int sy = 0; sy < F; ++sy)
#pragma unroll
                for (int sx = 0; sx < F; ++sx) a += v[sy][p * F + sx] >> 24;
            px[p] = word | (((a + FF / 2u) / FF) << 24);
        }
        uint32_t *o = out + (size_t)y * W + x0;
        if (PX == 4 && x0 + 4u <= W && (reinterpret_cast<uintptr_t>(o) & 15u) == 0u)
            *reinterpret_cast<uint4 *>(o) = make_uint4(px[0], px[PX > 1 ? 1 : 0], px[PX > 2 ? 2 : 0], px[PX > 3 ? 3 : 0]);
        else if (PX == 2 && x0 + 2u <= W && (reinterpret_cast<uintptr_t>(o) & 7u) == 0u)
            *reinterpret_cast<uint2 *>(o) = make_uint2(px[0], px[PX > 1 ? 1 : 0]);
        else {
#pragma unroll
            for (int p = 0; p < PX; ++p) if (x0 + (uint32_t)p < W) o[p] = px[p];
        }
    }
}

} // namespace vf

// vf_drape_mips.h -- a mip pyramid under the draped image and trilinear filtering of it.
//
//   the pyramid         level 0 is the RGBA8 image of vf_drape.h.  Level k >= 1 is (w_k, h_k) = (max(1, (w_{k-1} + 1) >> 1), likewise)
//                       texels of premultiplied linear (r, g, b, a) as four binary16 values, 8 bytes each, row-major; texel (i, j) is
//                       the mean of the parents (2i + {0, 1}, 2j + {0, 1}) that exist
//   the build kernel    k_drape_mips<FROM8>: one launch reads a level once and writes the next three
//   the level of detail mip_lod: from the (x, z) of the same primitive one pixel to the right and one below
//   the sampler         mip_sample: dr_sample where the image is magnified, else one or two levels of the pyramid
//   the shade pass      k_relight<., kDrapeMip> (vf_relight.h)
//
// The arithmetic is the contract's, bit for bit (tests/drape_mip_model/drape_mip_model.c is its CPU statement).  No float becomes a
// level or a texel index before it has been compared with the number of levels or clamped.  All kernels are templates.
#pragma once
#include "vf_drape.h"

namespace vf {

constexpr int kMipLevelsMax = 15;           // 16384 = 2^14: levels 0 ... 14

// What the shade pass reads of a pyramid: lvl[k] = level k's texels (k >= 1; lvl[0] is not read), its size in w[k] x h[k]
struct DrapeMips {
    const uint2 *lvl[kMipLevelsMax];
    uint16_t w[kMipLevelsMax], h[kMipLevelsMax];
    uint32_t levels;
    float bias;
};

// a relight pass's last kernel argument: the pyramid for kDrapeMip, nothing for the others
struct NoMips {};

// ---- binary16 ----------------------------------------------------------------------------------
// four binary32 values -> four binary16 values, round to nearest even each (a plain conversion: not the packed round-towards-zero one)
__device__ __forceinline__ uint2 mip_pack(const float q[4])
{
    const _Float16 a = (_Float16)q[0], b = (_Float16)q[1], c = (_Float16)q[2], d = (_Float16)q[3];
    return make_uint2((uint32_t)__builtin_bit_cast(uint16_t, a) | (uint32_t)__builtin_bit_cast(uint16_t, b) << 16,
                      (uint32_t)__builtin_bit_cast(uint16_t, c) | (uint32_t)__builtin_bit_cast(uint16_t, d) << 16);
}

__device__ __forceinline__ void mip_unpack(uint2 t, float q[4])
{
    q[0] = (float)__builtin_bit_cast(_Float16, (uint16_t)(t.x & 0xFFFFu)); q[1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(t.x >> 16));
    q[2] = (float)__builtin_bit_cast(_Float16, (uint16_t)(t.y & 0xFFFFu)); q[3] = (float)__builtin_bit_cast(_Float16, (uint16_t)(t.y >> 16));
}

// The mean of the parents that exist, as the texel stored: p00 always exists, p01 when e01 (the parent to the right), p10 when e10
// (the one below), p11 when both.  The sum in that order in binary32, times 1 / count (a power of two), then rounded.
__device__ __forceinline__ uint2 mip_mean(uint2 p00, uint2 p01, uint2 p10, uint2 p11, bool e01, bool e10)
{
    float a[4], b[4], c[4], d[4], m[4];
    mip_unpack(p00, a); mip_unpack(p01, b); mip_unpack(p10, c); mip_unpack(p11, d);
    const float inv = e01 ? (e10 ? 0.25f : 0.5f) : (e10 ? 0.5f : 1.0f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float s = a[k];
        if (e01) s = s + b[k];
        if (e10) s = s + c[k];
        if (e01 && e10) s = s + d[k];
        m[k] = s * inv;
    }
    return mip_pack(m);
}

__device__ __forceinline__ uint2 mip_shfl_xor(uint2 v, int mask)
{
    return make_uint2((uint32_t)__shfl_xor((int)v.x, mask, 64), (uint32_t)__shfl_xor((int)v.y, mask, 64));
}

// ---- the build kernel ----------------------------------------------------------------------------
// One level (sw x sh texels: FROM8 the RGBA8 image, else binary16 texels) -> the next `nout` levels (1 ... 3): d1 of (w1, h1) =
// ((sw + 1) >> 1, (sh + 1) >> 1) texels, d2 and d3 halved again.  The levels share their origin, so an aligned 8 x 8 block of the
// source gives 4 x 4, 2 x 2 and 1 texels of them and the source is read once.  A lane holds 4 x 2 source texels (16 bytes of each of
// two rows from the image, 32 from binary16 texels) and makes two texels of d1; a wave holds 64 x 8: lane = (lx, ly) = (lane & 15,
// lane >> 4).  A texel of d2 is formed by the lane with even ly from its own two and those of the lane below (lane ^ 16), a texel
// of d3 by the lane with even lx and ly = 0 (mod 4) from the d2 texels of lanes ^ 1, ^ 32 and ^ 33: every parent is the *stored*
// binary16 value, so the three levels have the bits that one launch per level gives.  Four waves of a workgroup lie below one
// another.  Vector loads where a row's start is 16-byte aligned (sw a multiple of four for the image, of two for texels) -- a group
// of four texels is then inside the row or outside it; single texels with their own bounds test otherwise.  Texel indices are 64-bit.
template <bool FROM8>
__global__ __launch_bounds__(256) void k_drape_mips(const void *__restrict__ src, const float *__restrict__ decode, uint32_t sw, uint32_t sh, uint32_t nout,
                                                     uint2 *__restrict__ d1, uint2 *__restrict__ d2, uint2 *__restrict__ d3)
{
    __shared__ float s_dec[256];
    if constexpr (FROM8) { s_dec[threadIdx.x] = decode[threadIdx.x]; __syncthreads(); }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t gx = blockIdx.x * 16u + (lane & 15u), gy = (blockIdx.y * 4u + wave) * 4u + (lane >> 4);   // this lane's place in the grid of 4 x 2 regions
    const uint32_t x0 = gx * 4u, y0 = gy * 2u;
    const uint32_t w1 = (sw + 1u) >> 1, h1 = (sh + 1u) >> 1;

    // the 4 x 2 source texels as binary32 premultiplied colour (zero where there is none), two rows
    float p[2][4][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t y = y0 + (uint32_t)r;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) p[r][c][k] = 0.0f;
        if (y >= sh || x0 >= sw) continue;
        const size_t row = (size_t)y * sw;
        if constexpr (FROM8) {
            const uint32_t *img = (const uint32_t *)src;
            uint32_t t[4] = { 0u, 0u, 0u, 0u };
            if ((sw & 3u) == 0u) { const uint4 v = *(const uint4 *)(img + row + x0); t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w; }
            else {
#pragma unroll
                for (int c = 0; c < 4; ++c) if (x0 + (uint32_t)c < sw) t[c] = img[row + x0 + (uint32_t)c];
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {                    // dr_texel's values
                const float a = (float)(t[c] >> 24) / 255.0f;
                p[r][c][0] = s_dec[t[c] & 255u] * a; p[r][c][1] = s_dec[(t[c] >> 8) & 255u] * a; p[r][c][2] = s_dec[(t[c] >> 16) & 255u] * a; p[r][c][3] = a;
            }
        } else {
            const uint2 *tex = (const uint2 *)src;
            uint2 t[4] = { make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u) };
            if ((sw & 1u) == 0u) {
                const uint4 v = *(const uint4 *)(tex + row + x0);
                t[0] = make_uint2(v.x, v.y); t[1] = make_uint2(v.z, v.w);
                if (x0 + 2u < sw) { const uint4 u = *(const uint4 *)(tex + row + x0 + 2u); t[2] = make_uint2(u.x, u.y); t[3] = make_uint2(u.z, u.w); }
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) if (x0 + (uint32_t)c < sw) t[c] = tex[row + x0 + (uint32_t)c];
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) mip_unpack(t[c], p[r][c]);
        }
    }

    // d1: texels (2 gx + c, gy), c = 0, 1, from source columns x0 + 2 c + {0, 1} and rows y0 + {0, 1}
    const bool e10 = y0 + 1u < sh;
    uint2 t1[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const bool e01 = x0 + 2u * (uint32_t)c + 1u < sw;
        const float inv = e01 ? (e10 ? 0.25f : 0.5f) : (e10 ? 0.5f : 1.0f);
        float m[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float s = p[0][2 * c][k];
            if (e01) s = s + p[0][2 * c + 1][k];
            if (e10) s = s + p[1][2 * c][k];
            if (e01 && e10) s = s + p[1][2 * c + 1][k];
            m[k] = s * inv;
        }
        t1[c] = mip_pack(m);
    }
    const uint32_t cx = gx * 2u;
    if (gy < h1 && cx < w1) {
        uint2 *o = d1 + (size_t)gy * w1 + cx;
        if (cx + 1u < w1 && (w1 & 1u) == 0u) *(uint4 *)o = make_uint4(t1[0].x, t1[0].y, t1[1].x, t1[1].y);
        else { o[0] = t1[0]; if (cx + 1u < w1) o[1] = t1[1]; }
    }
    if (nout < 2u) return;                                   // (uniform)

    // d2: texel (gx, gy >> 1) from the d1 texels (2 gx + {0, 1}, 2 (gy >> 1) + {0, 1}): this lane's pair above, lane ^ 16's below
    const uint32_t w2 = (w1 + 1u) >> 1, h2 = (h1 + 1u) >> 1;
    const uint2 o0 = mip_shfl_xor(t1[0], 16), o1 = mip_shfl_xor(t1[1], 16);
    const bool low = (gy & 1u) != 0u;                        // this lane holds the lower pair
    const uint32_t j2 = gy >> 1;
    const uint2 t2 = mip_mean(low ? o0 : t1[0], low ? o1 : t1[1], low ? t1[0] : o0, low ? t1[1] : o1, cx + 1u < w1, 2u * j2 + 1u < h1);
    if (!low && gx < w2 && j2 < h2) d2[(size_t)j2 * w2 + gx] = t2;
    if (nout < 3u) return;

    // d3: texel (gx >> 1, gy >> 2) from the d2 texels (2 (gx >> 1) + {0, 1}, 2 (gy >> 2) + {0, 1}): lanes ^ 1 right, ^ 32 below
    const uint32_t w3 = (w2 + 1u) >> 1, h3 = (h2 + 1u) >> 1;
    const uint2 r = mip_shfl_xor(t2, 1), b = mip_shfl_xor(t2, 32), rb = mip_shfl_xor(t2, 33);
    const uint32_t i3 = gx >> 1, j3 = gy >> 2;
    const uint2 t3 = mip_mean(t2, r, b, rb, 2u * i3 + 1u < w2, 2u * j3 + 1u < h2);
    if ((gx & 1u) == 0u && (gy & 3u) == 0u && i3 < w3 && j3 < h3) d3[(size_t)j3 * w3 + i3] = t3;
}

// ---- the level of detail -------------------------------------------------------------------------
// (x, z) at the pixel, (xr, zr) one pixel to the right and (xd, zd) one below -> lod; -inf: level 0 (rho2 NaN, zero, denormal or
// negative), +inf: the top level.  The piecewise-linear logarithm of rho2's bits: never above 0.5 log2(rho2), at most 0.0431 below.
__device__ __forceinline__ float mip_lod(const DrapeParams &D, float bias, float x, float z, float xr, float zr, float xd, float zd)
{
    const float dux = (xr - x) * D.sx, dvx = (zr - z) * D.sz;
    const float ax = fmaf(dux, dux, dvx * dvx);
    const float duy = (xd - x) * D.sx, dvy = (zd - z) * D.sz;
    const float ay = fmaf(duy, duy, dvy * dvy);
    const float rho2 = ay > ax ? ay : ax;
    const uint32_t bits = __float_as_uint(rho2);
    const uint32_t E = (bits >> 23) & 255u, M = bits & 0x7FFFFFu;
    if ((bits >> 31) != 0u || E == 0u || (E == 255u && M != 0u)) return -INFINITY;
    if (E == 255u) return INFINITY;
    return 0.5f * ((float)((int)E - 127) + (float)M * 0x1p-23f) + bias;
}

// ---- the sampler ---------------------------------------------------------------------------------
// Level k >= 1 at level-0 coordinates (fu, fv) inside the image: item 4 / 5 of 4j at (fu, fv) 2^-k with the level's sizes
__device__ __forceinline__ void mip_level_sample(const DrapeMips &M, int k, bool linear, float fu, float fv, float val[4])
{
    const float sc = __uint_as_float((uint32_t)(127 - k) << 23);       // 2^-k
    const float fuk = fu * sc, fvk = fv * sc;
    const uint2 *__restrict__ tex = M.lvl[k];
    const uint32_t wk = M.w[k], hk = M.h[k];
    const int mx = (int)wk - 1, my = (int)hk - 1;
    if (!linear) {
        mip_unpack(tex[(size_t)min((int)floorf(fvk), my) * wk + (size_t)min((int)floorf(fuk), mx)], val);
        return;
    }
    const float cu = fuk - 0.5f, cv = fvk - 0.5f;
    const float i0f = floorf(cu), j0f = floorf(cv);
    const float fx = cu - i0f, fy = cv - j0f;
    const int c0 = min(max((int)i0f, 0), mx), c1 = min(max((int)i0f + 1, 0), mx);
    const int r0 = min(max((int)j0f, 0), my), r1 = min(max((int)j0f + 1, 0), my);
    float q00[4], q01[4], q10[4], q11[4];
    mip_unpack(tex[(size_t)r0 * wk + (size_t)c0], q00); mip_unpack(tex[(size_t)r0 * wk + (size_t)c1], q01);
    mip_unpack(tex[(size_t)r1 * wk + (size_t)c0], q10); mip_unpack(tex[(size_t)r1 * wk + (size_t)c1], q11);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float top = fmaf(fx, q01[c] - q00[c], q00[c]);
        const float bot = fmaf(fx, q11[c] - q10[c], q10[c]);
        val[c] = fmaf(fy, bot - top, top);
    }
}

// level k of the pyramid, level 0 through dr_sample (the caller's inside test has passed, so it returns true)
__device__ __forceinline__ void mip_any_level(const DrapeParams &D, const DrapeMips &M, const uint32_t *__restrict__ img, const float *dec, int k,
                                              float x, float z, float fu, float fv, float val[4])
{
    if (k == 0) (void)dr_sample(D, img, dec, x, z, val);
    else mip_level_sample(M, k, D.linear != 0u, fu, fv, val);
}

// The image at world (x, z) with level of detail `lod`: false outside the extent, as dr_sample
__device__ __forceinline__ bool mip_sample(const DrapeParams &D, const DrapeMips &M, const uint32_t *__restrict__ img, const float *dec, float x, float z,
                                           float lod, float val[4])
{
    if (!(lod > 0.0f)) return dr_sample(D, img, dec, x, z, val);      // magnified: 4j's sample, the same bits
    const float fu = (x - D.x0) * D.sx, fv = (z - D.z0) * D.sz;
    if (!(fu >= 0.0f && fu <= (float)D.iw && fv >= 0.0f && fv <= (float)D.ih)) return false;
    const int top = (int)M.levels - 1;
    if (!D.linear) {
        const float ln = lod + 0.5f;
        mip_any_level(D, M, img, dec, ln >= (float)top ? top : (int)floorf(ln), x, z, fu, fv, val);
        return true;
    }
    if (lod >= (float)top) { mip_any_level(D, M, img, dec, top, x, z, fu, fv, val); return true; }
    const float lf = floorf(lod), t = lod - lf;
    const int l = (int)lf;
    float lo[4], hi[4];
    mip_any_level(D, M, img, dec, l, x, z, fu, fv, lo);
    mip_level_sample(M, l + 1, true, fu, fv, hi);
#pragma unroll
    for (int c = 0; c < 4; ++c) val[c] = fmaf(t, hi[c] - lo[c], lo[c]);
    return true;
}

} // namespace vf

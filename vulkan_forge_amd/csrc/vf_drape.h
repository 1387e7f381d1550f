// vf_drape.h -- a draped image layer: an RGBA8 raster as the terrain's albedo.
//
//   the image           row-major RGBA8 in device memory, iw * 4 bytes per row, sRGB with straight alpha; row 0 lies at the extent's
//                       z0 and column 0 at its x0 (k_drape_expand makes it from an RGB upload)
//   the sampler         dr_sample: the image at world (x, z), nearest or bilinear, as premultiplied linear colour and alpha
//   the shade pass      k_relight<., kDrape> (vf_relight.h): the image sampled at the (x, z) of every covered pixel, and
//                       where the sample is not transparent the pixel written again through the exact fragment function with the
//                       colormap value mixed with the sample
//
// Launched only for a handle that holds a drape.  The arithmetic is the contract's, bit for bit (tests/drape_model/drape_model.c is
// its CPU statement).  No float becomes a texel index before the inside test has passed: every index below is formed from a value
// in [-1, iw] (or ih) and clamped.  All kernels are templates.
#pragma once
#include "vf_ambient.h"

namespace vf {

// What the host passes of a drape: sx = (float)iw / (x1 - x0), sz = (float)ih / (z1 - z0), one division each
struct DrapeParams {
    float x0, z0, sx, sz;
    uint32_t iw, ih;
    float opacity;
    uint32_t linear;            // VF_DRAPE_LINEAR / VF_DRAPE_NEAREST
};

// RGB bytes -> RGBA8 words with alpha 255, one thread per texel
template <int UNUSED>
__global__ __launch_bounds__(256) void k_drape_expand(size_t count, const uint8_t *__restrict__ rgb, uint32_t *__restrict__ rgba)
{
    const size_t k = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (k < count) rgba[k] = (uint32_t)rgb[3u * k] | (uint32_t)rgb[3u * k + 1u] << 8 | (uint32_t)rgb[3u * k + 2u] << 16 | 0xFF000000u;
}

// texel (ix, iy), 0 <= ix < iw and 0 <= iy < ih: premultiplied linear colour and alpha
__device__ __forceinline__ void dr_texel(const uint32_t *__restrict__ img, const float *dec, uint32_t iw, int ix, int iy, float q[4])
{
    const uint32_t w = img[(size_t)iy * iw + (size_t)ix];
    const float a = (float)(w >> 24) / 255.0f;
    q[0] = dec[w & 255u] * a; q[1] = dec[(w >> 8) & 255u] * a; q[2] = dec[(w >> 16) & 255u] * a; q[3] = a;
}

// The image at world (x, z): false outside the extent (a NaN is outside), else val = premultiplied (r, g, b) and alpha
__device__ __forceinline__ bool dr_sample(const DrapeParams &D, const uint32_t *__restrict__ img, const float *dec, float x, float z, float val[4])
{
    const float fu = (x - D.x0) * D.sx, fv = (z - D.z0) * D.sz;
    const float fw = (float)D.iw, fh = (float)D.ih;
    if (!(fu >= 0.0f && fu <= fw && fv >= 0.0f && fv <= fh)) return false;
    const int mx = (int)D.iw - 1, my = (int)D.ih - 1;
    if (!D.linear) {
        dr_texel(img, dec, D.iw, min((int)floorf(fu), mx), min((int)floorf(fv), my), val);
        return true;
    }
    const float cu = fu - 0.5f, cv = fv - 0.5f;
    const float i0f = floorf(cu), j0f = floorf(cv);
    const float fx = cu - i0f, fy = cv - j0f;
    const int c0 = min(max((int)i0f, 0), mx), c1 = min(max((int)i0f + 1, 0), mx);
    const int r0 = min(max((int)j0f, 0), my), r1 = min(max((int)j0f + 1, 0), my);
    float q00[4], q01[4], q10[4], q11[4];
    dr_texel(img, dec, D.iw, c0, r0, q00); dr_texel(img, dec, D.iw, c1, r0, q01);
    dr_texel(img, dec, D.iw, c0, r1, q10); dr_texel(img, dec, D.iw, c1, r1, q11);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float top = fmaf(fx, q01[k] - q00[k], q00[k]);
        const float bot = fmaf(fx, q11[k] - q10[k], q10[k]);
        val[k] = fmaf(fy, bot - top, top);
    }
    return true;
}

} // namespace vf

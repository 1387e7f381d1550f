// vf_drape_aniso.h -- anisotropic filtering of the draped image's mip sampling.
//
//   the plan            aniso_plan: from the pixel's footprint on the image (4k item 2) its major screen axis, the level of detail of
//                       the minor axis and the number of taps N <= A along the major one
//   the sampler         aniso_sample: the mean of N taps, each 4k's sample (one or two levels, or for `nearest` the nearest texel of
//                       the nearest level) at texel coordinates clamped to the image rectangle
//   the shade pass      k_relight<., kDrapeAniso> (vf_relight.h)
//
// A pixel whose footprint is near-isotropic (or NaN), and one whose plan gives one tap, is mip_sample's unchanged.  The arithmetic is
// the contract's, bit for bit (tests/drape_aniso_model/drape_aniso_model.c is its CPU statement).  What belongs to the pixel and not
// to the tap -- the levels, their pointers, sizes and scales, the blend weight -- is formed once, before the tap loop.
#pragma once
#include "vf_drape_mips.h"

namespace vf {

struct AnisoPlan {
    float lod;                  // bias included; -inf: level 0, +inf: the top level (mip_lod's values)
    uint32_t n;                 // taps, 1 ... A; 1: mip_sample at the pixel's own (x, z)
    float dum, dvm;             // the footprint's major axis in texels of level 0
};

// 4k item 3's bit procedure on a squared length, plus bias
__device__ __forceinline__ float aniso_lod_of(float rho2, float bias)
{
    const uint32_t bits = __float_as_uint(rho2);
    const uint32_t E = (bits >> 23) & 255u, M = bits & 0x7FFFFFu;
    if ((bits >> 31) != 0u || E == 0u || (E == 255u && M != 0u)) return -INFINITY;
    if (E == 255u) return INFINITY;
    return 0.5f * ((float)((int)E - 127) + (float)M * 0x1p-23f) + bias;
}

// Items 1 - 4: (x, z) at the pixel, one pixel to the right and one below -> the plan.  inv_a2 = 1 / A^2 (a power of two).
__device__ __forceinline__ AnisoPlan aniso_plan(const DrapeParams &D, float bias, uint32_t A, float inv_a2, float x, float z, float xr, float zr,
                                                float xd, float zd)
{
    const float dux = (xr - x) * D.sx, dvx = (zr - z) * D.sz;
    const float ax = fmaf(dux, dux, dvx * dvx);
    const float duy = (xd - x) * D.sx, dvy = (zd - z) * D.sz;
    const float ay = fmaf(duy, duy, dvy * dvy);
    const bool ymajor = ay > ax;
    const float amax = ymajor ? ay : ax, amin = ymajor ? ax : ay;
    AnisoPlan p;
    p.dum = ymajor ? duy : dux; p.dvm = ymajor ? dvy : dvx;
    if (!(amax > 1.5625f * amin)) { p.lod = aniso_lod_of(amax, bias); p.n = 1u; return p; }   // ratio <= 1.25, or a NaN: 4k's pixel
    const float t = amax * inv_a2;
    const float m2 = amin > t ? amin : t;
    p.lod = aniso_lod_of(m2, bias);
    uint32_t n = 1u;
    while (n < A && !(amax <= (float)(n * n) * m2)) ++n;
    p.n = n;
    return p;
}

// A level as a tap reads it: level 0 is the RGBA8 image (tex NULL), level k >= 1 binary16 texels; sc = 2^-k
struct AnisoLevel {
    const uint2 *tex;
    uint32_t w, h;
    float sc;
};

__device__ __forceinline__ AnisoLevel aniso_level(const DrapeParams &D, const DrapeMips &M, int k)
{
    AnisoLevel L;
    L.tex = k ? M.lvl[k] : nullptr;
    L.w = k ? (uint32_t)M.w[k] : D.iw; L.h = k ? (uint32_t)M.h[k] : D.ih;
    L.sc = __uint_as_float((uint32_t)(127 - k) << 23);
    return L;
}

__device__ __forceinline__ void aniso_texel(const AnisoLevel &L, const uint32_t *__restrict__ img, const float *dec, int ix, int iy, float q[4])
{
    if (L.tex) mip_unpack(L.tex[(size_t)iy * L.w + (size_t)ix], q);
    else dr_texel(img, dec, L.w, ix, iy, q);
}

// One level at the level-0 texel coordinates (fu, fv), 0 <= fu <= iw and 0 <= fv <= ih: mip_level_sample's arithmetic, which at
// level 0 (sc = 1) is dr_sample's behind its inside test
__device__ __forceinline__ void aniso_level_sample(const AnisoLevel &L, const uint32_t *__restrict__ img, const float *dec, bool linear, float fu, float fv,
                                                   float val[4])
{
    const float fuk = fu * L.sc, fvk = fv * L.sc;
    const int mx = (int)L.w - 1, my = (int)L.h - 1;
    if (!linear) {
        aniso_texel(L, img, dec, min((int)floorf(fuk), mx), min((int)floorf(fvk), my), val);
        return;
    }
    const float cu = fuk - 0.5f, cv = fvk - 0.5f;
    const float i0f = floorf(cu), j0f = floorf(cv);
    const float fx = cu - i0f, fy = cv - j0f;
    const int c0 = min(max((int)i0f, 0), mx), c1 = min(max((int)i0f + 1, 0), mx);
    const int r0 = min(max((int)j0f, 0), my), r1 = min(max((int)j0f + 1, 0), my);
    float q00[4], q01[4], q10[4], q11[4];
    aniso_texel(L, img, dec, c0, r0, q00); aniso_texel(L, img, dec, c1, r0, q01);
    aniso_texel(L, img, dec, c0, r1, q10); aniso_texel(L, img, dec, c1, r1, q11);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float top = fmaf(fx, q01[c] - q00[c], q00[c]);
        const float bot = fmaf(fx, q11[c] - q10[c], q10[c]);
        val[c] = fmaf(fy, bot - top, top);
    }
}

// Items 5 and 6 for a plan of n > 1 taps: (fu, fv) are the pixel's texel coordinates, inside the image
__device__ __forceinline__ void aniso_sample(const DrapeParams &D, const DrapeMips &M, const uint32_t *__restrict__ img, const float *dec, float fu, float fv,
                                             const AnisoPlan &p, float val[4])
{
    // the pixel's levels: k0 alone, or k0 and k0 + 1 blended with weight t (mip_sample's choice)
    const int top = (int)M.levels - 1;
    const bool linear = D.linear != 0u;
    const float lod = p.lod;
    int k0 = 0;
    bool two = false;
    float t = 0.0f;
    if (lod > 0.0f) {
        if (!linear) { const float ln = lod + 0.5f; k0 = ln >= (float)top ? top : (int)floorf(ln); }
        else if (lod >= (float)top) k0 = top;
        else { const float lf = floorf(lod); t = lod - lf; k0 = (int)lf; two = true; }
    }
    const AnisoLevel L0 = aniso_level(D, M, k0), L1 = aniso_level(D, M, two ? k0 + 1 : k0);
    const float w = 1.0f / (float)p.n, fw = (float)D.iw, fh = (float)D.ih;
    float sum[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (uint32_t i = 0; i < p.n; ++i) {
        const float o = ((float)i + 0.5f) * w - 0.5f;
        const float fui = fminf(fmaxf(fmaf(o, p.dum, fu), 0.0f), fw), fvi = fminf(fmaxf(fmaf(o, p.dvm, fv), 0.0f), fh);
        float v[4];
        aniso_level_sample(L0, img, dec, linear, fui, fvi, v);
        if (two) {
            float hi[4];
            aniso_level_sample(L1, img, dec, true, fui, fvi, hi);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = fmaf(t, hi[c] - v[c], v[c]);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) sum[c] = i ? sum[c] + v[c] : v[c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) val[c] = sum[c] * w;
}

} // namespace vf

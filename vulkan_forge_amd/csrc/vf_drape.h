// vf_drape.h -- a draped image layer: an RGBA8 raster as the terrain's albedo.
//
//   the image           row-major RGBA8 in device memory, iw * 4 bytes per row, sRGB with straight alpha; row 0 lies at the extent's
//                       z0 and column 0 at its x0 (k_drape_expand makes it from an RGB upload)
//   the shade pass      k_drape_shade is k_shadow_shade's walk over the frame's stored visibility: the varyings (h, x, z) of every
//                       covered pixel, the image sampled at (x, z), and where the sample is not transparent the pixel written again
//                       through the exact fragment function with the colormap value mixed with the sample; lit and amb (4g, 4i) are
//                       formed here by their passes' rules, so the result does not depend on what those passes wrote before
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

// fragment_shader_lit (vf_kernels.h) with the colormap value lc of every channel replaced by the albedo
// fmaf(opacity, val, keep * lc), keep = 1 - val_a * opacity.  Its own text: fragment_shader_lit and the kernels it is inlined into
// stay as they are.
__device__ __forceinline__ uint32_t fragment_shader_drape(const FrameParams &P, const ShadeTables &S, const float attr[3], float lit, float amb,
                                                          const float val[4], float opacity, float keep)
{
    const float height = attr[0], x = attr[1], z = attr[2];
    float t = 0.5f + height / (2.0f * P.h_range);
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    float c = t * 256.0f - 0.5f;
    float i0f = floorf(c);
    float f = c - i0f;
    int i0 = (int)i0f, i1 = i0 + 1;
    i0 = min(max(i0, 0), 255); i1 = min(max(i1, 0), 255);
    float nx, ny, nz;
    if (P.shade_mode == 0u) {
        float dhdx = 1.3f * det_cos(x * 1.3f) * 0.25f;
        float dhdz = -1.1f * det_sin(z * 1.1f) * 0.25f;
        float d = fmaf(dhdz, dhdz, fmaf(dhdx, dhdx, 1.0f));
        float inv = 1.0f / sqrtf(d);
        nx = -dhdx * inv; ny = inv; nz = -dhdz * inv;
    } else {
        // SPEC_T32, as in fragment_shader_lit
        const float third = 1.0f / 3.0f;
        const float uu = fmaf(x, third, 0.5f), vv = fmaf(z, third, 0.5f);
        const float du = 1.0f / (float)(max(P.tw, 2u) - 1u), dv = 1.0f / (float)(max(P.th, 2u) - 1u);
        const int mx = (int)P.tw - 1, my = (int)P.th - 1;
        const int tx0 = min(max((int)floorf(uu * (float)P.tw), 0), mx), tx1 = min(max((int)floorf((uu + du) * (float)P.tw), 0), mx);
        const int ty0 = min(max((int)floorf(vv * (float)P.th), 0), my), ty1 = min(max((int)floorf((vv + dv) * (float)P.th), 0), my);
        const float h0 = P.tex[(size_t)ty0 * P.tw + tx0], hx = P.tex[(size_t)ty0 * P.tw + tx1], hy = P.tex[(size_t)ty1 * P.tw + tx0];
        const float ax = (hx - h0) * P.exag, az = (hy - h0) * P.exag, sp = P.spacing;
        const float vx = -(ax * sp), vy = sp * sp, vz = -(sp * az);
        const float d = fmaf(vz, vz, fmaf(vy, vy, vx * vx));
        const float inv = 1.0f / sqrtf(d);
        nx = vx * inv; ny = vy * inv; nz = vz * inv;
    }
    float ndl = fmaf(nz, P.Lz, fmaf(ny, P.Ly, nx * P.Lx));
    float lambert = fminf(fmaxf(ndl, 0.0f), 1.0f) * lit;
    float shade = (0.15f * (1.0f - lambert) + lambert) * amb;
    uint32_t out = 0xFF000000u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float l0 = S.lut[i0 * kLutStride + ch], l1 = S.lut[i1 * kLutStride + ch];
        float lc = fmaf(f, l1 - l0, l0);
        float alb = fmaf(opacity, val[ch], keep * lc);
        float v = alb * P.exposure * shade;
        if (P.shade_mode != 0u) v = v / (1.0f + v);          // Reinhard, before the sRGB store
        out |= srgb_encode(v, S.thresh) << (8 * ch);
    }
    return out;
}

// Pixel (px, py) with visibility id `id`: false when the image does not reach it or is transparent there (the pixel keeps the frame's
// bytes); else its colour with the mixed albedo.  lit, sky: the shadow and sky-view fields, NULL when the feature is off (the value
// is 1 then); three vertex values that are all 1 give 1 without interpolation, otherwise the interpolated value goes through
// fminf(., 1) -- sh_pixel's rules (vf_shadow.h).
template <bool CLIPPED>
__device__ __forceinline__ bool dr_pixel(const FrameParams &P, const SetupView &V, const ShadeTables &T, const float *dec, const DrapeParams &D,
                                         const uint32_t *__restrict__ img, const float *__restrict__ lit, const float *__restrict__ sky,
                                         float amb_strength, uint32_t id, int32_t px, int32_t py, uint32_t &rgba)
{
    const uint32_t prim = id - 1u;
    const VisibleSite s = visible_site<CLIPPED>(P, V, prim);
    const uint32_t i = s.i, j = s.j, odd = s.odd;
    float attr[3] = { 0.0f, 0.0f, 0.0f }, q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, rQ = 0.0f;
    GVert g[3];
    if constexpr (CLIPPED) {
        if (s.generic) {
            load_prim(P, V.hblk, prim, g[0], g[1], g[2]);
            (void)clipped_weights(g, P.hw, P.hh, P.W, P.H, px, py, attr);
        }
    }
    if (!s.generic) {
        const VertexRec r0 = V.vtx[s.r0], r1 = V.vtx[s.r1], r2 = V.vtx[s.r2];
        record_weights(r0, r1, r2, px, py, q0, q1, q2);
        rQ = 1.0f / ((q0 + q1) + q2);
        const float x0 = grid_coord(P, i + odd), x1 = grid_coord(P, i), x2 = grid_coord(P, i + 1u);
        const float z0 = grid_coord(P, j), z1 = grid_coord(P, j + 1u), z2 = grid_coord(P, j + odd);
        attr[0] = fmaf(q2, r2.h, fmaf(q1, r1.h, q0 * r0.h)) * rQ;
        attr[1] = fmaf(q2, x2, fmaf(q1, x1, q0 * x0)) * rQ;
        attr[2] = fmaf(q2, z2, fmaf(q1, z1, q0 * z0)) * rQ;
    }
    float val[4];
    if (!dr_sample(D, img, dec, attr[1], attr[2], val)) return false;
    const float Aop = val[3] * D.opacity;
    if (!(Aop > 0.0f)) return false;
    // vertex 0 = (i + odd, j), vertex 1 = (i, j + 1), vertex 2 = (i + 1, j + odd)
    const size_t v0 = (size_t)j * P.n + i + odd, v1 = (size_t)(j + 1u) * P.n + i, v2 = (size_t)(j + odd) * P.n + i + 1u;
    float l0 = 1.0f, l1 = 1.0f, l2 = 1.0f, a0 = 1.0f, a1 = 1.0f, a2 = 1.0f;
    if (lit != nullptr) { l0 = lit[v0]; l1 = lit[v1]; l2 = lit[v2]; }
    if (sky != nullptr) {
        a0 = 1.0f - amb_strength * (1.0f - sky[v0]);
        a1 = 1.0f - amb_strength * (1.0f - sky[v1]);
        a2 = 1.0f - amb_strength * (1.0f - sky[v2]);
    }
    const bool plain_l = l0 == 1.0f && l1 == 1.0f && l2 == 1.0f, plain_a = a0 == 1.0f && a1 == 1.0f && a2 == 1.0f;
    float v = 1.0f, w = 1.0f;
    if constexpr (CLIPPED) {
        if (s.generic) {
            // lit and amb ride through the clipper in the place of the height varying, as in sh_pixel
            float la[3];
            if (!plain_l) {
                g[0].a[0] = l0; g[1].a[0] = l1; g[2].a[0] = l2;
                (void)clipped_weights(g, P.hw, P.hh, P.W, P.H, px, py, la);
                v = fminf(la[0], 1.0f);
            }
            if (!plain_a) {
                g[0].a[0] = a0; g[1].a[0] = a1; g[2].a[0] = a2;
                (void)clipped_weights(g, P.hw, P.hh, P.W, P.H, px, py, la);
                w = fminf(la[0], 1.0f);
            }
        }
    }
    if (!s.generic) {
        if (!plain_l) v = fminf(fmaf(q2, l2, fmaf(q1, l1, q0 * l0)) * rQ, 1.0f);
        if (!plain_a) w = fminf(fmaf(q2, a2, fmaf(q1, a1, q0 * a0)) * rQ, 1.0f);
    }
    rgba = fragment_shader_drape(P, T, attr, v, w, val, D.opacity, 1.0f - Aop);
    return true;
}

// The frame's visibility (H, W) -> the pixels of its colour buffer the image covers, in the walk of for_each_visible (vf_visible.h).
// `redo` as in k_shadow_shade: both instantiations are launched behind a frame and the one it does not call for leaves at once.
template <bool CLIPPED>
__global__ __launch_bounds__(256) void k_drape_shade(FrameParams P, SetupView V, const float *__restrict__ lut_linear, const float *__restrict__ thresh,
                                                     const float *__restrict__ decode, const uint32_t *__restrict__ vis, DrapeParams D,
                                                     const uint32_t *__restrict__ img, const float *__restrict__ lit, const float *__restrict__ sky,
                                                     float strength, const uint32_t *__restrict__ redo, uint32_t *__restrict__ rgba)
{
    if ((*redo != 0u) != CLIPPED) return;
    __shared__ __attribute__((aligned(16))) float s_lut[kLutFloats];
    __shared__ float s_thr[256];
    __shared__ float s_dec[256];
    for (int k = threadIdx.x; k < kLutFloats; k += 256) s_lut[k] = lut_linear[k];
    s_thr[threadIdx.x] = thresh[threadIdx.x];
    s_dec[threadIdx.x] = decode[threadIdx.x];
    __syncthreads();
    const ShadeTables T = { s_lut, s_thr };
    for_each_visible(P, vis, [&](uint32_t id, uint32_t px, uint32_t py) {
        uint32_t c;
        if (id != 0u && dr_pixel<CLIPPED>(P, V, T, s_dec, D, img, lit, sky, strength, id, (int32_t)px, (int32_t)py, c)) rgba[(size_t)py * P.W + px] = c;
    });
}

} // namespace vf

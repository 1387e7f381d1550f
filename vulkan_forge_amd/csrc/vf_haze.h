// vf_haze.h -- atmospheric haze: a distance and height fog pass over a frame.
//
//   k_haze<CLIPPED, PLANE>   per pixel of the frame's stored visibility: the view depth d and the world height y of the surface point
//                            (the geometry buffers' depth and position.y), the opacity a = 1 - exp(-density l g) of
//                            the path l = d - start through air whose density falls off with height (g: its mean along the line of
//                            sight), and the haze colour blended over the pixel in linear light (vs_blend, vf_viewshed.h).
//                            PLANE = false rewrites the colour buffer; PLANE = true stores a into a float plane instead.
//
// Launched only for a handle with haze enabled, or for the opacity plane: the frame path is not touched.  The arithmetic is the
// contract's, bit for bit (tests/haze_model/haze_model.c is its CPU statement), always the exact path, whatever the shade precision.
// det_exp lives here, not in vf_device.h: the existing kernels keep their text.  Templates and inline functions only: the library's
// non-template kernels keep their places.
#pragma once
#include "vf_viewshed.h"

namespace vf {

// exp(x) for x in [-87, 16] (callers clamp: neither a subnormal nor an infinity arises), the same bits as the CPU model's: Cody-Waite
// reduction by n = rintf(x log2e) with ln 2 split in two (n ln2_hi is exact: nine significant bits times eight), exp(r) = 1 + (r + r^2 p(r))
// with p of degree 5 as an fmaf Horner chain, times 2^n built from bits.  Only correctly rounded operations: no expf, no hardware exp2.
__device__ __forceinline__ float det_exp(float x)
{
    const float n = rintf(x * 1.44269504088896341f);
    float r = fmaf(-n, 0.693359375f, x);
    r = fmaf(-n, -2.12194440e-4f, r);
    float p = fmaf(r, 1.9875691500e-4f, 1.3981999507e-3f);
    p = fmaf(r, p, 8.3334519073e-3f);
    p = fmaf(r, p, 4.1665795894e-2f);
    p = fmaf(r, p, 1.6666665459e-1f);
    p = fmaf(r, p, 5.0000001201e-1f);
    const float y = fmaf(r * r, p, r) + 1.0f;
    return y * __uint_as_float((uint32_t)((int32_t)n + 127) << 23);
}

struct HazeParams {
    const float *decode;        // 256 sRGB8 -> linear
    uint32_t rgba;              // the haze colour, r | g << 8 | b << 16 | a << 24
    float density, start;
    float falloff, base;        // falloff 0: uniform haze
    float max_opacity;
    float eye_y;                // y of the eye, from the frame's view matrix (the host forms it once per frame)
    uint32_t background;        // 1: pixels without terrain are blended with max_opacity
};

constexpr float kHazeSeriesBelow = 0.5f;

__device__ __forceinline__ float haze_clamp_k(float k) { return fminf(fmaxf(k, -16.0f), 64.0f); }

// the height factor g (contract item 3): the mean of exp(-(y - base) / falloff) from the eye's height to the point's
__device__ __forceinline__ float haze_g(const HazeParams &Z, float y)
{
    if (!(Z.falloff > 0.0f)) return 1.0f;
    const float k_e = haze_clamp_k((Z.eye_y - Z.base) / Z.falloff), k_p = haze_clamp_k((y - Z.base) / Z.falloff);
    const float s = k_p - k_e;
    const float E_e = det_exp(-k_e);
    if (fabsf(s) < kHazeSeriesBelow) {
        float t = fmaf(s, 2.7557319224e-6f, -2.4801587302e-5f);       // 1/9!, -1/8!
        t = fmaf(s, t, 1.9841269841e-4f);
        t = fmaf(s, t, -1.3888888889e-3f);
        t = fmaf(s, t, 8.3333333333e-3f);
        t = fmaf(s, t, -4.1666666667e-2f);
        t = fmaf(s, t, 1.6666666667e-1f);
        t = fmaf(s, t, -0.5f);
        t = fmaf(s, t, 1.0f);
        return E_e * t;
    }
    return (E_e - det_exp(-k_p)) / s;
}

// the opacity of a surface point at view depth d and height y (items 1, 2, 5); 0: the pass leaves the pixel
__device__ __forceinline__ float haze_alpha(const HazeParams &Z, float d, float y)
{
    if (!isfinite(d)) return 0.0f;
    const float l = fmaxf(d - Z.start, 0.0f);
    if (!(l > 0.0f)) return 0.0f;
    const float tau = (Z.density * l) * haze_g(Z, y);
    const float a0 = 1.0f - det_exp(-fminf(tau, 87.0f));
    const float a = fminf(a0, Z.max_opacity) * ((float)(Z.rgba >> 24) / 255.0f);
    return a > 0.0f ? a : 0.0f;
}

// d and y of pixel (px, py) with visibility id `id` != 0: the operations of gb_pixel (vf_gbuffer.h) on both of its paths
template <bool CLIPPED>
__device__ __forceinline__ void haze_point(const FrameParams &P, const SetupView &V, uint32_t id, int32_t px, int32_t py, float &d, float &y)
{
    const uint32_t prim = id - 1u;
    const VisibleSite s = visible_site<CLIPPED>(P, V, prim);
    if constexpr (CLIPPED) {
        if (s.generic) {
            GVert v[3];
            load_prim(P, V.hblk, prim, v[0], v[1], v[2]);
            float attr[3];
            const float Q = clipped_weights(v, P.hw, P.hh, P.W, P.H, px, py, attr);
            d = 1.0f / Q;
            y = attr[0] * P.exag;
            return;
        }
    }
    const VertexRec r0 = V.vtx[s.r0], r1 = V.vtx[s.r1], r2 = V.vtx[s.r2];
    float q0, q1, q2;
    record_weights(r0, r1, r2, px, py, q0, q1, q2);
    const float rQ = 1.0f / ((q0 + q1) + q2);
    d = rQ;
    y = (fmaf(q2, r2.h, fmaf(q1, r1.h, q0 * r0.h)) * rQ) * P.exag;
}

// The frame's visibility (H, W) -> its colour buffer under the haze (PLANE = false: `rgba`) or the opacity plane (PLANE = true:
// `plane`, every pixel of the frame written), in the walk of for_each_visible (vf_visible.h).  `redo` as for k_relight and
// k_viewshed_tint: both CLIPPED instantiations are launched behind a frame and the one the frame does not call for leaves at once.
template <bool CLIPPED, bool PLANE>
__global__ __launch_bounds__(256) void k_haze(FrameParams P, SetupView V, const float *__restrict__ thresh, const uint32_t *__restrict__ vis,
                                              HazeParams Z, const uint32_t *__restrict__ redo, uint32_t *__restrict__ rgba, float *__restrict__ plane)
{
    if ((*redo != 0u) != CLIPPED) return;
    __shared__ float s_thr[256];
    __shared__ float s_dec[256];
    if constexpr (!PLANE) {
        s_thr[threadIdx.x] = thresh[threadIdx.x];
        s_dec[threadIdx.x] = Z.decode[threadIdx.x];
        __syncthreads();
    }
    const float a_far = Z.background ? Z.max_opacity * ((float)(Z.rgba >> 24) / 255.0f) : 0.0f;      // item 7: a surface infinitely far away
    for_each_visible(P, vis, [&](uint32_t id, uint32_t px, uint32_t py) {
        const size_t o = (size_t)py * P.W + px;
        float a = a_far;
        if (id != 0u) {
            float d, y;
            haze_point<CLIPPED>(P, V, id, (int32_t)px, (int32_t)py, d, y);
            a = haze_alpha(Z, d, y);
        }
        if constexpr (PLANE) { plane[o] = a > 0.0f ? a : 0.0f; return; }
        else {
            if (!(a > 0.0f)) return;
            const uint32_t c0 = rgba[o];
            float c[3] = { s_dec[c0 & 255u], s_dec[(c0 >> 8) & 255u], s_dec[(c0 >> 16) & 255u] };
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = s_dec[(Z.rgba >> (8 * k)) & 255u] * a + c[k] * (1.0f - a);
            rgba[o] = srgb_encode(c[0], s_thr) | (srgb_encode(c[1], s_thr) << 8) | (srgb_encode(c[2], s_thr) << 16) | (id != 0u ? 0xFF000000u : c0 & 0xFF000000u);
        }
    });
}

} // namespace vf

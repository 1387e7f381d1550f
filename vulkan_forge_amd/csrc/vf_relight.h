// vf_relight.h -- the relight pass: one walk over a frame's stored visibility that writes pixels again through the
// exact fragment function, for the features that rewrite a frame behind the tile kernel.
//
//   kShadow    cast shadows (4g): the pixels whose interpolated lit is below 1, with lambert * lit
//   kAmbient   ambient occlusion, and cast shadows when they are on as well (4i): the pixels whose lit or amb is below 1, with
//              lambert * lit and shade * amb; amb = 1 - strength (1 - sky) per vertex
//   kDrape     the draped image (4j): the pixels where the image's sample at (x, z) is not transparent, with the colormap value
//              mixed with the sample; lit and amb are formed by the same rules, so the result does not depend on what the pass
//              before wrote
//   kDrapeMip  the draped image through its mip pyramid (4k): kDrape with the level of detail of the pixel's footprint on the image,
//              from the varyings of the same primitive one pixel to the right and one below
//   kDrapeAniso  kDrapeMip with up to A taps along the footprint's major axis, at the level of detail of the minor one (4p)
//
// The surface point, its varyings and the interpolation of a per-vertex scalar are vf_visible.h's.  The arithmetic is the
// contract's, bit for bit (tests/shadow_model, ambient_model, drape_model, drape_mip_model and drape_aniso_model are its CPU statements).  All kernels are templates
// (DESIGN.md 4d).
#pragma once
#include <type_traits>
#include "vf_drape_aniso.h"

namespace vf {

enum Relight : int { kShadow = 0, kAmbient = 1, kDrape = 2, kDrapeMip = 3, kDrapeAniso = 4 };
constexpr bool relight_mips(Relight pass) { return pass == kDrapeMip || pass == kDrapeAniso; }     // the passes that read the pyramid
constexpr bool relight_drapes(Relight pass) { return pass == kDrape || relight_mips(pass); }

// What a pass reads beside the frame.  lit / sky: the shadow and sky-view fields; kShadow reads lit alone, kAmbient takes sky for
// granted, and a field that is NULL otherwise belongs to a feature that is off (its value is 1).  The rest is the drape's.
struct RelightParams {
    const float *lit, *sky;
    float amb_strength;
    const float *decode;        // 256 sRGB8 -> linear
    const uint32_t *img;
    DrapeParams D;
};
// ... and kDrapeMip the pyramid beside it: the other passes keep their kernel arguments as they are
struct RelightMipParams : RelightParams { DrapeMips M; };
// ... and kDrapeAniso the largest anisotropy A and 1 / A^2 behind that
struct RelightAnisoParams : RelightMipParams { uint32_t max_aniso; float inv_a2; };
template <Relight PASS> using RelightArg = std::conditional_t<PASS == kDrapeAniso, RelightAnisoParams, std::conditional_t<PASS == kDrapeMip, RelightMipParams, RelightParams>>;

// lit and amb of a pixel.  At the three vertices first: a primitive whose three values are all 1 is `plain` and gives 1 without
// interpolation (x * (1 / x) need not round to 1).
struct LightTerms {
    float l[3], a[3];
    bool plain_l, plain_a;
};

template <Relight PASS>
__device__ __forceinline__ LightTerms vertex_light(const FrameParams &P, const VisibleSite &s, const RelightParams &R)
{
    const float *lit = R.lit, *sky = R.sky;
    const bool have_lit = PASS == kShadow || lit != nullptr, have_sky = PASS == kAmbient || (relight_drapes(PASS) && sky != nullptr);
    LightTerms L;
#pragma unroll
    for (int k = 0; k < 3; ++k) L.l[k] = have_lit ? lit[site_vertex(P, s, k)] : 1.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) L.a[k] = have_sky ? 1.0f - R.amb_strength * (1.0f - sky[site_vertex(P, s, k)]) : 1.0f;
    L.plain_l = L.l[0] == 1.0f && L.l[1] == 1.0f && L.l[2] == 1.0f;
    L.plain_a = L.a[0] == 1.0f && L.a[1] == 1.0f && L.a[2] == 1.0f;
    return L;
}

// ... then at the point (vf_visible.h).  kShadow hands lit on as it is (the pass leaves unless it is below 1); the others shade
// an interpolated value an ulp above 1 as 1.
template <bool CLIPPED, Relight PASS>
__device__ __forceinline__ void point_light(const FrameParams &P, const VisiblePoint<CLIPPED> &p, int32_t px, int32_t py, const LightTerms &L,
                                            float &lit, float &amb)
{
    lit = L.plain_l ? 1.0f : point_scalar(P, p, px, py, L.l[0], L.l[1], L.l[2]);
    amb = L.plain_a ? 1.0f : point_scalar(P, p, px, py, L.a[0], L.a[1], L.a[2]);
    if constexpr (PASS != kShadow) { lit = fminf(lit, 1.0f); amb = fminf(amb, 1.0f); }
}

// Pixel (px, py) with visibility id `id`: false when the pass leaves it as the frame drew it, else its colour again.  Each pass
// leaves before it computes what it does not need: kShadow and kAmbient on the vertex values alone, then on the interpolated ones,
// and form the varyings last; kDrape needs (x, z) for its sample and touches the fields only where the image shows; kDrapeMip
// evaluates the neighbouring centres only for a pixel inside the image's extent, and kDrapeAniso follows it with its plan between
// the neighbours and the sample.
template <bool CLIPPED, Relight PASS>
__device__ __forceinline__ bool relight_pixel(const FrameParams &P, const SetupView &V, const ShadeTables &T, const float *dec, const RelightArg<PASS> &R,
                                              uint32_t id, int32_t px, int32_t py, uint32_t &rgba)
{
    const uint32_t prim = id - 1u;
    const VisibleSite s = visible_site<CLIPPED>(P, V, prim);
    LightTerms L;
    if constexpr (!relight_drapes(PASS)) {
        L = vertex_light<PASS>(P, s, R);
        if (L.plain_l && L.plain_a) return false;
    }
    const VisiblePoint<CLIPPED> p = visible_point<CLIPPED>(P, V, s, prim, px, py);
    float attr[3], lit, amb;
    if constexpr (relight_drapes(PASS)) {
        point_varyings(P, p, px, py, attr);
        float val[4];
        if constexpr (PASS == kDrapeMip) {
            const float fu = (attr[1] - R.D.x0) * R.D.sx, fv = (attr[2] - R.D.z0) * R.D.sz;
            if (!(fu >= 0.0f && fu <= (float)R.D.iw && fv >= 0.0f && fv <= (float)R.D.ih)) return false;
            float right[3], down[3];
            point_neighbours(P, p, px, py, right, down);
            const float lod = mip_lod(R.D, R.M.bias, attr[1], attr[2], right[1], right[2], down[1], down[2]);
            if (!mip_sample(R.D, R.M, R.img, dec, attr[1], attr[2], lod, val)) return false;
        } else if constexpr (PASS == kDrapeAniso) {
            const float fu = (attr[1] - R.D.x0) * R.D.sx, fv = (attr[2] - R.D.z0) * R.D.sz;
            if (!(fu >= 0.0f && fu <= (float)R.D.iw && fv >= 0.0f && fv <= (float)R.D.ih)) return false;
            float right[3], down[3];
            point_neighbours(P, p, px, py, right, down);
            const AnisoPlan a = aniso_plan(R.D, R.M.bias, R.max_aniso, R.inv_a2, attr[1], attr[2], right[1], right[2], down[1], down[2]);
            if (a.n == 1u) { if (!mip_sample(R.D, R.M, R.img, dec, attr[1], attr[2], a.lod, val)) return false; }
            else aniso_sample(R.D, R.M, R.img, dec, fu, fv, a, val);
        } else {
            if (!dr_sample(R.D, R.img, dec, attr[1], attr[2], val)) return false;
        }
        const float Aop = val[3] * R.D.opacity;
        if (!(Aop > 0.0f)) return false;
        L = vertex_light<PASS>(P, s, R);
        point_light<CLIPPED, PASS>(P, p, px, py, L, lit, amb);
        rgba = fragment_shader_albedo<true>(P, T, attr, lit, amb, val, R.D.opacity, 1.0f - Aop);
    } else {
        point_light<CLIPPED, PASS>(P, p, px, py, L, lit, amb);
        if (!(lit < 1.0f) && !(amb < 1.0f)) return false;
        point_varyings(P, p, px, py, attr);
        rgba = fragment_shader_lit(P, T, attr, lit, PASS == kShadow ? 1.0f : amb);
    }
    return true;
}

// The frame's visibility (H, W) -> the pixels of its colour buffer the pass writes again, in the walk of for_each_visible
// (vf_visible.h).  `redo` is the frame's count of work items that met a clipped or oversized primitive: both instantiations are
// launched behind a frame and the one the frame does not call for leaves at once (no host round trip between the frame and the pass).
template <bool CLIPPED, Relight PASS>
__global__ __launch_bounds__(256) void k_relight(FrameParams P, SetupView V, const float *__restrict__ lut_linear, const float *__restrict__ thresh,
                                                 const uint32_t *__restrict__ vis, RelightArg<PASS> R, const uint32_t *__restrict__ redo,
                                                 uint32_t *__restrict__ rgba)
{
    if ((*redo != 0u) != CLIPPED) return;
    __shared__ __attribute__((aligned(16))) float s_lut[kLutFloats];
    __shared__ float s_thr[256];
    for (int k = threadIdx.x; k < kLutFloats; k += 256) s_lut[k] = lut_linear[k];
    s_thr[threadIdx.x] = thresh[threadIdx.x];
    const float *dec = nullptr;
    if constexpr (relight_drapes(PASS)) {
        __shared__ float s_dec[256];
        s_dec[threadIdx.x] = R.decode[threadIdx.x];
        dec = s_dec;
    }
    __syncthreads();
    const ShadeTables T = { s_lut, s_thr };
    for_each_visible(P, vis, [&](uint32_t id, uint32_t px, uint32_t py) {
        uint32_t c;
        if (id != 0u && relight_pixel<CLIPPED, PASS>(P, V, T, dec, R, id, (int32_t)px, (int32_t)py, c)) rgba[(size_t)py * P.W + px] = c;
    });
}

} // namespace vf

// vf_gbuffer.h -- geometry buffers of a frame: per pixel the view depth, the world position, the geometric normal
// and the visibility id of the surface, from the frame's stored visibility (H, W) u32 and its set-up arrays.  A pass of its own,
// launched only when a caller asks (vf_terrain_gbuffer_device / _read_gbuffer / _pick): the frame path is not touched.
//
// The arithmetic is the contract's, bit for bit (tests/gbuffer_model/gbuffer_model.c is its CPU statement): the lookup, the
// perspective weights and the clipped walk of vf_visible.h, always the exact path, whatever the shade precision.  Both kernels are
// templates: the library's non-template kernels keep their places.
#pragma once
#include "vf_visible.h"

namespace vf {

// one pixel's eight words, as k_gbuffer_pick stores them
struct GbPixel { float depth, x, y, z, nx, ny, nz; uint32_t id; };
static_assert(sizeof(GbPixel) == 32, "a pick record is two 16-byte words");

// destinations of k_gbuffer; a NULL plane is neither computed nor stored
struct GbPlanes { float *depth, *position, *normal; uint32_t *primitive; };

// unit normal of the triangle P0 P1 P2 (world space), pointing up; (0, 0, 0) when it has no finite length
__device__ __forceinline__ void gb_normal(const float P0[3], const float P1[3], const float P2[3], float n[3])
{
    const float ax = P1[0] - P0[0], ay = P1[1] - P0[1], az = P1[2] - P0[2];
    const float bx = P2[0] - P0[0], by = P2[1] - P0[1], bz = P2[2] - P0[2];
    float nx = fmaf(ay, bz, -(az * by)), ny = fmaf(az, bx, -(ax * bz)), nz = fmaf(ax, by, -(ay * bx));
    if (ny < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    const float len = sqrtf(fmaf(nz, nz, fmaf(ny, ny, nx * nx)));
    const bool ok = len > 0.0f && isfinite(len);
    n[0] = ok ? nx / len : 0.0f; n[1] = ok ? ny / len : 0.0f; n[2] = ok ? nz / len : 0.0f;
}

// The eight words of pixel (px, py) with visibility id `id`.  want_pos / want_nrm (uniform across a launch): position and normal
// are left at zero when the caller stores neither.
template <bool CLIPPED>
__device__ __forceinline__ GbPixel gb_pixel(const FrameParams &P, const SetupView &V, uint32_t id, int32_t px, int32_t py, bool want_pos, bool want_nrm)
{
    GbPixel g = { __builtin_inff(), 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, id };
    if (id == 0u) return g;
    const uint32_t prim = id - 1u;
    const VisibleSite s = visible_site<CLIPPED>(P, V, prim);
    const uint32_t i = s.i, j = s.j, odd = s.odd;
    float n[3];
    if constexpr (CLIPPED) {
        if (s.generic) {
            GVert v[3];
            load_prim(P, V.hblk, prim, v[0], v[1], v[2]);
            float attr[3];
            const float Q = clipped_weights(v, P.hw, P.hh, P.W, P.H, px, py, attr);
            g.depth = 1.0f / Q;
            g.x = attr[1] * P.spacing; g.y = attr[0] * P.exag; g.z = attr[2] * P.spacing;
            if (want_nrm) {
                float W3[3][3];
                for (int k = 0; k < 3; ++k) { W3[k][0] = v[k].a[1] * P.spacing; W3[k][1] = v[k].a[0] * P.exag; W3[k][2] = v[k].a[2] * P.spacing; }
                gb_normal(W3[0], W3[1], W3[2], n);
                g.nx = n[0]; g.ny = n[1]; g.nz = n[2];
            }
            return g;
        }
    }
    const VertexRec r0 = V.vtx[s.r0], r1 = V.vtx[s.r1], r2 = V.vtx[s.r2];
    float q0, q1, q2;
    record_weights(r0, r1, r2, px, py, q0, q1, q2);
    const float rQ = 1.0f / ((q0 + q1) + q2);
    g.depth = rQ;
    if (want_pos || want_nrm) {
        // varyings xz (terrain.wgsl:64): vertex 0 = (i + odd, j), vertex 1 = (i, j + 1), vertex 2 = (i + 1, j + odd)
        const float x0 = grid_coord(P, i + odd), x1 = grid_coord(P, i), x2 = grid_coord(P, i + 1u);
        const float z0 = grid_coord(P, j), z1 = grid_coord(P, j + 1u), z2 = grid_coord(P, j + odd);
        if (want_pos) {
            const float h = fmaf(q2, r2.h, fmaf(q1, r1.h, q0 * r0.h)) * rQ;
            const float x = fmaf(q2, x2, fmaf(q1, x1, q0 * x0)) * rQ;
            const float z = fmaf(q2, z2, fmaf(q1, z1, q0 * z0)) * rQ;
            g.x = x * P.spacing; g.y = h * P.exag; g.z = z * P.spacing;
        }
        if (want_nrm) {
            const float P0[3] = { x0 * P.spacing, r0.h * P.exag, z0 * P.spacing }, P1[3] = { x1 * P.spacing, r1.h * P.exag, z1 * P.spacing };
            const float P2[3] = { x2 * P.spacing, r2.h * P.exag, z2 * P.spacing };
            gb_normal(P0, P1, P2, n);
            g.nx = n[0]; g.ny = n[1]; g.nz = n[2];
        }
    }
    return g;
}

// Visibility (H, W) u32 -> the requested planes, in the walk of for_each_visible (vf_visible.h).  CLIPPED = false (the frame held no
// generic primitive): no clipper, no scratch.
template <bool CLIPPED>
__global__ __launch_bounds__(256) void k_gbuffer(FrameParams P, SetupView V, const uint32_t *__restrict__ vis, GbPlanes O)
{
    const bool want_pos = O.position != nullptr, want_nrm = O.normal != nullptr;
    for_each_visible(P, vis, [&](uint32_t id, uint32_t px, uint32_t py) {
        const GbPixel g = gb_pixel<CLIPPED>(P, V, id, (int32_t)px, (int32_t)py, want_pos, want_nrm);
        const size_t o = (size_t)py * P.W + px;
        if (O.depth) O.depth[o] = g.depth;
        if (want_pos) { float *p = O.position + 3u * o; p[0] = g.x; p[1] = g.y; p[2] = g.z; }
        if (want_nrm) { float *p = O.normal + 3u * o; p[0] = g.nx; p[1] = g.ny; p[2] = g.nz; }
        if (O.primitive) O.primitive[o] = id;
    });
}

// "what is under these pixels": the same per-pixel function for a list of n pixels (x, y), all inside the frame (the host checks),
// one 32-byte record each
template <bool CLIPPED>
__global__ __launch_bounds__(256) void k_gbuffer_pick(FrameParams P, SetupView V, const uint32_t *__restrict__ vis, const int2 *__restrict__ pixels,
                                                      uint32_t n, GbPixel *__restrict__ out)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const int2 p = pixels[k];
    if (p.x < 0 || p.y < 0 || (uint32_t)p.x >= P.W || (uint32_t)p.y >= P.H) return;     // (never: vf_terrain_pick refuses such a list)
    out[k] = gb_pixel<CLIPPED>(P, V, vis[(size_t)p.y * P.W + (size_t)p.x], p.x, p.y, true, true);
}

} // namespace vf

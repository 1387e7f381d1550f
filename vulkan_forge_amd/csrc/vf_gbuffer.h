// vf_gbuffer.h -- geometry buffers of a frame: per pixel the view depth, the world position, the geometric normal
// and the visibility id of the surface, from the frame's stored visibility (H, W) u32 and its set-up arrays.  A pass of its own,
// launched only when a caller asks (vf_terrain_gbuffer_device / _read_gbuffer / _pick): the frame path is not touched.
//
// The arithmetic is the contract's, bit for bit (tests/gbuffer_model/gbuffer_model.c is its CPU statement): the perspective weights
// of shade_from_records / terrain_rw (ordinary primitives) and of interpolate() on the sub-triangle clipped_attributes picks
// (generic ones), always the exact path, whatever the shade precision.  Both kernels are templates: the library's non-template
// kernels keep their places and every kernel of the frame path stays instruction-identical.
#pragma once
#include "vf_kernels.h"

namespace vf {

// one pixel's eight words, as k_gbuffer_pick stores them
struct GbPixel { float depth, x, y, z, nx, ny, nz; uint32_t id; };
static_assert(sizeof(GbPixel) == 32, "a pick record is two 16-byte words");

// destinations of k_gbuffer; a NULL plane is neither computed nor stored
struct GbPlanes { float *depth, *position, *normal; uint32_t *primitive; };

// perspective weights q_i = lambda_i rw_i of an ordinary primitive at the pixel centre from its three vertex records: the
// arithmetic of shade_from_records / terrain_rw (FP64 edge functions on integers below 2^25: exact)
__device__ __forceinline__ void gb_record_weights(const VertexRec &r0, const VertexRec &r1, const VertexRec &r2, int32_t px, int32_t py,
                                                  float &q0, float &q1, float &q2)
{
    const double Px = (double)(px * 256 + 128), Py = (double)(py * 256 + 128);
    const double X0 = r0.X, Y0 = r0.Y, X1 = r1.X, Y1 = r1.Y, X2 = r2.X, Y2 = r2.Y;
    const double e0 = -fma(X2 - X1, Py - Y1, -((Y2 - Y1) * (Px - X1)));
    const double e1 = -fma(X0 - X2, Py - Y2, -((Y0 - Y2) * (Px - X2)));
    const double e2 = -fma(X1 - X0, Py - Y0, -((Y1 - Y0) * (Px - X0)));
    const double area2 = fma(X1 - X0, Y2 - Y0, -((Y1 - Y0) * (X2 - X0)));
    const float fA = (float)(-area2);
    const float la0 = (float)e0 / fA, la1 = (float)e1 / fA, la2 = (float)e2 / fA;
    q0 = la0 * r0.rw; q1 = la1 * r1.rw; q2 = la2 * r2.rw;
}

// the generic path: clip, fan, the last piece that covers the pixel centre (as clipped_attributes) -> Q and the varyings (h, x, z);
// Q = 0 and zero varyings when no piece covers it (unreachable when the visibility is consistent)
__device__ __forceinline__ float gb_clipped(const GVert v[3], float hw, float hh, uint32_t W, uint32_t H, int32_t px, int32_t py, float attr[3])
{
    GVert poly[8];
    const int np = clip_primitive(v, poly);
    float Q = 0.0f;
    attr[0] = attr[1] = attr[2] = 0.0f;
    for (int f = 1; f + 1 < np; ++f) {
        TriSetup T;
        int64_t e[3];
        if (setup_triangle(poly[0], poly[f], poly[f + 1], hw, hh, W, H, T) && covers(T, px, py, e)) {
            const float fA = (float)(-T.area2);
            const float l0 = (float)e[0] / fA, l1 = (float)e[1] / fA, l2 = (float)e[2] / fA;
            const float q0 = l0 * T.s[0].rw, q1 = l1 * T.s[1].rw, q2 = l2 * T.s[2].rw;
            Q = (q0 + q1) + q2;
            const float rQ = 1.0f / Q;
            for (int k = 0; k < 3; ++k) attr[k] = fmaf(q2, T.s[2].a[k], fmaf(q1, T.s[1].a[k], q0 * T.s[0].a[k])) * rQ;
        }
    }
    return Q;
}

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
__device__ inline GbPixel gb_pixel(const FrameParams &P, const SetupView &V, uint32_t id, int32_t px, int32_t py, bool want_pos, bool want_nrm)
{
    GbPixel g = { __builtin_inff(), 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, id };
    if (id == 0u) return g;
    const uint32_t prim = id - 1u, cell = prim >> 1, odd = prim & 1u;
    const uint32_t j = cell_row(P, cell), i = cell - j * P.nm1;
    const uint32_t li = i & 7u, lj = j & 7u;
    const size_t b = (size_t)(j >> 3) * P.nb + (i >> 3);
    float n[3];
    if constexpr (CLIPPED) {
        if (V.recs[b].flags & kRecGeneric) {
            const ulonglong2 gen = V.gen[b];
            if (((odd ? gen.y : gen.x) >> (lj * 8u + li)) & 1ull) {
                GVert v[3];
                load_prim(P, V.hblk, prim, v[0], v[1], v[2]);
                float attr[3];
                const float Q = gb_clipped(v, P.hw, P.hh, P.W, P.H, px, py, attr);
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
    }
    const uint32_t va = lj * kBlockVerts + li;
    const uint32_t l0 = odd ? va + 1u : va, l1 = va + kBlockVerts, l2 = odd ? va + kBlockVerts + 1u : va + 1u;
    const size_t base = b * kBlockStride;
    const VertexRec r0 = V.vtx[base + l0], r1 = V.vtx[base + l1], r2 = V.vtx[base + l2];
    float q0, q1, q2;
    gb_record_weights(r0, r1, r2, px, py, q0, q1, q2);
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

// Visibility (H, W) u32 -> the requested planes.  The shape of k_resolve, for its reasons (vf_kernels.h): what bounds such a pass is
// the L1's handling of the three 16-byte record gathers per pixel, so a wave takes an 8 x 8 pixel tile (four side by side per
// workgroup: every row segment of the 32 x 8 region is one whole 128-byte line of visibility words), the regions are dealt to
// persistent workgroups so that each XCD owns a band of region columns (RegionWalk), and the next region's visibility word is
// requested before the current one is worked on.  CLIPPED = false (the frame held no generic primitive): no clipper, no scratch.
template <bool CLIPPED>
__global__ __launch_bounds__(256) void k_gbuffer(FrameParams P, SetupView V, const uint32_t *__restrict__ vis, GbPlanes O)
{
    const uint32_t lx = (threadIdx.x >> 6) * 8u + (threadIdx.x & 7u), ly = (threadIdx.x >> 3) & 7u;
    const bool want_pos = O.position != nullptr, want_nrm = O.normal != nullptr;
    RegionWalk R;
    R.init((P.W + 31u) / 32u, (P.H + 7u) / 8u);
    auto fetch = [&](uint32_t kk) -> uint32_t {
        uint32_t rx, ry;
        R.at(kk, rx, ry);
        const uint32_t px = rx * 32u + lx, py = ry * 8u + ly;
        return px < P.W && py < P.H ? vis[(size_t)py * P.W + px] : 0u;
    };
    uint32_t id_next = R.valid() ? fetch(R.k) : 0u;
    while (R.valid()) {
        const uint32_t id = id_next;
        const uint32_t kn = R.k + R.stride;
        if (kn < R.total) id_next = fetch(kn);
        uint32_t rx, ry;
        R.at(R.k, rx, ry);
        const uint32_t px = rx * 32u + lx, py = ry * 8u + ly;
        if (px < P.W && py < P.H) {
            const GbPixel g = gb_pixel<CLIPPED>(P, V, id, (int32_t)px, (int32_t)py, want_pos, want_nrm);
            const size_t o = (size_t)py * P.W + px;
            if (O.depth) O.depth[o] = g.depth;
            if (want_pos) { float *p = O.position + 3u * o; p[0] = g.x; p[1] = g.y; p[2] = g.z; }
            if (want_nrm) { float *p = O.normal + 3u * o; p[0] = g.nx; p[1] = g.ny; p[2] = g.nz; }
            if (O.primitive) O.primitive[o] = id;
        }
        R.k = kn;
    }
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

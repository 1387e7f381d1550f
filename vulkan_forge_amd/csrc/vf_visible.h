// vf_visible.h -- from a stored visibility id back to the surface at the pixel centre: which primitive, which three vertex records,
// which perspective weights.  The one statement of that lookup for every pass that reads a frame's stored visibility (H, W) u32
// behind the frame: overlay occlusion (terrain_rw), the geometry buffers (vf_gbuffer.h, 4f) and the relight pass
// (vf_relight.h, 4h).  The fused fragment stage (shade_pixel / shade_from_records / clipped_attributes / k_resolve*, vf_kernels.h)
// keeps its own text of the same arithmetic, for the reason given above shade_from_records.
//
// The arithmetic is the contract's, bit for bit (the CPU models under tests/*_model restate it): always the exact path, whatever
// the shade precision.  Inline functions and templates only: the library's kernels keep their places.
#pragma once
#include "vf_kernels.h"

namespace vf {

// Where primitive `prim` lives in the frame's set-up arrays
struct VisibleSite {
    uint32_t i, j, odd;         // grid cell (i, j); indices [a,c,b, b,c,d] (src/terrain/mod.rs:578-582): even = (a, c, b), odd = (b, c, d)
    size_t b;                   // its 8 x 8 block
    size_t r0, r1, r2;          // its vertex records in SetupView::vtx: vertex 0 = (i + odd, j), vertex 1 = (i, j + 1), vertex 2 = (i + 1, j + odd)
    bool generic;               // near / far clipped or oversized: the clipper's path (always false when CLIPPED is)
};

// CLIPPED = false: the frame held no generic primitive, so the block flags are not read and the callers' clipping code is not compiled in
template <bool CLIPPED>
__device__ __forceinline__ VisibleSite visible_site(const FrameParams &P, const SetupView &V, uint32_t prim)
{
    VisibleSite s;
    const uint32_t cell = prim >> 1;
    s.odd = prim & 1u;
    s.j = cell_row(P, cell); s.i = cell - s.j * P.nm1;
    const uint32_t li = s.i & 7u, lj = s.j & 7u;
    s.b = (size_t)(s.j >> 3) * P.nb + (s.i >> 3);
    s.generic = false;
    if constexpr (CLIPPED) {
        if (V.recs[s.b].flags & kRecGeneric) {
            const ulonglong2 g = V.gen[s.b];
            s.generic = ((s.odd ? g.y : g.x) >> (lj * 8u + li)) & 1ull;
        }
    }
    const uint32_t va = lj * kBlockVerts + li;
    const size_t base = s.b * kBlockStride;
    s.r0 = base + (s.odd ? va + 1u : va); s.r1 = base + (va + kBlockVerts); s.r2 = base + (s.odd ? va + kBlockVerts + 1u : va + 1u);
    return s;
}

// Perspective weights q_i = lambda_i rw_i of an ordinary primitive at the pixel centre from its three vertex records: inside-positive
// edge weights (covers() / edge_fn() in int64, here exactly the same values in FP64: operands are integers below 2^25, every product
// and sum stays below 2^53), lambda_i = e_i / -area2 in float as interpolate() forms them.  Q = (q0 + q1) + q2 is the interpolated 1/w.
__device__ __forceinline__ void record_weights(const VertexRec &r0, const VertexRec &r1, const VertexRec &r2, int32_t px, int32_t py,
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

// The generic path: clip, fan, the last piece that covers the pixel centre wins (as clipped_attributes, as in the draw order) -> its Q
// and the varyings (h, x, z); Q = 0 and zero varyings when no piece covers it (unreachable when the visibility is consistent; such a
// pixel hides nothing).  Inlined into its callers on purpose: a __noinline__ version changed clipped_attributes and moved the
// PC-relative calls in k_tile.
__device__ __forceinline__ float clipped_weights(const GVert v[3], float hw, float hh, uint32_t W, uint32_t H, int32_t px, int32_t py, float attr[3])
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

// The three field indices of a site: where a per-vertex field (n x n, row-major) holds vertex k = 0, 1, 2 of its primitive
__device__ __forceinline__ size_t site_vertex(const FrameParams &P, const VisibleSite &s, int k)
{
    const uint32_t dj = k == 1 ? 1u : k == 2 ? s.odd : 0u, di = k == 0 ? s.odd : k == 2 ? 1u : 0u;
    return (size_t)(s.j + dj) * P.n + s.i + di;
}

// The surface point of a visible pixel: what is loaded once per pixel, for point_varyings and point_scalar below.
// A pass that can leave on its site alone (site_vertex) does so before it asks for the point.
template <bool CLIPPED>
struct VisiblePoint {
    VisibleSite s;
    VertexRec r0, r1, r2;       // the record path: the three records, q_i = lambda_i rw_i and 1 / Q
    float q0, q1, q2, rQ;
    GVert g[CLIPPED ? 3 : 1];   // the generic path (CLIPPED only): the primitive as load_prim gives it
};

template <bool CLIPPED>
__device__ __forceinline__ VisiblePoint<CLIPPED> visible_point(const FrameParams &P, const SetupView &V, const VisibleSite &s, uint32_t prim,
                                                               int32_t px, int32_t py)
{
    VisiblePoint<CLIPPED> p;
    p.s = s;
    p.q0 = p.q1 = p.q2 = p.rQ = 0.0f;
    if constexpr (CLIPPED) {
        if (s.generic) { load_prim(P, V.hblk, prim, p.g[0], p.g[1], p.g[2]); return p; }
    }
    p.r0 = V.vtx[s.r0]; p.r1 = V.vtx[s.r1]; p.r2 = V.vtx[s.r2];
    record_weights(p.r0, p.r1, p.r2, px, py, p.q0, p.q1, p.q2);
    p.rQ = 1.0f / ((p.q0 + p.q1) + p.q2);
    return p;
}

// One per-vertex scalar (f0, f1, f2 at vertex 0, 1, 2) interpolated at the point.  On the generic path it rides through the clipper
// in the place of the height varying: the same crossings, the same piece.
template <bool CLIPPED>
__device__ __forceinline__ float point_scalar(const FrameParams &P, const VisiblePoint<CLIPPED> &p, int32_t px, int32_t py, float f0, float f1, float f2)
{
    if constexpr (CLIPPED) {
        if (p.s.generic) {
            GVert g[3] = { p.g[0], p.g[1], p.g[2] };
            g[0].a[0] = f0; g[1].a[0] = f1; g[2].a[0] = f2;
            float attr[3];
            (void)clipped_weights(g, P.hw, P.hh, P.W, P.H, px, py, attr);
            return attr[0];
        }
    }
    return fmaf(p.q2, f2, fmaf(p.q1, f1, p.q0 * f0)) * p.rQ;
}

// The varyings (h, x, z) at the point: vertex 0 = (i + odd, j), vertex 1 = (i, j + 1), vertex 2 = (i + 1, j + odd)
template <bool CLIPPED>
__device__ __forceinline__ void point_varyings(const FrameParams &P, const VisiblePoint<CLIPPED> &p, int32_t px, int32_t py, float attr[3])
{
    if constexpr (CLIPPED) {
        if (p.s.generic) { (void)clipped_weights(p.g, P.hw, P.hh, P.W, P.H, px, py, attr); return; }
    }
    const uint32_t i = p.s.i, j = p.s.j, odd = p.s.odd;
    attr[0] = point_scalar(P, p, px, py, p.r0.h, p.r1.h, p.r2.h);
    attr[1] = point_scalar(P, p, px, py, grid_coord(P, i + odd), grid_coord(P, i), grid_coord(P, i + 1u));
    attr[2] = point_scalar(P, p, px, py, grid_coord(P, j), grid_coord(P, j + 1u), grid_coord(P, j + odd));
}

// The generic path of point_neighbours below: the piece of the clipped fan that covers (px, py) -- the last one, as in
// clipped_weights -- evaluated at the centres of (px + 1, py) and (px, py + 1) as well: its edge values there through the same int64
// edge function, with no cover test (the piece's plane goes on outside the piece and outside the frame).  Zero varyings when no piece
// covers (px, py).
__device__ __forceinline__ void clipped_neighbours(const GVert v[3], float hw, float hh, uint32_t W, uint32_t H, int32_t px, int32_t py,
                                                   float right[3], float down[3])
{
    GVert poly[8];
    const int np = clip_primitive(v, poly);
    right[0] = right[1] = right[2] = down[0] = down[1] = down[2] = 0.0f;
    for (int f = 1; f + 1 < np; ++f) {
        TriSetup T;
        int64_t e[3];
        if (setup_triangle(poly[0], poly[f], poly[f + 1], hw, hh, W, H, T) && covers(T, px, py, e)) {
            (void)covers(T, px + 1, py, e); interpolate(T, e, right);
            (void)covers(T, px, py + 1, e); interpolate(T, e, down);
        }
    }
}

// The varyings (h, x, z) of the point's primitive at the centres of the pixel to the right and the pixel below: the
// same records and edge functions one pixel on, wherever that centre lies.  What a footprint on the surface is measured from.
template <bool CLIPPED>
__device__ __forceinline__ void point_neighbours(const FrameParams &P, const VisiblePoint<CLIPPED> &p, int32_t px, int32_t py, float right[3], float down[3])
{
    if constexpr (CLIPPED) {
        if (p.s.generic) { clipped_neighbours(p.g, P.hw, P.hh, P.W, P.H, px, py, right, down); return; }
    }
    VisiblePoint<CLIPPED> n = p;
    record_weights(p.r0, p.r1, p.r2, px + 1, py, n.q0, n.q1, n.q2);
    n.rQ = 1.0f / ((n.q0 + n.q1) + n.q2);
    point_varyings(P, n, px + 1, py, right);
    record_weights(p.r0, p.r1, p.r2, px, py + 1, n.q0, n.q1, n.q2);
    n.rQ = 1.0f / ((n.q0 + n.q1) + n.q2);
    point_varyings(P, n, px, py + 1, down);
}

// Terrain depth at a pixel, for overlay occlusion: Q of the visible primitive `prim`, its interpolated 1/w at the pixel centre
__device__ inline float terrain_rw(const FrameParams &P, const SetupView &V, uint32_t prim, int32_t px, int32_t py)
{
    const VisibleSite s = visible_site<true>(P, V, prim);
    if (s.generic) {
        GVert v[3];
        load_prim(P, V.hblk, prim, v[0], v[1], v[2]);
        float attr[3];
        return clipped_weights(v, P.hw, P.hh, P.W, P.H, px, py, attr);
    }
    const VertexRec r0 = V.vtx[s.r0], r1 = V.vtx[s.r1], r2 = V.vtx[s.r2];
    float q0, q1, q2;
    record_weights(r0, r1, r2, px, py, q0, q1, q2);
    return (q0 + q1) + q2;
}

// The walk of a pass over the stored visibility, in k_resolve's shape and for its reasons (vf_kernels.h): what bounds such a pass is
// the L1's handling of the three 16-byte record gathers per pixel, so a wave takes an 8 x 8 pixel tile (four side by side per
// 256-thread workgroup: every row segment of the 32 x 8 region is one whole 128-byte line of visibility words), the regions are dealt
// to persistent workgroups so that each XCD owns a band of region columns (RegionWalk), and the next region's visibility word is
// requested before the current one is worked on.  pixel(id, px, py) is called for this lane's pixel of every region, where it lies
// inside the frame.  k_resolve keeps its own loop: it counts covered pixels with a wave ballot per region beside the in-frame test,
// and on this walk (the ballot inside the callable) all four instantiations compiled to other code, 7 to 20 instructions more; it
// stays instruction-identical instead.  k_resolve4 walks 32 x 32 regions of 16-byte words, a different loop.
template <typename F>
__device__ __forceinline__ void for_each_visible(const FrameParams &P, const uint32_t *__restrict__ vis, F &&pixel)
{
    // lane -> pixel of the workgroup's 32 x 8 region: wave w holds the 8 x 8 tile at x = 8 w
    const uint32_t lx = (threadIdx.x >> 6) * 8u + (threadIdx.x & 7u), ly = (threadIdx.x >> 3) & 7u;
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
        if (px < P.W && py < P.H) pixel(id, px, py);
        R.k = kn;
    }
}

} // namespace vf

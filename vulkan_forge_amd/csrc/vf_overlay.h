// vf_overlay.h -- point and polyline overlays composited over the terrain frame (DESIGN.md "Overlays").
//
// Every overlay feature is cut into primitives when it is added (host, vf_hip.hip): a point is one circle or square, a polyline is
// its butt segments plus a disc (a circle of radius width/2) at every interior vertex and, for round caps, at both ends.  The
// primitives of all layers lie in ONE array in feature order (layers in insertion order, features in input order, a feature's
// primitives next to each other), so "feature order" is "primitive index order".  Per frame, on the draw stream behind the tile kernel:
//   k_ov_setup      one thread per primitive: drape, vertex transform, near / far clipping, viewport, exact screen geometry,
//                   a conservative pixel box, and one count per 16x16 screen bin the box reaches
//   k_ov_scan       one workgroup: exclusive scan of the bin counts -> each bin's slice of the pair list (and the total, for the host)
//   k_ov_scatter    one thread per primitive: its index into the slice of every bin its box reaches (atomic slots: any order)
//   k_ov_composite  one workgroup per bin: the bin's indices sorted ascending in LDS (bitonic; a bin with more than kOvSortCap of
//                   them is walked in windows of kOvSortCap consecutive primitive indices, each sorted), so every pixel sees its
//                   primitives in feature order whatever the scatter's order; coverage folded with max over a feature's primitives,
//                   blended in linear light, encoded once.  Pixels no feature covers are never written.
// Polygon fills add, for a handle that has them, between k_ov_setup and k_ov_scan:
//   k_pg_setup      one thread per ring-edge slot: drape, transform, near-plane clip (the kept part, or for the closing slot of an exit
//                   edge the segment along the plane to the ring's next entry point), exact screen edge, bin counts, feature box
//   k_pg_header     one thread per fill feature: its box -> a header primitive counted in every bin of the box, and its mask storage
// and after the pair count is read back, before k_ov_scatter:
//   k_pg_backdrop   one thread per edge slot: one atomic XOR per crossed pixel row into the (feature, bin) mask of the bin left of x_c
//   k_pg_prefix     one wave per fill feature: right-to-left prefix XOR along each bin row of its box
// k_ov_composite walks a fill feature as its header (the mask bit of the pixel's row: crossings right of the bin) and its edges in
// the bin (crossings between the pixel and the bin's right edge, and the nearest-edge distance).
// Occlusion: a handle with an occluding point or line layer draws its terrain with the visibility store on, k_ov_setup
// keeps the 1/w of those layers' primitives in a side array, and k_ov_composite_occlude forms the terrain's 1/w of each pixel of a bin
// that holds primitives (terrain_rw, vf_visible.h) and drops an occluding primitive's coverage where the terrain is in front of it.
// All arithmetic is binary32 in the order DESIGN.md states (compiled with -ffp-contract=off); tests/overlay_model/overlay_model.c
// and tests/polygon_model/polygon_model.c are the same contract on the CPU and the GPU frames equal it bit for bit.
#pragma once
#include "vf_device.h"
#include "vf_kernels.h"
#include "vf_visible.h"     // inline functions and templates only: the kernels keep their places

namespace vf {

constexpr uint32_t kOvBin = 16;                 // screen bin = 16 x 16 pixels = one composite workgroup (one pixel per thread)
constexpr uint32_t kOvSortCap = 4096;           // indices a bin sorts in LDS at once
constexpr uint32_t kOvMaxPrims = 1u << 24;      // primitive budget of a handle (all layers)
constexpr uint32_t kOvCircle = 0u, kOvSquare = 1u, kOvSegment = 2u;
constexpr uint32_t kOvKindMask = 3u, kOvDrape = 4u, kOvExt0 = 8u, kOvExt1 = 16u;
constexpr uint32_t kOvOcclude = 32u;            // point / segment of an occluding layer: hidden behind the terrain (pad[0] = bits of kb)
constexpr uint32_t kOvHaze = 64u;               // point / segment of a hazed layer: it takes the handle's atmospheric haze
// polygon fill records (OvIn kind kOvPoly): kPgHeader marks a feature's header, kPgClose an edge's closing-segment slot
constexpr uint32_t kOvPoly = 3u, kPgHeader = kOvExt0, kPgClose = kOvExt1;
constexpr uint32_t kOvFillHdr = 3u, kOvFillEdge = 4u, kOvNone = 7u;  // OvPrim kinds of fill records (kOvNone: nothing this frame)
constexpr uint32_t kPgOff = 1u << 24;           // feature boxes are folded as kPgOff - lo (max) and hi + kPgOff (max): zero is empty

// one primitive as added (host -> HBM once): world-space vertices, y an offset above the surface when kOvDrape is set
struct OvIn {
    float p0[3];
    float p1[3];           // segment end (segments only)
    float size;            // circle / square: r = clamp(size_px, 1, 64) / 2; segment: hw = clamp(width_px, 1, 64) / 2
    uint32_t flags;        // kind | kOvDrape | kOvExt0 / kOvExt1 (square cap: the segment reaches hw past its path's first / last vertex)
    uint32_t rgba;         // sRGB8 bytes, r | g << 8 | b << 16 | alpha << 24
    uint32_t feature;      // feature number (ascending with the primitive index; equal for the primitives of one polyline)
    uint32_t pad[2];       // polygon edge slot: the record index of its ring's first slot, the ring's vertex count;
                           // point / segment with kOvOcclude: pad[0] = bits of kb = 1 + depth_bias (the layer's depth factor)
};
// A polygon fill feature is one header record (rgba = its fill colour) followed by two slots per ring edge (v_e -> v_e+1, ring order):
// the kept part (flags without kPgClose) and the closing segment (kPgClose).  p0 / p1 = v_e / v_e+1; size holds the bits of the
// feature's fill number (0, 1, ... over the handle's fill features), which indexes the per-feature arrays of the polygon pass.
static_assert(sizeof(OvIn) == 48, "OvIn layout is shared with tests/overlay_model");

// one primitive as a frame sees it (k_ov_setup)
struct OvPrim {
    float4 g;              // circle / square: (cx, cy, r, 0); segment: (ax, ay, ux, uy) -- start and unit direction
    float4 h;              // segment: (L, hw, e0, e1)
    uint32_t kind, rgba, feature, pad;
    // fill edge (kOvFillEdge): g = (x0, y0, ex, ey), h = (1 / (ex ex + ey ey) or 0, ex / ey or 0, min x, max x), rgba / pad = bits of
    // min y / max y.  fill header (kOvFillHdr): g = bits of (mask base, bin x0 | bin y0 << 16, bins across, the bin's mask word --
    // filled in by the composite's staging), h = bits of the pixel box (x0, y0, x1, y1), rgba = the fill colour.
};
static_assert(sizeof(OvPrim) == 48, "OvPrim is staged in LDS");

// ---- drape: the rendered surface's height under world (x, z) -----------------------------------------
__device__ __forceinline__ float ov_drape(const FrameParams &P, const AxisTables &A, float x, float z)
{
    float mx = x / P.spacing, mz = z / P.spacing;
    mx = fminf(fmaxf(mx, -1.5f), 1.5f);
    mz = fminf(fmaxf(mz, -1.5f), 1.5f);
    const float gx = (mx + 1.5f) / P.step, gz = (mz + 1.5f) / P.step;
    int i = (int)floorf(gx), j = (int)floorf(gz);
    i = min(max(i, 0), (int)P.nm1 - 1);
    j = min(max(j, 0), (int)P.nm1 - 1);
    const float fx = gx - (float)i, fz = gz - (float)j;
    const uint32_t ui = (uint32_t)i, uj = (uint32_t)j;
    if (fx + fz <= 1.0f) {                                              // triangle (a, b, c)
        const float ha = displaced_height(A, P.tex, P.tw, ui, uj);
        const float hb = displaced_height(A, P.tex, P.tw, ui + 1u, uj);
        const float hc = displaced_height(A, P.tex, P.tw, ui, uj + 1u);
        return (ha + fx * (hb - ha)) + fz * (hc - ha);
    }
    const float hb = displaced_height(A, P.tex, P.tw, ui + 1u, uj);     // triangle (b, c, d)
    const float hc = displaced_height(A, P.tex, P.tw, ui, uj + 1u);
    const float hd = displaced_height(A, P.tex, P.tw, ui + 1u, uj + 1u);
    return (hd + (1.0f - fx) * (hc - hd)) + (1.0f - fz) * (hb - hd);
}

// a vertex in clip space; returns its world height, the y that goes into the view matrix (DESIGN.md 4r reads it)
__device__ __forceinline__ float ov_clip_y(const FrameParams &P, const AxisTables &A, const float p[3], bool drape, float c[4])
{
    float y = p[1];
    if (drape) y = ov_drape(P, A, p[0], p[2]) * P.exag + p[1];
    float vp[4];
    mat_vec(P.view, p[0], y, p[2], 1.0f, vp);
    mat_vec(P.proj, vp[0], vp[1], vp[2], vp[3], c);
    return y;
}

__device__ __forceinline__ void ov_clip(const FrameParams &P, const AxisTables &A, const float p[3], bool drape, float c[4])
{
    (void)ov_clip_y(P, A, p, drape, c);
}

// pixel index range [lo, hi] of coordinate range [a, b] on an axis of n pixels (conservative; empty: lo > hi)
__device__ __forceinline__ void ov_span(float a, float b, uint32_t n, int &lo, int &hi)
{
    const float lim = (float)n + 2.0f;
    lo = (int)floorf(fminf(fmaxf(a, -2.0f), lim));
    hi = (int)floorf(fminf(fmaxf(b, -2.0f), lim));
    lo = max(lo, 0);
    hi = min(hi, (int)n - 1);
}

// dep (a handle with an occluding layer; else nullptr): per primitive (rw_a, rw_b - rw_a, kb, 0) of an occluding point (rw_b = rw_a)
// or segment (its ends after clipping), zero for every other primitive
__global__ __launch_bounds__(256) void k_ov_setup(FrameParams P, AxisTables A, uint32_t nprims, const OvIn *__restrict__ in,
                                                  OvPrim *__restrict__ out, uint2 *__restrict__ box, uint32_t *__restrict__ cnt, uint32_t nbx,
                                                  float4 *__restrict__ dep)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nprims) return;
    const OvIn q = in[i];
    const uint32_t kind = q.flags & kOvKindMask;
    if (kind == kOvPoly) return;                                        // (fill records: k_pg_setup / k_pg_header)
    const bool drape = (q.flags & kOvDrape) != 0u;
    OvPrim o;
    o.g = make_float4(0.0f, 0.0f, 0.0f, 0.0f); o.h = o.g;
    o.kind = kind; o.rgba = q.rgba; o.feature = q.feature; o.pad = 0u;
    float x0 = 0.0f, x1 = -1.0f, y0 = 0.0f, y1 = -1.0f;                // conservative screen extent (empty by default)
    const bool occl = (q.flags & kOvOcclude) != 0u;
    const float kb = __uint_as_float(q.pad[0]);
    float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float a[4];
    ov_clip(P, A, q.p0, drape, a);
    if (kind != kOvSegment) {
        if (finite4(a[0], a[1], a[2], a[3]) && a[3] > 0.0f && !(a[2] < 0.0f) && !(a[2] > a[3])) {
            const float rw = 1.0f / a[3];
            const float sx = fmaf(a[0] * rw, P.hw, P.hw), sy = fmaf(-(a[1] * rw), P.hh, P.hh);
            if (isfinite(sx) && isfinite(sy)) {
                const float r = q.size, R = r + 1.0f;
                o.g = make_float4(sx, sy, r, 0.0f);
                if (occl) d = make_float4(rw, 0.0f, kb, 0.0f);
                x0 = sx - R; x1 = sx + R; y0 = sy - R; y1 = sy + R;
            }
        }
    } else {
        float b[4];
        ov_clip(P, A, q.p1, drape, b);
        bool keep = finite4(a[0], a[1], a[2], a[3]) && finite4(b[0], b[1], b[2], b[3]);
        bool ext0 = (q.flags & kOvExt0) != 0u, ext1 = (q.flags & kOvExt1) != 0u;
        for (int plane = 0; plane < 2 && keep; ++plane) {              // z >= 0, then z <= w; the crossing from the inside vertex outwards
            const float da = plane == 0 ? a[2] : a[3] - a[2], db = plane == 0 ? b[2] : b[3] - b[2];
            const bool ain = da >= 0.0f, bin = db >= 0.0f;
            if (!ain && !bin) { keep = false; break; }
            if (ain && bin) continue;
            float *ou = ain ? b : a;
            const float *inv = ain ? a : b;
            const float di = ain ? da : db, dou = ain ? db : da;
            const float t = di / (di - dou);
            float r[4];
            for (int k = 0; k < 4; ++k) r[k] = fmaf(t, ou[k] - inv[k], inv[k]);
            for (int k = 0; k < 4; ++k) ou[k] = r[k];
            if (ain) ext1 = false; else ext0 = false;                    // a clipped end has no cap
        }
        if (keep && a[3] > 0.0f && b[3] > 0.0f) {
            const float rwa = 1.0f / a[3], rwb = 1.0f / b[3];
            const float ax = fmaf(a[0] * rwa, P.hw, P.hw), ay = fmaf(-(a[1] * rwa), P.hh, P.hh);
            const float bx = fmaf(b[0] * rwb, P.hw, P.hw), by = fmaf(-(b[1] * rwb), P.hh, P.hh);
            const float ex = bx - ax, ey = by - ay;
            const float L = sqrtf(ex * ex + ey * ey);
            if (isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by) && L > 0.0f && isfinite(L)) {
                const float hw = q.size, e0 = ext0 ? hw : 0.0f, e1 = ext1 ? hw : 0.0f;
                o.g = make_float4(ax, ay, ex / L, ey / L);
                o.h = make_float4(L, hw, e0, e1);
                if (occl) d = make_float4(rwa, rwb - rwa, kb, 0.0f);
                const float R = hw + fmaxf(e0, e1) + 1.0f;
                x0 = fminf(ax, bx) - R; x1 = fmaxf(ax, bx) + R; y0 = fminf(ay, by) - R; y1 = fmaxf(ay, by) + R;
            }
        }
    }
    out[i] = o;
    if (dep) dep[i] = d;
    int px0 = 1, px1 = 0, py0 = 1, py1 = 0;
    if (x0 <= x1) { ov_span(x0, x1, P.W, px0, px1); ov_span(y0, y1, P.H, py0, py1); }
    if (px0 > px1 || py0 > py1) { box[i] = make_uint2(1u, 0u); return; }   // (bin x0 = 1 > x1 = 0: nothing)
    const uint32_t bx0 = (uint32_t)px0 / kOvBin, bx1 = (uint32_t)px1 / kOvBin, by0 = (uint32_t)py0 / kOvBin, by1 = (uint32_t)py1 / kOvBin;
    box[i] = make_uint2(bx0 | (by0 << 16), bx1 | (by1 << 16));
    for (uint32_t by = by0; by <= by1; ++by)
        for (uint32_t bx = bx0; bx <= bx1; ++bx) atomicAdd(&cnt[by * nbx + bx], 1u);
}

// exclusive scan of the bin counts into start[0..nbins), the total into start[nbins] (saturated at 2^32 - 1) and ovf[0]; counts reset to 0
__global__ __launch_bounds__(1024) void k_ov_scan(uint32_t nbins, uint32_t *__restrict__ cnt, uint32_t *__restrict__ start)
{
    __shared__ uint32_t part[1024];
    __shared__ unsigned long long carry;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) carry = 0ull;
    __syncthreads();
    for (uint32_t base = 0; base < nbins; base += 1024u) {
        const uint32_t k = base + tid;
        const uint32_t v = k < nbins ? cnt[k] : 0u;
        part[tid] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 1024u; d <<= 1) {                     // inclusive Hillis-Steele scan
            const uint32_t add = tid >= d ? part[tid - d] : 0u;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        const unsigned long long c = carry, excl = c + part[tid] - v;
        if (k < nbins) { start[k] = excl > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)excl; cnt[k] = 0u; }
        __syncthreads();
        if (tid == 1023u) carry = c + part[1023];
        __syncthreads();
    }
    if (tid == 0) start[nbins] = carry > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)carry;
}

__global__ __launch_bounds__(256) void k_ov_scatter(uint32_t nprims, const uint2 *__restrict__ box, uint32_t nbx,
                                                    const uint32_t *__restrict__ start, uint32_t *__restrict__ cnt, uint32_t *__restrict__ list)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nprims) return;
    const uint2 b = box[i];
    const uint32_t bx0 = b.x & 0xFFFFu, by0 = b.x >> 16, bx1 = b.y & 0xFFFFu, by1 = b.y >> 16;
    for (uint32_t by = by0; by <= by1 && bx0 <= bx1; ++by)
        for (uint32_t bx = bx0; bx <= bx1; ++bx) {
            const uint32_t bin = by * nbx + bx;
            list[start[bin] + atomicAdd(&cnt[bin], 1u)] = i;
        }
}

// ---- polygon fills ----------------------------------------------------------------

// the near plane (z >= 0) crossing of clip-space segment in -> out, §4b's formula
__device__ __forceinline__ void pg_cross(const float in[4], const float out[4], float r[4])
{
    const float di = in[2], dou = out[2];
    const float t = di / (di - dou);
    for (int k = 0; k < 4; ++k) r[k] = fmaf(t, out[k] - in[k], in[k]);
}

__device__ __forceinline__ bool pg_screen(const FrameParams &P, const float c[4], float &sx, float &sy)
{
    if (!(c[3] > 0.0f)) return false;
    const float rw = 1.0f / c[3];
    sx = fmaf(c[0] * rw, P.hw, P.hw);
    sy = fmaf(-(c[1] * rw), P.hh, P.hh);
    return isfinite(sx) && isfinite(sy);
}

// row crossing of a fill edge at pixel-centre row qy (the caller has checked min y <= qy < max y): x_c, clamped to the edge's x range
__device__ __forceinline__ float pg_xc(const OvPrim &p, float qy)
{
    return fminf(fmaxf(fmaf(qy - p.g.y, p.h.y, p.g.x), p.h.z), p.h.w);
}

__global__ __launch_bounds__(256) void k_pg_setup(FrameParams P, AxisTables A, uint32_t lo, uint32_t hi, const OvIn *__restrict__ in,
                                                  OvPrim *__restrict__ out, uint2 *__restrict__ box, uint32_t *__restrict__ cnt, uint32_t nbx,
                                                  uint4 *__restrict__ fbox)
{
    // (no early return: the whole wave takes part in the feature-box fold below)
    const uint32_t i = lo + blockIdx.x * blockDim.x + threadIdx.x;
    OvIn q{};
    if (i < hi) q = in[i];
    const bool slot = i < hi && (q.flags & kOvKindMask) == kOvPoly && (q.flags & kPgHeader) == 0u;
    const bool drape = (q.flags & kOvDrape) != 0u;
    float s0[4], s1[4];
    bool have = false;
    if (slot) {
        float a[4], b[4];
        ov_clip(P, A, q.p0, drape, a);
        ov_clip(P, A, q.p1, drape, b);
        const bool ain = a[2] >= 0.0f, bin = b[2] >= 0.0f;
        if ((q.flags & kPgClose) == 0u) {                               // the kept part of v_e -> v_e+1
            if (ain || bin) {
                have = true;
                for (int k = 0; k < 4; ++k) { s0[k] = a[k]; s1[k] = b[k]; }
                if (!bin) pg_cross(a, b, s1);
                else if (!ain) pg_cross(b, a, s0);
            }
        } else if (ain && !bin) {                                       // an exit: along the plane to the ring's next entry point
            pg_cross(a, b, s0);
            const uint32_t first = q.pad[0], nv = q.pad[1], e = (i - first) >> 1;
            float prev[4] = { b[0], b[1], b[2], b[3] };
            for (uint32_t k = 2; k <= nv; ++k) {                        // v_e+k; v_e+nv = v_e is inside, so this ends
                const uint32_t j = (e + k) % nv;
                float c[4];
                ov_clip(P, A, in[first + 2u * j].p0, drape, c);
                if (c[2] >= 0.0f) { pg_cross(c, prev, s1); have = true; break; }
                for (int m = 0; m < 4; ++m) prev[m] = c[m];
            }
        }
    }
    OvPrim o;
    o.g = make_float4(0.0f, 0.0f, 0.0f, 0.0f); o.h = o.g;
    o.kind = kOvNone; o.rgba = 0u; o.feature = q.feature; o.pad = 0u;
    float ax, ay, bx, by;
    uint4 f = make_uint4(0u, 0u, 0u, 0u);                               // this edge's share of the feature box (folded with max)
    if (have && pg_screen(P, s0, ax, ay) && pg_screen(P, s1, bx, by)) {
        const float ex = bx - ax, ey = by - ay;
        const float l2 = ex * ex + ey * ey;
        const float xmin = fminf(ax, bx), xmax = fmaxf(ax, bx), ymin = fminf(ay, by), ymax = fmaxf(ay, by);
        o.g = make_float4(ax, ay, ex, ey);
        o.h = make_float4(l2 > 0.0f ? 1.0f / l2 : 0.0f, ey != 0.0f ? ex / ey : 0.0f, xmin, xmax);
        o.kind = kOvFillEdge; o.rgba = __float_as_uint(ymin); o.pad = __float_as_uint(ymax);
        // the feature box folds every kept edge's extent +-1 px (each axis floored in [-2, n + 2]), clipped to the frame later
        const float lim_x = (float)P.W + 2.0f, lim_y = (float)P.H + 2.0f;
        const int fx0 = (int)floorf(fminf(fmaxf(xmin - 1.0f, -2.0f), lim_x)), fx1 = (int)floorf(fminf(fmaxf(xmax + 1.0f, -2.0f), lim_x));
        const int fy0 = (int)floorf(fminf(fmaxf(ymin - 1.0f, -2.0f), lim_y)), fy1 = (int)floorf(fminf(fmaxf(ymax + 1.0f, -2.0f), lim_y));
        f = make_uint4(kPgOff - (uint32_t)(fx0 + 2) + 2u, kPgOff - (uint32_t)(fy0 + 2) + 2u,   // (kPgOff - fx0, unsigned)
                       (uint32_t)(fx1 + 2) + kPgOff - 2u, (uint32_t)(fy1 + 2) + kPgOff - 2u);
    }
    // fold into fbox[feature]: one set of atomics per wave when its edges all belong to one feature (a long ring's edges otherwise
    // queue on the same four words), else one per edge
    const bool edge = o.kind == kOvFillEdge;
    const uint32_t kf = __float_as_uint(q.size);
    const unsigned long long voters = __ballot(edge);
    if (voters) {
        const int leader = __ffsll((long long)voters) - 1;
        const uint32_t k0 = __shfl(kf, leader);
        if (__all(!edge || kf == k0)) {
            for (int d = 1; d < 64; d <<= 1) {
                f.x = max(f.x, __shfl_xor(f.x, d)); f.y = max(f.y, __shfl_xor(f.y, d));
                f.z = max(f.z, __shfl_xor(f.z, d)); f.w = max(f.w, __shfl_xor(f.w, d));
            }
            if ((int)(threadIdx.x & 63u) == leader) {
                uint4 *F = fbox + k0;
                atomicMax(&F->x, f.x); atomicMax(&F->y, f.y); atomicMax(&F->z, f.z); atomicMax(&F->w, f.w);
            }
        } else if (edge) {
            uint4 *F = fbox + kf;
            atomicMax(&F->x, f.x); atomicMax(&F->y, f.y); atomicMax(&F->z, f.z); atomicMax(&F->w, f.w);
        }
    }
    if (!slot) return;
    out[i] = o;
    int px0 = 1, px1 = 0, py0 = 1, py1 = 0;
    // x over the whole width of the bins, not the frame's: the last bin column of a frame that is no multiple of the bin width counts
    // the crossings between the frame's edge and its own right edge itself (k_pg_backdrop gives a bin the crossings beyond it only)
    if (edge) { ov_span(o.h.z - 1.0f, o.h.w + 1.0f, nbx * kOvBin, px0, px1); ov_span(__uint_as_float(o.rgba) - 1.0f, __uint_as_float(o.pad) + 1.0f, P.H, py0, py1); }
    if (px0 > px1 || py0 > py1) { box[i] = make_uint2(1u, 0u); return; }
    const uint32_t bx0 = (uint32_t)px0 / kOvBin, bx1 = (uint32_t)px1 / kOvBin, by0 = (uint32_t)py0 / kOvBin, by1 = (uint32_t)py1 / kOvBin;
    box[i] = make_uint2(bx0 | (by0 << 16), bx1 | (by1 << 16));
    for (uint32_t y = by0; y <= by1; ++y)
        for (uint32_t x = bx0; x <= bx1; ++x) atomicAdd(&cnt[y * nbx + x], 1u);
}

// one thread per fill feature: the folded box (reset for the next frame) -> the header primitive, counted in every bin of the box,
// and the feature's share of the mask storage: fbin = (mask base, bin x0 | bin y0 << 16, bins across, bins down)
__global__ __launch_bounds__(256) void k_pg_header(FrameParams P, uint32_t nfill, const uint32_t *__restrict__ hdr, const OvIn *__restrict__ in,
                                                   uint4 *__restrict__ fbox, uint4 *__restrict__ fbin, OvPrim *__restrict__ out,
                                                   uint2 *__restrict__ box, uint32_t *__restrict__ cnt, uint32_t nbx,
                                                   unsigned long long *__restrict__ mask_total)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nfill) return;
    const uint32_t i = hdr[k];
    const uint4 f = fbox[k];
    fbox[k] = make_uint4(0u, 0u, 0u, 0u);
    OvPrim o;
    o.g = make_float4(0.0f, 0.0f, 0.0f, 0.0f); o.h = o.g;
    o.kind = kOvFillHdr; o.rgba = in[i].rgba; o.feature = in[i].feature; o.pad = 0u;
    int px0 = 1, px1 = 0, py0 = 1, py1 = 0;
    if (f.x != 0u) {
        px0 = max((int)(kPgOff - f.x), 0); py0 = max((int)(kPgOff - f.y), 0);
        px1 = min((int)(f.z - kPgOff), (int)P.W - 1); py1 = min((int)(f.w - kPgOff), (int)P.H - 1);
    }
    if (px0 > px1 || py0 > py1) {
        o.kind = kOvNone; out[i] = o; box[i] = make_uint2(1u, 0u); fbin[k] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const uint32_t bx0 = (uint32_t)px0 / kOvBin, bx1 = (uint32_t)px1 / kOvBin, by0 = (uint32_t)py0 / kOvBin, by1 = (uint32_t)py1 / kOvBin;
    const uint32_t fw = bx1 - bx0 + 1u, fh = by1 - by0 + 1u;
    const uint32_t base = (uint32_t)atomicAdd(mask_total, (unsigned long long)fw * fh);   // (the host refuses a total beyond 2^32 - 1)
    o.g = make_float4(__uint_as_float(base), __uint_as_float(bx0 | (by0 << 16)), __uint_as_float(fw), 0.0f);
    o.h = make_float4(__uint_as_float((uint32_t)px0), __uint_as_float((uint32_t)py0), __uint_as_float((uint32_t)px1), __uint_as_float((uint32_t)py1));
    out[i] = o;
    fbin[k] = make_uint4(base, bx0 | (by0 << 16), fw, fh);
    box[i] = make_uint2(bx0 | (by0 << 16), bx1 | (by1 << 16));
    for (uint32_t y = by0; y <= by1; ++y)
        for (uint32_t x = bx0; x <= bx1; ++x) atomicAdd(&cnt[y * nbx + x], 1u);
}

// one thread per edge slot: for every pixel row the edge crosses (min y <= qy < max y), flip bit (row & 15) of the mask word of the
// rightmost bin of the feature's box whose right edge is <= x_c (none left of the box: no flip)
__global__ __launch_bounds__(256) void k_pg_backdrop(uint32_t H, uint32_t lo, uint32_t hi, const OvIn *__restrict__ in,
                                                     const OvPrim *__restrict__ prims, const uint4 *__restrict__ fbin, uint32_t *__restrict__ mask)
{
    const uint32_t i = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hi) return;
    const OvPrim p = prims[i];
    if ((in[i].flags & kOvKindMask) != kOvPoly || p.kind != kOvFillEdge) return;
    const uint4 f = fbin[__float_as_uint(in[i].size)];
    if (f.z == 0u) return;
    const int bx0 = (int)(f.y & 0xFFFFu), by0 = (int)(f.y >> 16), bx1 = bx0 + (int)f.z - 1;
    const float ymin = __uint_as_float(p.rgba), ymax = __uint_as_float(p.pad);
    int r0, r1;
    ov_span(ymin - 1.0f, ymax + 1.0f, H, r0, r1);
    for (int r = r0; r <= r1; ++r) {
        const float qy = (float)r + 0.5f;
        if (!(ymin <= qy && qy < ymax)) continue;
        const float xc = pg_xc(p, qy);
        int j = (int)floorf(fminf(fmaxf(xc * 0.0625f, -1.0f), 65536.0f)) - 1;       // (j + 1) * 16 <= x_c
        if (j < bx0) continue;
        j = min(j, bx1);
        atomicXor(&mask[f.x + (uint32_t)(r / (int)kOvBin - by0) * f.z + (uint32_t)(j - bx0)], 1u << (r & 15));
    }
}

// one wave per fill feature, a lane per bin row of its box: mask[b] ^= mask[b + 1] ^ ... (right to left)
__global__ __launch_bounds__(256) void k_pg_prefix(uint32_t nfill, const uint4 *__restrict__ fbin, uint32_t *__restrict__ mask)
{
    const uint32_t k = (blockIdx.x * blockDim.x + threadIdx.x) / 64u, lane = threadIdx.x & 63u;
    if (k >= nfill) return;
    const uint4 f = fbin[k];
    for (uint32_t row = lane; row < f.w; row += 64u) {
        uint32_t *m = mask + f.x + row * f.z;
        uint32_t acc = 0u;
        for (uint32_t c = f.z; c-- > 0u;) { acc ^= m[c]; m[c] = acc; }
    }
}

// coverage of pixel centre (qx, qy) by one primitive
__device__ __forceinline__ float ov_cover(const OvPrim &p, float qx, float qy)
{
    float sd;
    if (p.kind == kOvSegment) {
        const float dx = qx - p.g.x, dy = qy - p.g.y;
        const float u = dx * p.g.z + dy * p.g.w;
        const float v = fabsf(dy * p.g.z - dx * p.g.w);
        sd = fmaxf(v - p.h.y, fmaxf(-u - p.h.z, (u - p.h.x) - p.h.w));
    } else {
        const float dx = qx - p.g.x, dy = qy - p.g.y;
        sd = p.kind == kOvCircle ? sqrtf(dx * dx + dy * dy) - p.g.z : fmaxf(fabsf(dx), fabsf(dy)) - p.g.z;
    }
    return fminf(fmaxf(0.5f - sd, 0.0f), 1.0f);
}

struct OvPixel {
    float c[3];
    bool touched;
    uint32_t feature, rgba;
    float cov;
    bool fill;             // the feature in hand is a fill and the pixel is in its box: par / d2 give its coverage
    uint32_t par;          // even-odd parity of the crossings right of the pixel so far
    float d2;              // squared distance to the nearest edge so far
};

// a fill feature's coverage, once its header and every edge of the bin are folded in
__device__ __forceinline__ void pg_fill_cover(OvPixel &S)
{
    if (!S.fill) return;
    const float d = sqrtf(S.d2);
    const float sd = S.par ? -d : d;
    S.cov = fminf(fmaxf(0.5f - sd, 0.0f), 1.0f);
}

// the feature in hand is done at this pixel: blend it (if it covers the pixel at all)
__device__ __forceinline__ void ov_flush(OvPixel &S, const float *dec, const uint32_t *rgba, size_t o)
{
    if (!(S.cov > 0.0f)) return;
    if (!S.touched) {
        const uint32_t px = rgba[o];
        S.c[0] = dec[px & 255u]; S.c[1] = dec[(px >> 8) & 255u]; S.c[2] = dec[(px >> 16) & 255u];
        S.touched = true;
    }
    const float a = S.cov * ((float)(S.rgba >> 24) / 255.0f);
    for (int k = 0; k < 3; ++k) {
        const float s = dec[(S.rgba >> (8 * k)) & 255u];
        S.c[k] = s * a + S.c[k] * (1.0f - a);
    }
}

// What a pixel of a composite that hazes overlays keeps beside OvPixel: nothing in the other composites
template <bool HAZE> struct OvHazePixel {};
template <> struct OvHazePixel<true> {
    float ah;              // the haze opacity of the primitive that gave S.cov (0: none, or a primitive of a layer that is not hazed)
    float lin[3];          // the haze colour in linear light
};

// What such a composite is handed beside the others' arguments: the frame's haze Z (vf_haze.h's HazeParams -- a template parameter,
// HZ, because that header comes behind the library's last plain kernel, 4d), the side records hz of k_ov_haze_setup and their staging
// array in LDS.  Empty otherwise, and every use of it is a dependent name: the other instantiations are what they were without it.
template <bool HAZE, class HZ> struct OvHazeArgs {};
template <class HZ> struct OvHazeArgs<true, HZ> {
    const HZ *Z;
    const float4 *hz;
    float4 *shz;
};

// ov_flush for a composite that hazes overlays: the feature's own alpha is not changed
__device__ __forceinline__ void ov_flush_hazed(OvPixel &S, const OvHazePixel<true> &Hz, const float *dec, const uint32_t *rgba, size_t o)
{
    const float ah = Hz.ah;
    const float *hzl = Hz.lin;
    if (!(S.cov > 0.0f)) return;
    if (!S.touched) {
        const uint32_t px = rgba[o];
        S.c[0] = dec[px & 255u]; S.c[1] = dec[(px >> 8) & 255u]; S.c[2] = dec[(px >> 16) & 255u];
        S.touched = true;
    }
    const float a = S.cov * ((float)(S.rgba >> 24) / 255.0f);
    for (int k = 0; k < 3; ++k) {
        float s = dec[(S.rgba >> (8 * k)) & 255u];
        if (ah > 0.0f) s = hzl[k] * ah + s * (1.0f - ah);
        S.c[k] = s * a + S.c[k] * (1.0f - a);
    }
}

// The haze opacity of primitive p at pixel centre (qx, qy), from its side record hz (k_ov_haze_setup; rw_a == 0: not hazed).  A
// segment's is (rw_a, rw_b - rw_a, yq_a, yq_b - yq_a): its depth d = 1 / rw and its world height y at the pixel, perspective-correct
// along it.  A point's is (rw, 0, y_c, ah): the same at every pixel, formed by the set-up kernel.  HZ is vf_haze.h's HazeParams, and haze_alpha is found there when this is instantiated: that
// header comes behind the library's last plain kernel (4d), so this one does not include it.
template <class HZ>
__device__ __forceinline__ float ov_haze_at(const HZ &Z, const OvPrim &p, const float4 hz, float qx, float qy)
{
    if (!(hz.x > 0.0f)) return 0.0f;
    if (p.kind != kOvSegment) return hz.w;
    const float u = (qx - p.g.x) * p.g.z + (qy - p.g.y) * p.g.w;
    const float t = fminf(fmaxf(u / p.h.x, 0.0f), 1.0f);
    const float rw = fmaf(t, hz.y, hz.x);
    const float y = fmaf(t, hz.w, hz.z) / rw;
    return haze_alpha(Z, 1.0f / rw, y);
}

// terrain_rw (vf_visible.h) for the composite that hazes and occludes: the same statements, always inlined.  terrain_rw is an
// ordinary inline function; a second kernel calling it changed the register allocation of its first caller, k_ov_composite_occlude
// (24 instructions of the clipper's scratch path, the count unchanged -- tools/isa_hash.py), so that kernel stays its
// only caller.  tests/test_gpu_overlay_haze.py holds both to the occlusion model's terrain_q.
__device__ __forceinline__ float ov_terrain_rw(const FrameParams &P, const SetupView &V, uint32_t prim, int32_t px, int32_t py)
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

// bitonic sort of keys[0..m) ascending, m a power of two <= kOvSortCap (whole workgroup)
__device__ __forceinline__ void ov_sort(uint32_t *keys, uint32_t m)
{
    for (uint32_t k = 2; k <= m; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint32_t x = keys[i], y = keys[l];
                    if ((x > y) == ((i & k) == 0u)) { keys[i] = y; keys[l] = x; }
                }
            }
            __syncthreads();
        }
}

__device__ __forceinline__ uint32_t ov_pow2(uint32_t n)
{
    uint32_t m = 1;
    while (m < n) m <<= 1;
    return m;
}

// The compositing workgroup of one bin (k_ov_composite, k_ov_composite_occlude; the LDS arrays are the kernel's).  OCCLUDE (a handle
// with an occluding layer): P, V and vis give each pixel the terrain's 1/w, dep / sdep each occluding primitive its own;
// the other instantiation does not read them.  HAZE (a frame that hazes overlay layers; the kernels are in
// vf_overlay_haze.h): HA gives each primitive of a hazed layer its depth and height, and the frame's haze.
template <bool OCCLUDE, bool HAZE = false, class HZ = void>
__device__ __forceinline__ void ov_composite(uint32_t W, uint32_t H, uint32_t nbx, const OvPrim *__restrict__ prims,
                                             uint32_t *__restrict__ cnt, const uint32_t *__restrict__ start,
                                             const uint32_t *__restrict__ list, const float *__restrict__ decode,
                                             const float *__restrict__ thresh, const uint32_t *__restrict__ mask,
                                             uint32_t *__restrict__ rgba, const FrameParams *P, const SetupView *V,
                                             const uint32_t *__restrict__ vis, const float4 *__restrict__ dep,
                                             uint32_t *keys, OvPrim *recs, float4 *sdep, float *sdec, float *sthr, uint32_t &s_n, uint32_t &s_next,
                                             const OvHazeArgs<HAZE, HZ> HA = {})
{
    // (built without the tuning switches this kernel takes exactly v0..v39 and a 64-bit shift by v39: the form isa_lint refuses, vf_device.h)
    VF_RESERVE_VGPR(40);
    const uint32_t bin = blockIdx.x, tid = threadIdx.x;
    const uint32_t n = cnt[bin];
    if (n == 0u) return;
    sdec[tid] = decode[tid];
    sthr[tid] = thresh[tid];
    const uint32_t px = (bin % nbx) * kOvBin + (tid & (kOvBin - 1u)), py = (bin / nbx) * kOvBin + tid / kOvBin;
    const bool on = px < W && py < H;
    const size_t o = (size_t)py * W + px;
    const float qx = (float)px + 0.5f, qy = (float)py + 0.5f;
    const float rb = (float)((bin % nbx + 1u) * kOvBin);                // the bin's right edge (fill crossings beyond it: the mask)
    float Q = 0.0f;                                                     // the terrain's 1/w here (background: 0, hides nothing)
    if constexpr (OCCLUDE) {
        if (on) {
            const uint32_t id = vis[o];
            if constexpr (HAZE) { if (id) Q = ov_terrain_rw(*P, *V, id - 1u, (int32_t)px, (int32_t)py); }
            else if (id) Q = terrain_rw(*P, *V, id - 1u, (int32_t)px, (int32_t)py);
        }
    }
    OvPixel S;
    S.c[0] = S.c[1] = S.c[2] = 0.0f; S.touched = false; S.feature = 0xFFFFFFFFu; S.rgba = 0u; S.cov = 0.0f;
    S.fill = false; S.par = 0u; S.d2 = 0.0f;
    OvHazePixel<HAZE> Hz;
    if constexpr (HAZE) {
        Hz.ah = 0.0f;
        for (int k = 0; k < 3; ++k) Hz.lin[k] = decode[(HA.Z->rgba >> (8 * k)) & 255u];
    }
    const uint32_t *L = list + start[bin];
    // composite keys[0..m) (sorted): records staged 256 at a time, every pixel walks them in order
    auto run = [&](uint32_t m) {
        for (uint32_t k0 = 0; k0 < m; k0 += 256u) {
            __syncthreads();
            if (k0 + tid < m) {
                recs[tid] = prims[keys[k0 + tid]];
                if constexpr (OCCLUDE) sdep[tid] = dep[keys[k0 + tid]];
                if constexpr (HAZE) HA.shz[tid] = HA.hz[keys[k0 + tid]];
                OvPrim &r = recs[tid];
                if (r.kind == kOvFillHdr) {                             // this bin's word of the feature's backdrop mask
                    const uint32_t b0 = __float_as_uint(r.g.y), fw = __float_as_uint(r.g.z);
                    const uint32_t w = __float_as_uint(r.g.x) + (bin / nbx - (b0 >> 16)) * fw + (bin % nbx - (b0 & 0xFFFFu));
                    r.g.w = __uint_as_float(mask[w]);
                }
            }
            __syncthreads();
            const uint32_t kn = min(256u, m - k0);
            if (on)
                for (uint32_t k = 0; k < kn; ++k) {
                    const OvPrim &p = recs[k];
                    if (p.feature != S.feature) {
                        pg_fill_cover(S);
                        if constexpr (HAZE) { ov_flush_hazed(S, Hz, sdec, rgba, o); Hz.ah = 0.0f; }
                        else ov_flush(S, sdec, rgba, o);
                        S.feature = p.feature; S.rgba = p.rgba; S.cov = 0.0f; S.fill = false;
                    }
                    if (p.kind <= kOvSegment) {
                        float c = ov_cover(p, qx, qy);
                        if constexpr (OCCLUDE) {
                            const float4 d = sdep[k];
                            if (d.z > 0.0f && c > 0.0f) {                // an occluding primitive: its 1/w here against the terrain's
                                float rw = d.x;
                                if (p.kind == kOvSegment) {
                                    const float u = (qx - p.g.x) * p.g.z + (qy - p.g.y) * p.g.w;
                                    rw = fmaf(fminf(fmaxf(u / p.h.x, 0.0f), 1.0f), d.y, d.x);
                                }
                                if (Q > rw * d.z) c = 0.0f;
                            }
                        }
                        if constexpr (HAZE) {                           // the first primitive that reaches the feature's maximum speaks for it
                            if (c > S.cov) { S.cov = c; Hz.ah = ov_haze_at(*HA.Z, p, HA.shz[k], qx, qy); }
                        }
                        else S.cov = fmaxf(S.cov, c);
                    }
                    else if (p.kind == kOvFillEdge) {
                        const float ymin = __uint_as_float(p.rgba), ymax = __uint_as_float(p.pad);
                        if (ymin <= qy && qy < ymax) {
                            const float xc = pg_xc(p, qy);
                            S.par ^= (qx < xc && xc < rb) ? 1u : 0u;
                        }
                        const float dx = qx - p.g.x, dy = qy - p.g.y;
                        const float t = fminf(fmaxf((dx * p.g.z + dy * p.g.w) * p.h.x, 0.0f), 1.0f);
                        const float rx = dx - t * p.g.z, ry = dy - t * p.g.w;
                        S.d2 = fminf(S.d2, rx * rx + ry * ry);
                    } else {                                            // fill header: the pixel's row of the mask, nothing near yet
                        S.par = (__float_as_uint(p.g.w) >> (tid / kOvBin)) & 1u;
                        S.d2 = INFINITY;
                        S.fill = px >= __float_as_uint(p.h.x) && py >= __float_as_uint(p.h.y) && px <= __float_as_uint(p.h.z) && py <= __float_as_uint(p.h.w);
                    }
                }
        }
    };
    if (n <= kOvSortCap) {
        const uint32_t m = ov_pow2(n);
        for (uint32_t k = tid; k < m; k += 256u) keys[k] = k < n ? L[k] : 0xFFFFFFFFu;
        __syncthreads();
        ov_sort(keys, m);
        run(n);
    } else {
        // more than fit: windows of kOvSortCap consecutive primitive indices (indices are unique in a bin, so a window never holds more),
        // each gathered, sorted and composited in turn; the next window starts at the smallest index beyond the current one
        uint32_t lo = 0;
        for (;;) {
            __syncthreads();
            if (tid == 0) { s_n = 0u; s_next = 0xFFFFFFFFu; }
            __syncthreads();
            uint32_t next = 0xFFFFFFFFu;
            for (uint32_t k = tid; k < n; k += 256u) {
                const uint32_t v = L[k];
                if (v >= lo && v - lo < kOvSortCap) keys[atomicAdd(&s_n, 1u)] = v;
                else if (v >= lo) next = min(next, v);
            }
            atomicMin(&s_next, next);
            __syncthreads();
            const uint32_t got = s_n, m = ov_pow2(got), nxt = s_next;
            for (uint32_t k = got + tid; k < m; k += 256u) keys[k] = 0xFFFFFFFFu;
            __syncthreads();
            ov_sort(keys, m);
            run(got);
            if (nxt == 0xFFFFFFFFu) break;
            lo = nxt;
        }
    }
    if (on) {
        pg_fill_cover(S);
        if constexpr (HAZE) ov_flush_hazed(S, Hz, sdec, rgba, o);
        else ov_flush(S, sdec, rgba, o);
        if (S.touched)
            rgba[o] = srgb_encode(S.c[0], sthr) | (srgb_encode(S.c[1], sthr) << 8) | (srgb_encode(S.c[2], sthr) << 16) | 0xFF000000u;
    }
    __syncthreads();
    if (tid == 0) cnt[bin] = 0u;                         // (the next frame's k_ov_setup counts from zero)
}

} // namespace vf
#include "vf_contour.h"     // the contour kernels, here: k_ov_composite stays the library's last non-template kernel (4d)
namespace vf {

// vf_terrain_set_layer_occlusion: a point / line layer's records [lo, hi) gain or lose kOvOcclude and kb, in place
__global__ __launch_bounds__(256) void k_ov_occlude(uint32_t lo, uint32_t hi, OvIn *__restrict__ in, uint32_t on, uint32_t kb_bits)
{
    const uint32_t i = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hi) return;
    OvIn &q = in[i];
    if ((q.flags & kOvKindMask) == kOvPoly) return;
    q.flags = on ? (q.flags | kOvOcclude) : (q.flags & ~kOvOcclude);
    q.pad[0] = on ? kb_bits : 0u;
}

// The composite of a handle with an occluding layer (reads the frame's visibility, vis, and the set-up's vertex records, V).
__global__ __launch_bounds__(256) void k_ov_composite_occlude(uint32_t W, uint32_t H, uint32_t nbx, const OvPrim *__restrict__ prims,
                                                              uint32_t *__restrict__ cnt, const uint32_t *__restrict__ start,
                                                              const uint32_t *__restrict__ list, const float *__restrict__ decode,
                                                              const float *__restrict__ thresh, const uint32_t *__restrict__ mask,
                                                              uint32_t *__restrict__ rgba, FrameParams P, SetupView V,
                                                              const uint32_t *__restrict__ vis, const float4 *__restrict__ dep)
{
    __shared__ uint32_t keys[kOvSortCap];
    __shared__ OvPrim recs[256];
    __shared__ float4 sdep[256];
    __shared__ float sdec[256], sthr[256];
    __shared__ uint32_t s_n, s_next;
    ov_composite<true>(W, H, nbx, prims, cnt, start, list, decode, thresh, mask, rgba, &P, &V, vis, dep, keys, recs, sdep, sdec, sthr, s_n, s_next);
}

// The composite of every other handle with overlays.  (Kept the last plain kernel of the library, and as it was before occlusion
// existed: the code after it -- the generic raster path the tile kernels call -- keeps its place, so their calls stay bit-identical.)
__global__ __launch_bounds__(256) void k_ov_composite(uint32_t W, uint32_t H, uint32_t nbx, const OvPrim *__restrict__ prims,
                                                      uint32_t *__restrict__ cnt, const uint32_t *__restrict__ start,
                                                      const uint32_t *__restrict__ list, const float *__restrict__ decode,
                                                      const float *__restrict__ thresh, const uint32_t *__restrict__ mask,
                                                      uint32_t *__restrict__ rgba)
{
    __shared__ uint32_t keys[kOvSortCap];
    __shared__ OvPrim recs[256];
    __shared__ float sdec[256], sthr[256];
    __shared__ uint32_t s_n, s_next;
    ov_composite<false>(W, H, nbx, prims, cnt, start, list, decode, thresh, mask, rgba, nullptr, nullptr, nullptr, nullptr, keys, recs, nullptr,
                        sdec, sthr, s_n, s_next);
}

} // namespace vf

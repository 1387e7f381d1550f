// raster_cases.h -- the case stream of the span-solver checks, stated once: random triangles of ten kinds (24.8 fixed point, around a
// 4096^2 target, or around one of another extent up to the frame limit of 16384) with a tile (or strip) window that meets their
// bounding box, and the brute-force int64 evaluation of the coverage rule of DESIGN.md section 4 (pixel centres, top-left rule on
// inside-positive edge functions) they are all held against.
// Users: tests/cpp/raster_fuzz.cpp (vf_raster.h compiled for the host) and tests/hip/raster_device_fuzz.hip (the same header, and the
// line loop that walks it, as device code).  The same seed gives the same triangles in both.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <random>

namespace raster_cases {

static inline bool covered(const int32_t X[3], const int32_t Y[3], int32_t px, int32_t py)
{
    const int64_t Px = (int64_t)px * 256 + 128, Py = (int64_t)py * 256 + 128;
    for (int i = 0; i < 3; ++i) {
        const int a = i == 0 ? 1 : (i == 1 ? 2 : 0), b = i == 0 ? 2 : (i == 1 ? 0 : 1);
        const int64_t A = (int64_t)Y[b] - Y[a], B = -((int64_t)X[b] - X[a]);
        const int64_t e = A * (Px - X[a]) + B * (Py - Y[a]);
        const bool tl = A > 0 || (A == 0 && B > 0);
        if (!(e > 0 || (e == 0 && tl))) return false;
    }
    return true;
}

// One accepted draw: a front-facing triangle (negative area in y-down pixels, extents below 2^24), the window and the pixel
// rectangle [px0, px1] x [py0, py1] where its box and the window meet (never empty).
struct Case {
    int kind;                                  // 0 - 9, see Stream::draw
    int32_t X[3], Y[3];
    int32_t tx_lo, tx_hi, ty_lo, ty_hi;        // the window: width 4 .. 64 (a power of two), height 1 .. 64
    int32_t px0, px1, py0, py1;
};

// What the solver is handed for a case: the short axis of the rectangle is the outer one.
struct SolverArgs {
    bool cols;                                 // the outer axis is x (swapped = !cols)
    int32_t U[3], V[3], n_outer, n_inner, u0c, v0c;
};
static inline SolverArgs solver_args(const Case &c)
{
    SolverArgs a;
    a.cols = (c.px1 - c.px0) <= (c.py1 - c.py0);
    for (int k = 0; k < 3; ++k) { a.U[k] = a.cols ? c.X[k] : c.Y[k]; a.V[k] = a.cols ? c.Y[k] : c.X[k]; }
    a.n_outer = a.cols ? c.px1 - c.px0 : c.py1 - c.py0; a.n_inner = a.cols ? c.py1 - c.py0 : c.px1 - c.px0;
    a.u0c = (a.cols ? c.px0 : c.py0) * 256 + 128; a.v0c = (a.cols ? c.py0 : c.px0) * 256 + 128;
    return a;
}

struct Stream {
    std::mt19937_64 rng;
    int64_t centre_hi;                         // centres run from -20000 to 51424 past the target's far edge (1100000 at the default extent)
    explicit Stream(uint64_t seed, int64_t extent = 4096) : rng(seed), centre_hi(extent * 256 + 51424) {}
    int64_t uni(int64_t lo, int64_t hi) { return (int64_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); }

    // One draw; false: rejected (no area, too large, no pixel centre in the box, window beside the box) -- the draw still counts.
    bool draw(Case &c)
    {
        int32_t *X = c.X, *Y = c.Y;
        const int kind = c.kind = (int)uni(0, 9);
        const int32_t cx = (int32_t)uni(-20000, centre_hi), cy = (int32_t)uni(-20000, centre_hi);    // 24.8: around the target
        if (kind <= 4) {                                   // sliver: long, thin, any direction (what a noise terrain is made of)
            const double ang = (double)uni(0, 6283185) * 1e-6, len = (double)uni(256, 80000), wid = (double)uni(1, 400);
            const double dx = cos(ang), dy = sin(ang);
            X[0] = cx; Y[0] = cy;
            X[1] = cx + (int32_t)(len * dx); Y[1] = cy + (int32_t)(len * dy);
            X[2] = cx + (int32_t)(0.5 * len * dx - wid * dy); Y[2] = cy + (int32_t)(0.5 * len * dy + wid * dx);
            if (kind == 0) { X[1] = X[0]; }                // an edge exactly parallel to y
            if (kind == 1) { Y[1] = Y[0]; }                // ... to x
        } else if (kind <= 6) {                            // general triangle up to ~300 px
            for (int k = 0; k < 3; ++k) { X[k] = cx + (int32_t)uni(-40000, 40000); Y[k] = cy + (int32_t)uni(-40000, 40000); }
        } else if (kind == 7) {                            // vertices and edges through pixel centres (the top-left rule decides)
            for (int k = 0; k < 3; ++k) { X[k] = ((cx >> 8) + (int32_t)uni(-6, 6)) * 256 + 128; Y[k] = ((cy >> 8) + (int32_t)uni(-6, 6)) * 256 + 128; }
        } else if (kind == 8) {                            // small, sub-pixel scale
            for (int k = 0; k < 3; ++k) { X[k] = cx + (int32_t)uni(-600, 600); Y[k] = cy + (int32_t)uni(-600, 600); }
        } else {                                           // huge: extents just below the fast path's limit (2^24)
            for (int k = 0; k < 3; ++k) { X[k] = cx + (int32_t)uni(-8000000, 8000000); Y[k] = cy + (int32_t)uni(-8000000, 8000000); }
        }
        int64_t area2 = (int64_t)(X[1] - X[0]) * (Y[2] - Y[0]) - (int64_t)(Y[1] - Y[0]) * (X[2] - X[0]);
        if (area2 == 0) return false;
        if (area2 > 0) { std::swap(X[1], X[2]); std::swap(Y[1], Y[2]); }     // front-facing = negative area in y-down pixels
        const int32_t xmin = std::min(X[0], std::min(X[1], X[2])), xmax = std::max(X[0], std::max(X[1], X[2]));
        const int32_t ymin = std::min(Y[0], std::min(Y[1], Y[2])), ymax = std::max(Y[0], std::max(Y[1], Y[2]));
        if ((uint32_t)xmax - (uint32_t)xmin >= (1u << 24) || (uint32_t)ymax - (uint32_t)ymin >= (1u << 24)) return false;
        // a tile (or strip) window that meets the bounding box
        const int32_t bx0 = (xmin + 127) >> 8, bx1 = (xmax - 128) >> 8, by0 = (ymin + 127) >> 8, by1 = (ymax - 128) >> 8;
        if (bx0 > bx1 || by0 > by1) return false;
        const int32_t tw = (int32_t)(1 << uni(2, 6)), th = 64;
        c.tx_lo = (int32_t)uni(bx0 - tw + 1, bx1); c.ty_lo = (int32_t)uni(by0 - th + 1, by1);
        c.tx_hi = c.tx_lo + tw - 1; c.ty_hi = c.ty_lo + (int32_t)uni(0, th - 1);
        c.px0 = std::max(bx0, c.tx_lo); c.px1 = std::min(bx1, c.tx_hi); c.py0 = std::max(by0, c.ty_lo); c.py1 = std::min(by1, c.ty_hi);
        return c.px0 <= c.px1 && c.py0 <= c.py1;
    }
};

} // namespace raster_cases

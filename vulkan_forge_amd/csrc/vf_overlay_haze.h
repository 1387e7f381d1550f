// vf_overlay_haze.h -- point, line and contour overlay layers under the atmospheric haze.
//
// A hazed layer is a flag on its records (kOvHaze, vf_overlay.h).  On a frame of a handle whose haze is enabled with a density above
// zero, and that has a hazed layer, the overlay pass (overlay_pass, vf_hip.hip) launches behind k_ov_setup
//   k_ov_haze_setup          one thread per primitive: the side record (rw_a, rw_b - rw_a, yq_a or y_c, yq_b - yq_a or ah) of a hazed
//                            point (1/w and world height of its centre, and its haze opacity, which is the same at every pixel) or
//                            segment (1/w and y/w of its ends after clipping, both affine along the projected segment), zero for
//                            every other primitive
// and, in place of k_ov_composite / k_ov_composite_occlude,
//   k_ov_composite_haze<OCCLUDE>   ov_composite<OCCLUDE, true> (vf_overlay.h): the primitive that gives a feature its coverage at a
//                            pixel gives it its haze opacity too, haze_alpha (vf_haze.h) of its depth and height there, and the
//                            feature's colour is blended towards the haze colour by it before it goes over the pixel.
// Every other frame launches what it launched before these existed.  The arithmetic is the contract's, bit for bit
// (tests/overlay_haze_model/overlay_haze_model.c is its CPU statement), whatever the shade precision.  Templates only: the library's
// non-template kernels keep their places.
#pragma once
#include "vf_overlay.h"
#include "vf_haze.h"

namespace vf {

// vf_terrain_set_layer_haze: a point / line layer's records [lo, hi) gain or lose kOvHaze, in place
template <int UNUSED>
__global__ __launch_bounds__(256) void k_ov_haze_flag(uint32_t lo, uint32_t hi, OvIn *__restrict__ in, uint32_t on)
{
    const uint32_t i = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hi) return;
    OvIn &q = in[i];
    if ((q.flags & kOvKindMask) == kOvPoly) return;
    q.flags = on ? (q.flags | kOvHaze) : (q.flags & ~kOvHaze);
}

// k_ov_setup's clip step of a segment a -> b in clip space (z >= 0, then z <= w; the crossing from the inside vertex outwards) with
// the ends' world heights ya / yb carried along by the clipper's own t.  `keep` comes in as "both ends are
// finite"; false: nothing is left.  A restatement, not a function the two kernels share: calling one from k_ov_setup changed that
// kernel's instructions (4r, "Kernels"), and the frame tests hold both to the one CPU statement of the step.
__device__ __forceinline__ bool ov_clip_segment_y(float a[4], float b[4], bool keep, float &ya, float &yb)
{
    for (int plane = 0; plane < 2 && keep; ++plane) {
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
        if (ain) yb = fmaf(t, yb - ya, ya); else ya = fmaf(t, ya - yb, yb);
    }
    return keep;
}

// hz[i] of every primitive: the vertex stage is k_ov_setup's (ov_clip_y).  A primitive that k_ov_setup does not draw reaches no
// bin, so its record is never read.  A point's depth and height are its centre's at every pixel, so its opacity
// is formed here, once, and not per covered pixel in the composite: the same haze_alpha of the same two numbers.
template <int UNUSED>
__global__ __launch_bounds__(256) void k_ov_haze_setup(FrameParams P, AxisTables A, uint32_t nprims, const OvIn *__restrict__ in, float4 *__restrict__ hz,
                                                       HazeParams Z)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nprims) return;
    float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t flags = in[i].flags, kind = flags & kOvKindMask;
    if ((flags & kOvHaze) != 0u && kind != kOvPoly) {
        const OvIn q = in[i];
        const bool drape = (flags & kOvDrape) != 0u;
        float a[4];
        float ya = ov_clip_y(P, A, q.p0, drape, a);
        if (kind != kOvSegment) {
            if (finite4(a[0], a[1], a[2], a[3]) && a[3] > 0.0f && !(a[2] < 0.0f) && !(a[2] > a[3])) {
                const float rw = 1.0f / a[3];
                d = make_float4(rw, 0.0f, ya, haze_alpha(Z, 1.0f / rw, ya));
            }
        } else {
            float b[4];
            float yb = ov_clip_y(P, A, q.p1, drape, b);
            const bool keep = ov_clip_segment_y(a, b, finite4(a[0], a[1], a[2], a[3]) && finite4(b[0], b[1], b[2], b[3]), ya, yb);
            if (keep && a[3] > 0.0f && b[3] > 0.0f) {
                const float rwa = 1.0f / a[3], rwb = 1.0f / b[3];
                const float yqa = ya * rwa, yqb = yb * rwb;
                d = make_float4(rwa, rwb - rwa, yqa, yqb - yqa);
            }
        }
    }
    hz[i] = d;
}

// The composite of a frame that hazes overlay layers; OCCLUDE as k_ov_composite_occlude (a handle with an occluding layer): the
// other instantiation reads neither P, V, vis nor dep.
template <bool OCCLUDE>
__global__ __launch_bounds__(256) void k_ov_composite_haze(uint32_t W, uint32_t H, uint32_t nbx, const OvPrim *__restrict__ prims,
                                                           uint32_t *__restrict__ cnt, const uint32_t *__restrict__ start,
                                                           const uint32_t *__restrict__ list, const float *__restrict__ decode,
                                                           const float *__restrict__ thresh, const uint32_t *__restrict__ mask,
                                                           uint32_t *__restrict__ rgba, FrameParams P, SetupView V,
                                                           const uint32_t *__restrict__ vis, const float4 *__restrict__ dep,
                                                           const float4 *__restrict__ hz, HazeParams Z)
{
    __shared__ uint32_t keys[kOvSortCap];
    __shared__ OvPrim recs[256];
    __shared__ float4 side[OCCLUDE ? 512 : 256];                        // the haze records, then the occlusion records
    __shared__ float sdec[256], sthr[256];
    __shared__ uint32_t s_n, s_next;
    ov_composite<OCCLUDE, true, HazeParams>(W, H, nbx, prims, cnt, start, list, decode, thresh, mask, rgba, &P, &V, vis, dep, keys, recs,
                                            OCCLUDE ? side + 256 : nullptr, sdec, sthr, s_n, s_next, OvHazeArgs<true, HazeParams>{ &Z, hz, side });
}

} // namespace vf

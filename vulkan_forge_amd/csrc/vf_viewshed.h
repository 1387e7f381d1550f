// vf_viewshed.h -- viewshed analysis: what can be seen from a point of the terrain.
//
//   the viewshed field   one float per grid vertex, seen in [0, 1], from the displaced-height cache and an observer vertex: a prefix
//                        maximum of slopes along lines that fan out from the observer (Franklin's R2 rule with true distances), in
//                        the shadow scan's decoupled shape -- k_viewshed_chunk_max (the maximum of every 64-step chunk of every
//                        line), k_viewshed_carry (their exclusive running maximum along each line), k_viewshed_seen (the scan inside a
//                        chunk by DPP, seeded with the chunk's carry, the horizon test, and the store by the line that owns the vertex)
//   the tint pass        k_viewshed_tint<CLIPPED> blends a hidden and a visible colour over the covered pixels of a frame from its
//                        stored visibility, flat: it does not call the fragment function
//
// Launched only for a handle that asked for a viewshed or for the field: the frame path is not touched.  The arithmetic is the
// contract's, bit for bit (tests/viewshed_model/viewshed_model.c is its CPU statement): max is exact and associative, so the scan
// gives the sequential walk's bits however a line is cut; every term is formed from its own step.  All kernels are templates: the
// library's non-template kernels keep their places.
#pragma once
#include "vf_shadow.h"

namespace vf {

// The frame of reference of one field (the host fills it: viewshed_plan in vf_hip.hip).  Quadrant q = 0, 1: the major axis is x,
// towards higher / lower i; q = 2, 3: the major axis is z, towards higher / lower j.  Line l = c + L, c in [-L, L], holds at step
// k = 1, 2, ... the vertex at major offset k and minor offset r(k, c) = sgn(c) floor((2 k |c| + L) / (2 L)) from the observer.
struct ViewshedPlan {
    uint32_t n, nb;
    uint32_t io, jo;            // the observer's vertex
    uint32_t L;                 // n - 1
    uint32_t nlines, nchunks;   // 2 L + 1 lines, ceil(L / 64) chunks per quadrant
    uint32_t steps[4];          // steps that exist in each quadrant: n - 1 - io, io, n - 1 - jo, jo
    float exag, eye_height, target_height, softness, bias;
};

// minor offset of step k of line c = line - L (|r| <= k; it does not shrink with k: a line that has left the grid stays outside)
__device__ __forceinline__ int32_t vs_minor(const ViewshedPlan &V, uint32_t line, uint32_t k)
{
    const int32_t c = (int32_t)line - (int32_t)V.L;
    const uint32_t ac = (uint32_t)(c < 0 ? -c : c);
    const int32_t r = (int32_t)((2u * k * ac + V.L) / (2u * V.L));
    return c < 0 ? -r : r;
}

// the line that owns the vertex at major offset k >= 1 and minor offset m: c*(k, m) + L
__device__ __forceinline__ uint32_t vs_owner(const ViewshedPlan &V, uint32_t k, int32_t m)
{
    const uint32_t am = (uint32_t)(m < 0 ? -m : m);
    const int32_t c = (int32_t)((2u * am * V.L + k) / (2u * k));
    return (uint32_t)((int32_t)V.L + (m < 0 ? -c : c));
}

// step k of a line of quadrant q has a vertex: (i, j), and its minor offset r
__device__ __forceinline__ bool vs_vertex(const ViewshedPlan &V, uint32_t q, uint32_t line, uint32_t k, uint32_t &i, uint32_t &j, int32_t &r)
{
    if (line >= V.nlines || k > V.steps[q]) return false;
    r = vs_minor(V, line, k);
    const int32_t minor = (int32_t)(q < 2u ? V.jo : V.io) + r;
    if (minor < 0 || minor >= (int32_t)V.n) return false;
    const uint32_t major = (q & 1u) ? (q < 2u ? V.io : V.jo) - k : (q < 2u ? V.io : V.jo) + k;
    i = q < 2u ? major : (uint32_t)minor;
    j = q < 2u ? (uint32_t)minor : major;
    return true;
}

// the line still has a vertex at step k (then also at every step before it)
__device__ __forceinline__ bool vs_live(const ViewshedPlan &V, uint32_t q, uint32_t line, uint32_t k)
{
    uint32_t i, j;
    int32_t r;
    return vs_vertex(V, q, line, k, i, j, r);
}

// some line of the workgroup's 64 from l0 has a vertex at step k: the one nearest to c = 0 leaves the grid last
__device__ __forceinline__ bool vs_group_live(const ViewshedPlan &V, uint32_t q, uint32_t l0, uint32_t k)
{
    const uint32_t l1 = min(l0 + kShLines, V.nlines) - 1u;
    return vs_live(V, q, l1 < V.L ? l1 : l0 > V.L ? l0 : V.L, k);
}

__device__ __forceinline__ float vs_eye(const ViewshedPlan &V, const float *__restrict__ hblk) { return cached_height(hblk, V.nb, V.io, V.jo) * V.exag + V.eye_height; }

// y = h * exag of step k of a line and its distance D from the observer in cells; y = NaN where the line has no vertex (a non-finite
// y contributes nothing and is seen)
__device__ __forceinline__ float vs_height(const ViewshedPlan &V, const float *__restrict__ hblk, uint32_t q, uint32_t line, uint32_t k, float &D)
{
    uint32_t i, j;
    int32_t r;
    D = 1.0f;
    if (!vs_vertex(V, q, line, k, i, j, r)) return __builtin_nanf("");
    D = sqrtf((float)(k * k + (uint32_t)(r * r)));
    return cached_height(hblk, V.nb, i, j) * V.exag;
}

__device__ __forceinline__ float vs_term(float y, float y_eye, float D) { return isfinite(y) ? (y - y_eye) / D : -INFINITY; }

// seen of a step: y its height, D its distance, M the maximum of the terms of the steps before it on its line (-inf: none)
__device__ __forceinline__ float vs_seen(const ViewshedPlan &V, float y, float y_eye, float D, float M)
{
    if (!isfinite(y)) return 1.0f;
    const float s = ((y + V.target_height) - y_eye) / D;
    const float e = (M - s) * D;
    return 1.0f - fminf(fmaxf((e - V.bias) / V.softness, 0.0f), 1.0f);
}

// ---- the three stages of the scan, stated once ----
// Their bodies serve the single field's kernels below and the batched ones of vf_cumulative_viewshed.h, which wrap them: a wrapper
// decodes its plan and quadrant from the grid, passes the base of *that plan's* carries and, for the last stage, a sink that takes
// every value.  V comes by reference: a by-value kernel argument or a record in device memory.

// the carries of a plan, cmax[quadrant][chunk][line]: where those of chunk `chunk` of quadrant q begin
__device__ __forceinline__ size_t vs_carries(const ViewshedPlan &V, uint32_t q, uint32_t chunk) { return ((size_t)q * V.nchunks + chunk) * V.nlines; }

// Chunk (blockIdx.x) of 64 lines (blockIdx.y) of quadrant q: the maximum of each line's 64 terms -> out[line], out = the plan's
// cmax[q][chunk].  Lines that have left the grid by the chunk's first step are skipped (the other two stages skip them by the same
// test).
// ZMAJOR = false: memory runs along the steps -- lane = step, a wave reduces one line at a time.
// ZMAJOR = true: memory runs across the lines -- lane = line, each wave walks a quarter of the steps, the quarters meet in LDS.
template <bool ZMAJOR>
__device__ __forceinline__ void vs_stage_chunk_max(const ViewshedPlan &V, uint32_t q, const float *__restrict__ hblk, float *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t k0 = blockIdx.x * kShChunk + 1u, l0 = blockIdx.y * kShLines;
    if (!vs_group_live(V, q, l0, k0)) return;
    const float y_eye = vs_eye(V, hblk);
    if constexpr (ZMAJOR) {
        __shared__ float part[4][kShLines];
        float m = -INFINITY;
        for (uint32_t kk = wave; kk < kShChunk; kk += 4u) {
            float D;
            const float y = vs_height(V, hblk, q, l0 + lane, k0 + kk, D);
            m = fmaxf(m, vs_term(y, y_eye, D));
        }
        part[wave][lane] = m;
        __syncthreads();
        if (wave == 0u && l0 + lane < V.nlines)
            out[l0 + lane] = fmaxf(fmaxf(part[0][lane], part[1][lane]), fmaxf(part[2][lane], part[3][lane]));
    } else {
        for (uint32_t g = wave; g < kShLines; g += 4u) {
            const uint32_t line = l0 + g;
            if (line >= V.nlines) break;                       // (wave-uniform)
            if (!vs_live(V, q, line, k0)) continue;            // (wave-uniform)
            float D;
            const float y = vs_height(V, hblk, q, line, k0 + lane, D);
            float m = vs_term(y, y_eye, D);
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            if (lane == 0u) out[line] = m;
        }
    }
}

// quadrant 2 ZMAJOR + blockIdx.z
template <bool ZMAJOR>
__global__ __launch_bounds__(256) void k_viewshed_chunk_max(ViewshedPlan V, const float *__restrict__ hblk, float *__restrict__ cmax)
{
    const uint32_t q = (ZMAJOR ? 2u : 0u) + blockIdx.z;
    vs_stage_chunk_max<ZMAJOR>(V, q, hblk, cmax + vs_carries(V, q, blockIdx.x));
}

// per line of quadrant q: the chunk maxima -> the maximum of the chunks before each (in place, c = the plan's cmax[q]), one thread
// per line, as far as the line has vertices
__device__ __forceinline__ void vs_stage_carry(const ViewshedPlan &V, uint32_t q, float *__restrict__ c)
{
    const uint32_t line = blockIdx.x * 256u + threadIdx.x;
    if (line >= V.nlines) return;
    float run = -INFINITY;
    for (uint32_t k = 0; k < V.nchunks; ++k) {
        if (!vs_live(V, q, line, k * kShChunk + 1u)) break;
        const size_t o = (size_t)k * V.nlines + line;
        const float m = c[o];
        c[o] = run;
        run = fmaxf(run, m);
    }
}

// quadrant blockIdx.y
template <int UNUSED>
__global__ __launch_bounds__(256) void k_viewshed_carry(ViewshedPlan V, float *__restrict__ cmax)
{
    vs_stage_carry(V, blockIdx.y, cmax + vs_carries(V, blockIdx.y, 0u));
}

// lane = step k0 + lane of one line: its seen from its height y, its distance D and the line's carry into the chunk
__device__ __forceinline__ float vs_scan_seen(const ViewshedPlan &V, float y, float y_eye, float D, float carry)
{
    const uint32_t inc = wave_scan_max(sh_order(vs_term(y, y_eye, D)));        // terms of the chunk's steps up to and including this one
    const uint32_t before = __shfl_up(inc, 1u);                                // ... up to the one before
    const float M = (threadIdx.x & 63u) ? fmaxf(sh_unorder(before), carry) : carry;
    return vs_seen(V, y, y_eye, D, M);
}

// One writer per vertex: step k of a line of quadrant q writes its vertex (i, j), at minor offset r, only if the line owns it --
// c == c*(k, r), and a vertex on a diagonal belongs to the x-major quadrants.  False: no vertex there, or another line's.
__device__ __forceinline__ bool vs_owned(const ViewshedPlan &V, uint32_t q, uint32_t line, uint32_t k, uint32_t &i, uint32_t &j, int32_t &r)
{
    if (!vs_vertex(V, q, line, k, i, j, r)) return false;
    if (q >= 2u && (uint32_t)(r < 0 ? -r : r) >= k) return false;
    return vs_owner(V, k, r) == line;
}

// the store of step k of a line
__device__ __forceinline__ void vs_store(const ViewshedPlan &V, uint32_t q, uint32_t line, uint32_t k, float v, float *__restrict__ seen)
{
    uint32_t i, j;
    int32_t r;
    if (vs_owned(V, q, line, k, i, j, r)) seen[(size_t)j * V.n + i] = v;
}

// The observer's own vertex lies on no line: one thread of a plan's launches writes its 1 -- the first of quadrant 0's first workgroup
template <bool ZMAJOR>
__device__ __forceinline__ bool vs_writes_observer(uint32_t q) { return !ZMAJOR && blockIdx.x == 0u && blockIdx.y == 0u && q == 0u && threadIdx.x == 0u; }

// The scan inside chunk (blockIdx.x) of 64 lines (blockIdx.y) of quadrant q, seeded with in[line], in = the plan's carry[q][chunk]:
// sink(q, line, k, seen) for every step of a live line, those without a vertex or of another line's vertex among them (the sink asks
// vs_owned)
template <bool ZMAJOR, class Sink>
__device__ __forceinline__ void vs_stage_seen(const ViewshedPlan &V, uint32_t q, const float *__restrict__ hblk, const float *__restrict__ in, Sink sink)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t k0 = blockIdx.x * kShChunk + 1u, l0 = blockIdx.y * kShLines;
    if (!vs_group_live(V, q, l0, k0)) return;
    const float y_obs = cached_height(hblk, V.nb, V.io, V.jo) * V.exag;
    const float y_eye = y_obs + V.eye_height;
    const bool blind = !isfinite(y_obs);                       // an observer without a height: 1 wherever a value goes
    if constexpr (ZMAJOR) {
        // rows of the grid are contiguous across the lines: heights come in and seen goes out with lane = line, the scan runs with
        // lane = step, and the 64 x 64 tile changes hands in LDS (distances are formed again where they are used)
        __shared__ float tile[kShLines * kShPitch];
        for (uint32_t kk = wave; kk < kShChunk; kk += 4u) {
            float D;
            tile[lane * kShPitch + kk] = vs_height(V, hblk, q, l0 + lane, k0 + kk, D);
        }
        __syncthreads();
        for (uint32_t g = wave; g < kShLines; g += 4u) {
            const uint32_t line = l0 + g;
            const float c = vs_live(V, q, line, k0) ? in[line] : -INFINITY;
            const int32_t r = vs_minor(V, min(line, V.nlines - 1u), k0 + lane);
            const float D = sqrtf((float)((k0 + lane) * (k0 + lane) + (uint32_t)(r * r)));
            const float v = vs_scan_seen(V, tile[g * kShPitch + lane], y_eye, D, c);
            tile[g * kShPitch + lane] = blind ? 1.0f : v;
        }
        __syncthreads();
        for (uint32_t kk = wave; kk < kShChunk; kk += 4u) sink(q, l0 + lane, k0 + kk, tile[lane * kShPitch + kk]);
    } else {
        for (uint32_t g = wave; g < kShLines; g += 4u) {
            const uint32_t line = l0 + g;
            if (line >= V.nlines) break;                       // (wave-uniform)
            if (!vs_live(V, q, line, k0)) continue;            // (wave-uniform)
            float D;
            const float y = vs_height(V, hblk, q, line, k0 + lane, D);
            const float v = vs_scan_seen(V, y, y_eye, D, in[line]);
            sink(q, line, k0 + lane, blind ? 1.0f : v);
        }
    }
}

// quadrant 2 ZMAJOR + blockIdx.z
template <bool ZMAJOR>
__global__ __launch_bounds__(256) void k_viewshed_seen(ViewshedPlan V, const float *__restrict__ hblk, const float *__restrict__ carry,
                                                       float *__restrict__ seen)
{
    const uint32_t q = (ZMAJOR ? 2u : 0u) + blockIdx.z;
    if (vs_writes_observer<ZMAJOR>(q)) seen[(size_t)V.jo * V.n + V.io] = 1.0f;
    vs_stage_seen<ZMAJOR>(V, q, hblk, carry + vs_carries(V, q, blockIdx.x),
                          [&](uint32_t q_, uint32_t line, uint32_t k, float v) { vs_store(V, q_, line, k, v, seen); });
}

// ---- the tint pass (contract item 4) ----

struct ViewshedTint {
    const float *seen;          // the field, n x n
    const float *decode;        // 256 sRGB8 -> linear
    uint32_t visible_rgba, hidden_rgba;
    float xo, zo;               // the observer vertex's grid coordinates
    float RR;                   // (radius / spacing)^2
    uint32_t radius_on;         // 0: no radius, every covered pixel is treated
};

// c = t a + c (1 - a) with a = cov (alpha8 / 255), the overlay's blend; false: a is not > 0, nothing done
__device__ __forceinline__ bool vs_blend(float c[3], const float *dec, uint32_t rgba, float cov)
{
    const float a = cov * ((float)(rgba >> 24) / 255.0f);
    if (!(a > 0.0f)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = dec[(rgba >> (8 * k)) & 255u] * a + c[k] * (1.0f - a);
    return true;
}

// The end of a depth tint (the flood's water, vf_flood.h; the spill's sinks, vf_spill.h): `shallow` and `deep` over the colour `rgba`,
// the deep one by min(d / depth_full, 1) and the shallow one by the rest; false: neither has an opacity, `rgba` is left
__device__ __forceinline__ bool vs_depth_tint(const float *dec, const float *thr, float d, float depth_full, uint32_t shallow, uint32_t deep, uint32_t &rgba)
{
    const float sd = fminf(d / depth_full, 1.0f);
    float c[3] = { dec[rgba & 255u], dec[(rgba >> 8) & 255u], dec[(rgba >> 16) & 255u] };
    const bool sh = vs_blend(c, dec, shallow, 1.0f - sd);
    const bool dp = vs_blend(c, dec, deep, sd);
    if (!sh && !dp) return false;
    rgba = srgb_encode(c[0], thr) | (srgb_encode(c[1], thr) << 8) | (srgb_encode(c[2], thr) << 16) | 0xFF000000u;
    return true;
}

// Pixel (px, py) with visibility id `id` and colour `rgba`: false when the pass leaves it as the frame drew it
template <bool CLIPPED>
__device__ __forceinline__ bool viewshed_pixel(const FrameParams &P, const SetupView &V, const ViewshedTint &T, const float *dec, const float *thr,
                                               uint32_t id, int32_t px, int32_t py, uint32_t &rgba)
{
    const uint32_t prim = id - 1u;
    const VisibleSite s = visible_site<CLIPPED>(P, V, prim);
    const float f0 = T.seen[site_vertex(P, s, 0)], f1 = T.seen[site_vertex(P, s, 1)], f2 = T.seen[site_vertex(P, s, 2)];
    const bool plain = f0 == 1.0f && f1 == 1.0f && f2 == 1.0f;
    float sn = 1.0f;
    if (!plain || T.radius_on) {
        const VisiblePoint<CLIPPED> p = visible_point<CLIPPED>(P, V, s, prim, px, py);
        if (T.radius_on) {
            float attr[3];
            point_varyings(P, p, px, py, attr);
            const float dx = attr[1] - T.xo, dz = attr[2] - T.zo;
            const float d2 = dx * dx + dz * dz;
            if (!(d2 <= T.RR)) return false;
        }
        if (!plain) sn = fminf(fmaxf(point_scalar(P, p, px, py, f0, f1, f2), 0.0f), 1.0f);
    }
    float c[3] = { dec[rgba & 255u], dec[(rgba >> 8) & 255u], dec[(rgba >> 16) & 255u] };
    const bool hid = vs_blend(c, dec, T.hidden_rgba, 1.0f - sn);
    const bool vis = vs_blend(c, dec, T.visible_rgba, sn);
    if (!hid && !vis) return false;
    rgba = srgb_encode(c[0], thr) | (srgb_encode(c[1], thr) << 8) | (srgb_encode(c[2], thr) << 16) | 0xFF000000u;
    return true;
}

// The body of a tint kernel of 256 threads (this one's, k_flood_tint, k_spill_tint): the frame's visibility (H, W) -> the covered
// pixels of its colour buffer, each as pixel(dec, thr, id, px, py, colour) leaves it (false: as the frame drew it), in the walk of
// for_each_visible (vf_visible.h), with the two sRGB tables in LDS.  `redo` as for k_relight: both instantiations are launched
// behind a frame and the one the frame does not call for leaves at once.
template <bool CLIPPED, typename Pixel>
__device__ __forceinline__ void tint_visible(const FrameParams &P, const float *__restrict__ thresh, const float *__restrict__ decode,
                                             const uint32_t *__restrict__ vis, const uint32_t *__restrict__ redo, uint32_t *__restrict__ rgba, Pixel &&pixel)
{
    if ((*redo != 0u) != CLIPPED) return;
    __shared__ float s_thr[256];
    __shared__ float s_dec[256];
    s_thr[threadIdx.x] = thresh[threadIdx.x];
    s_dec[threadIdx.x] = decode[threadIdx.x];
    __syncthreads();
    for_each_visible(P, vis, [&](uint32_t id, uint32_t px, uint32_t py) {
        if (id == 0u) return;
        const size_t o = (size_t)py * P.W + px;
        uint32_t c = rgba[o];
        if (pixel(s_dec, s_thr, id, (int32_t)px, (int32_t)py, c)) rgba[o] = c;
    });
}

template <bool CLIPPED>
__global__ __launch_bounds__(256) void k_viewshed_tint(FrameParams P, SetupView V, const float *__restrict__ thresh, const uint32_t *__restrict__ vis,
                                                       ViewshedTint T, const uint32_t *__restrict__ redo, uint32_t *__restrict__ rgba)
{
    tint_visible<CLIPPED>(P, thresh, T.decode, vis, redo, rgba, [&](const float *dec, const float *thr, uint32_t id, int32_t px, int32_t py, uint32_t &c) {
        return viewshed_pixel<CLIPPED>(P, V, T, dec, thr, id, px, py, c);
    });
}

} // namespace vf

// vf_hip.hip -- C-ABI (include/vf_hip.h) over the gfx950 kernels in vf_kernels.h.
// Built by __graft_entry__.build():  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC + the -mllvm code-generation switches of HIPCC_TUNING
#include "../../include/vf_hip.h"
#include "vf_kernels.h"
#include "vf_overlay.h"     // (brings vf_contour.h)
#include "vf_gbuffer.h"     // templates only, behind the last non-template kernel
#include "vf_shadow.h"      // templates only
#include "vf_ambient.h"     // templates only
#include "vf_drape.h"       // templates only
#include "vf_relight.h"     // templates only: the shade pass of the three
#include "vf_viewshed.h"    // templates only
#include "vf_cumulative_viewshed.h"   // templates only
#include "vf_sun_exposure.h"          // templates only
#include "vf_resolve.h"               // templates only
#include "vf_haze.h"                  // templates only
#include "vf_overlay_haze.h"          // templates only
#include "vf_flood.h"                 // templates only
#include "vf_spill.h"                 // templates only
#include "vf_line_loop.h"

#include <algorithm>
#include <cmath>
#include <vector>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <functional>
#include <new>
#include <string>
#include <atomic>
#include <memory>
#include <mutex>
#include <thread>
#include <dlfcn.h>
#include <sys/mman.h>
#include <rccl/rccl.h>     // types only: the functions are resolved at run time (resolve_rccl)

using namespace vf;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#define VF_HIP_TRY(expr)                                                                           \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(VF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)

double eotf_d(double s) { return s <= 0.04045 ? s / 12.92 : std::pow((s + 0.055) / 1.055, 2.4); }

struct SrgbTables {
    float decode[256];
    float thresh[256];
    SrgbTables()
    {
        for (int k = 0; k < 256; ++k) {
            decode[k] = (float)eotf_d((double)k / 255.0);
            thresh[k] = k == 0 ? -INFINITY : (float)eotf_d(((double)k - 0.5) / 255.0);
        }
    }
    uint32_t encode(float c) const
    {
        uint32_t k = 0;
        while (k < 255 && c >= thresh[k + 1]) ++k;
        return k;
    }
};
const SrgbTables &tables()
{
    static const SrgbTables t;
    return t;
}

bool is_pow2(uint32_t v) { return v && !(v & (v - 1)); }
// Tile-shard layouts are passed as one word, `skew | stripe_log2 << 16` (include/vf_hip.h, VF_TILE_LAYOUT): tile (tx, ty) belongs
// to rank ((tx >> stripe_log2) + skew * ty) % nranks.
uint32_t layout_skew(uint32_t layout) { return layout & 0xFFFFu; }
uint32_t layout_shift(uint32_t layout) { return (layout >> 16) & 0xFu; }
// Round 5: a layout word with bit 20 set names a REGISTERED stripe map (vf_tile_layout_register_map): an explicit owner per column
// stripe instead of the round-robin rule -- what a load-balanced deal of the stripes needs (vf_balance_stripes).  Bits 21..26: the
// map's number in the process-wide registry below; skew 0 by construction (column stripes).  Maps are immutable once registered.
constexpr uint32_t kLayoutMapBit = 1u << 20, kMaxStripeMaps = 64, kMaxStripes = 256;
struct StripeMap { std::vector<uint8_t> owner; uint32_t shift = 0, nranks = 0; };
std::mutex g_maps_mu;
std::vector<StripeMap> g_maps;                              // (entries are never removed or changed: a pointer into it stays valid ... while the vector does not grow:
const StripeMap *layout_map(uint32_t layout)                //  so it is reserved to its final capacity at the first registration)
{
    if (!(layout & kLayoutMapBit)) return nullptr;
    std::lock_guard<std::mutex> lk(g_maps_mu);
    const uint32_t id = (layout >> 21) & 0x3Fu;
    return id < g_maps.size() ? &g_maps[id] : nullptr;
}
bool layout_valid(uint32_t layout)
{
    if (layout & kLayoutMapBit) {
        const StripeMap *m = layout_map(layout);
        return m && (layout >> 27) == 0u && layout_skew(layout) == 0u && layout_shift(layout) == m->shift;
    }
    return (layout >> 20) == 0u;                            // skew < 65536, stripe_log2 <= 15, nothing above
}
// owner of tile (tx, ty) under a layout word (valid, see above)
uint32_t layout_owner(uint32_t layout, const StripeMap *m, uint32_t tx, uint32_t ty, uint32_t nranks)
{
    if (m) { const uint32_t sc = tx >> m->shift; return sc < m->owner.size() ? m->owner[sc] : 0u; }
    return ((tx >> layout_shift(layout)) + layout_skew(layout) * ty) % nranks;
}
uint32_t ilog2(uint32_t v)
{
    uint32_t s = 0;
    while ((1u << s) < v) ++s;
    return s;
}

} // namespace

// Page-locked host memory.  hipHostMalloc takes 7-9 ms for a C4 frame (64 MiB), the first copy into it another 11-16, hipHostFree 5:
// the runtime faults the buffer in 4 KiB page by page.  The same bytes as 2 MiB-aligned ordinary memory with MADV_HUGEPAGE, then
// hipHostRegister: 2.5-2.8 ms to make, copies at full rate (1.19 ms) from the first one, 2.5 ms to free (tools/micro/pin_cost.hip,
// round 5) -- cheaper than the page faults of ONE copy into fresh ordinary memory (4.4-4.9 ms), so even a one-shot caller's only
// read-back goes into such a buffer.  Small buffers and hosts without huge pages: hipHostMalloc.
struct PinnedRegistry {
    std::mutex mu;
    std::vector<void *> registered;                            // made by pinned_alloc's huge-page branch (freed by unregister + free)
    static PinnedRegistry &get() { static PinnedRegistry *r = new PinnedRegistry; return *r; }
};
static hipError_t pinned_alloc(void **out, size_t n)
{
    constexpr size_t kHuge = (size_t)2 << 20;
    *out = nullptr;
    if (n >= 2 * kHuge) {
        void *p = nullptr;
        const size_t r = (n + kHuge - 1) & ~(kHuge - 1);
        if (posix_memalign(&p, kHuge, r) == 0) {
            (void)madvise(p, r, MADV_HUGEPAGE);                 // (refused or unavailable: ordinary pages, still correct)
            if (hipHostRegister(p, r, hipHostRegisterDefault) == hipSuccess) {
                std::lock_guard<std::mutex> lk(PinnedRegistry::get().mu);
                PinnedRegistry::get().registered.push_back(p);
                *out = p;
                return hipSuccess;
            }
            (void)hipGetLastError();
            std::free(p);
        }
    }
    return hipHostMalloc(out, n, hipHostMallocDefault);
}
static void pinned_free(void *p)
{
    if (!p) return;
    bool ours = false;
    {
        PinnedRegistry &R = PinnedRegistry::get();
        std::lock_guard<std::mutex> lk(R.mu);
        auto it = std::find(R.registered.begin(), R.registered.end(), p);
        if (it != R.registered.end()) { R.registered.erase(it); ours = true; }
    }
    if (ours) { (void)hipHostUnregister(p); std::free(p); }
    else (void)hipHostFree(p);
}

struct vf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipDeviceProp_t prop;
    float *d_decode = nullptr;   // 256 sRGB8 -> linear (SrgbTables::decode), the head of the one allocation that holds both tables
    float *d_thresh = nullptr;   // 256 sRGB store thresholds, behind it
    // Streams the handles of this context borrow, made on first need: a stream costs 3-10 ms to create and 2-3 ms to destroy on this
    // runtime (round 5, measured), so they belong to the process-lifetime context, not to every handle.  side / side2: a frame's plan
    // chain and set-up pass (they overlap the previous frame's tile kernel; a handle's first frame needs neither); copy: batch read-back.
    // Handles that render at the same time share them: order is kept by events, sharing only serialises their plan chains.
    hipStream_t side = nullptr, side2 = nullptr, copy = nullptr;
    uint8_t *d_maps = nullptr;   // [kMaxStripeMaps][kMaxStripes] owner tables of the registered stripe maps, uploaded on first use (vf_stitch_tiles_device)
    uint64_t maps_uploaded = 0;  // bit k: map k is there
    // The members above that are made on first need are shared by every handle of the context, and the drop-in module keeps ONE context
    // and releases the GIL while it renders: two objects drawing their second frames on two threads would both find `side` missing.
    std::mutex lazy_mu;
};

// the context's plan streams, made once (3-10 ms each), under the context's lock
static hipError_t ctx_side_streams(vf_ctx *c, hipStream_t *side, hipStream_t *side2)
{
    std::lock_guard<std::mutex> lk(c->lazy_mu);
    hipError_t e = hipSuccess;
    if (!c->side) e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
    if (e == hipSuccess && !c->side2) e = hipStreamCreateWithFlags(&c->side2, hipStreamNonBlocking);
    *side = c->side; *side2 = c->side2;
    return e;
}
static hipError_t ctx_copy_stream(vf_ctx *c, hipStream_t *copy)
{
    std::lock_guard<std::mutex> lk(c->lazy_mu);
    hipError_t e = hipSuccess;
    if (!c->copy) e = hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking);
    *copy = c->copy;
    return e;
}

// What the second half of a frame (draw_frame) needs of the first (plan_frame)
struct FramePlan {
    FrameParams P;
    uint32_t set = 0, ntiles = 0;
    uint32_t mode = 0;                                           // VF_PLAN_* bits: how plan_frame planned it (vf_terrain_debug_plan_mode)
    bool motion_starts = false;
    bool sampled = true;                                         // timing level 3: this frame is one of those that carry events
    uint32_t *rc_lo = nullptr, *rc_hi = nullptr, *seg_count = nullptr;
    bool lists = false;                                          // the tile kernel reads this plan state's per-tile candidate lists (k_tile_lists)
};

// A device array that grows (the overlay state).  reserve: when need > cap, a new allocation of new_cap elements, zero-filled on request,
// with the first `keep` elements copied over; the old one is freed only when all of that has succeeded -- a failure frees the new one and
// leaves the array as it was.
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t need, size_t new_cap, size_t keep = 0, bool zero = false)
    {
        if (need <= cap) return hipSuccess;
        T *q = nullptr;
        hipError_t e = hipMalloc(&q, new_cap * sizeof(T));
        if (e == hipSuccess && zero) e = hipMemset(q, 0, new_cap * sizeof(T));
        if (e == hipSuccess && keep) e = hipMemcpy(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            if (q) (void)hipFree(q);
            return e;
        }
        release();
        p = q; cap = new_cap;
        return hipSuccess;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
};

// A per-vertex analysis field of a handle with its cache ("The field cache"): when `valid`, d holds the field of `key`
// and of the heights generation `height_gen`.  The key: the bit patterns of everything beside the heights that the field is computed
// from, in an order the feature fixes, the lengths of its lists among them.  Keys compare bit for bit: -0 is not +0, a NaN equals itself.
struct VertexField {
    DevBuf<float> d;                     // n x n, row-major
    bool valid = false;
    uint64_t height_gen = 0;
    std::vector<uint32_t> key;
    uint32_t scans = 0;                  // times the field was computed (the vf_terrain_debug_*_scans calls)
    // *current: d holds the field of `k` and the handle's heights, and force is not set.  Otherwise d is ready to be computed: allocated
    // (nomem: the feature's message when that fails) and not valid until computed(), so launches that fail leave no field behind.
    int prepare(const vf_terrain *t, const std::vector<uint32_t> &k, bool force, const char *nomem, bool *current);
    void computed(const vf_terrain *t, std::vector<uint32_t> &k);   // the launches are queued: d is the field of `k` (which is taken)
    void release() { d.release(); valid = false; }                  // the buffer goes, the count stays
};

// A per-vertex field that is a sum over a list, batch by batch: the scans of a batch add q = rint(term * 65536) to
// d_sum, k_sum_finish turns the sums into `value` and into d_frac, which the tint pass reads between low_rgba and high_rgba.  The
// feature that holds one keeps what is its own: the list, the key, the batch size rule, the carries and the launches of a batch.
struct SummedField {
    uint32_t high_rgba, low_rgba;        // r | g << 8 | b << 16 | a << 24
    SummedField(uint32_t high, uint32_t low) : high_rgba(high), low_rgba(low) {}    // (the feature's defaults)
    VertexField value;                  // sum / 65536; the feature states its key
    DevBuf<uint32_t> d_sum;              // n x n sums of q
    DevBuf<float> d_frac;                // n x n: min(value / total, 1)
    uint32_t forced_batch = 0;           // the feature's vf_terrain_debug_*_batch call; 0: from the memory budget
    uint32_t batch = 0;                  // the batch size of the last computation
    int reserve(const vf_terrain *t, const char *nomem);            // d_sum and d_frac (value: by its prepare)
    hipError_t zero(const vf_terrain *t, hipStream_t s);            // queue d_sum = 0
    // queue k_sum_finish with `total`; then value is the field of `key` (which is taken), computed in batches of `B`
    int finish(const vf_terrain *t, hipStream_t s, float total, std::vector<uint32_t> &key, uint32_t B);
    // k_viewshed_tint on d_frac, with no radius: every covered pixel is treated
    int tint(const vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba) const;
    void release() { value.release(); d_sum.release(); d_frac.release(); }
    void force_batch(uint32_t b)
    {
        if (forced_batch != b) value.valid = false;                 // (the next call computes the field again, with this batch size)
        forced_batch = b;
    }
    void colours(uint8_t high[4], uint8_t low[4]) const
    {
        for (int k = 0; k < 4; ++k) { high[k] = (uint8_t)(high_rgba >> (8 * k)); low[k] = (uint8_t)(low_rgba >> (8 * k)); }
    }
};
// A feature struct with a SummedField `sum`, its other buffers released: gone, as if the handle never asked (the caller has
// synchronised); the scan counter and a forced batch size stay
template <typename Feature> static void summed_reset(Feature &H)
{
    H.sum.release();
    const uint32_t scans = H.sum.value.scans, forced = H.sum.forced_batch;
    H = Feature();
    H.sum.value.scans = scans; H.sum.forced_batch = forced;
}

// A per-vertex field that spreads from sources over the height field, pass by pass to a fixpoint, and is shown as a depth tint
// (DESIGN.md 4s, 4t): what the flood and the spill share.  The feature that holds one keeps what is its own: further inputs, its
// working buffers, its kernels and counts, and the words of its refusals.
struct SeededFill {
    // Passes queued per read-back of their `changed` words.  16: at grid 4096 the fastest of 1, 4 and 16 on both probes of DESIGN.md 4s
    // and on 4t's (a read-back costs more than a dozen passes that find nothing to do)
    static constexpr uint32_t kGroup = 16, kMaxGroup = 64;
    static constexpr int kSeeds = 2;     // the mode of a seed list (VF_FLOOD_SEEDS, VF_SPILL_SEEDS)
    bool enabled = false, have = false;  // have: the feature's set call has stored its inputs
    int mode;
    std::vector<float> xz;               // mode kSeeds: the seeds in the overlays' world frame, (x, z) each; else empty
    uint32_t shallow_rgba, deep_rgba;    // r | g << 8 | b << 16 | a << 24
    float depth_full;
    SeededFill(int mode0, uint32_t shallow, uint32_t deep, float full) : mode(mode0), shallow_rgba(shallow), deep_rgba(deep), depth_full(full) {}   // (the feature's defaults)
    VertexField field;                   // the feature states what stands in front of key_tail
    DevBuf<uint32_t> d_seeds;            // the seeds' vertices
    DevBuf<uint32_t> d_ctl;              // kMaxGroup `changed` words, then the feature's counts
    std::vector<uint32_t> ij;            // the host's copy of d_seeds (the source of its upload)
    uint32_t forced_group = 0;           // the feature's vf_terrain_debug_*_group call; 0: kGroup
    uint32_t passes = 0;                 // of the last computation
    struct Words { int modes; const char *unknown_mode, *count, *sharded; };   // the feature's modes (bit m: mode m is one), the words of its refusals
    // What a set call does once its own arguments are in order: the checks on depth_full, the mode and the seed list, the refusal of a
    // sharded handle, the wait for the frame in flight, the visibility buffer, the values stored.  other_changed: an input of the
    // feature's own differs from the one held (the caller stores it afterwards).
    int set(vf_terrain *t, int enable, int new_mode, const float *seeds_xz, uint32_t count, const uint8_t shallow[4], const uint8_t deep[4], float full,
            bool other_changed, const Words &W);
    // the seeds' vertices (i, j) for the spacing of the uniforms `u`, snapped as the viewshed's observer is
    std::vector<uint32_t> vertices(const vf_terrain *t, const float *u) const;
    int read_seeds(const vf_terrain *t, uint32_t *out, const char *none) const;      // the same for the live uniforms, to a caller
    // the end of the field's key: the mode, the length of the vertex list, the vertices (which are returned)
    std::vector<uint32_t> key_tail(const vf_terrain *t, const float *u, std::vector<uint32_t> &key) const
    {
        std::vector<uint32_t> v = vertices(t, u);
        key.push_back((uint32_t)mode); key.push_back((uint32_t)v.size());
        key.insert(key.end(), v.begin(), v.end());
        return v;
    }
    hipError_t reserve(size_t counts, size_t nseeds) { const hipError_t e = d_ctl.reserve(kMaxGroup + counts, kMaxGroup + counts); return e != hipSuccess ? e : d_seeds.reserve(nseeds, nseeds); }
    hipError_t upload(std::vector<uint32_t> &v, hipStream_t s)     // v (taken) -> d_seeds (a pageable source: returns when the copy is staged)
    {
        ij.swap(v);
        return hipMemcpyAsync(d_seeds.p, ij.data(), ij.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    }
    uint32_t *counts() const { return d_ctl.p + kMaxGroup; }
    uint32_t group() const { return std::min(forced_group ? forced_group : kGroup, kMaxGroup); }
    // The loop to the fixpoint: groups of passes, each pass with its own `changed` word, until the first pass that changed nothing;
    // *count: that pass's number.  queue(p, changed) queues pass p = 1, 2, ... on `s`.  A pass that changes something changes at least
    // one of nv vertices for good, so pass nv + 1 is not reached: `unreached` is the feature's refusal should it be.
    template <typename Queue> int fixpoint(hipStream_t s, size_t nv, const char *unreached, uint32_t *count, Queue &&queue) const
    {
        const uint32_t G = group();
        uint32_t changed[kMaxGroup], n = 0;
        for (bool done = false; !done && n <= nv;) {
            VF_HIP_TRY(hipMemsetAsync(d_ctl.p, 0, G * sizeof(uint32_t), s));
            for (uint32_t g = 0; g < G; ++g) queue(n + g + 1u, d_ctl.p + g);
            VF_HIP_TRY(hipGetLastError());
            VF_HIP_TRY(hipMemcpyAsync(changed, d_ctl.p, G * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            VF_HIP_TRY(hipStreamSynchronize(s));
            for (uint32_t g = 0; g < G && !done; ++g, ++n) done = changed[g] == 0u;
        }
        if (n > nv) return fail(VF_ERR_HIP, unreached);
        *count = n;
        return VF_OK;
    }
    int force_group(uint32_t g)
    {
        if (g > kMaxGroup) return fail(VF_ERR_INVALID, "a group holds at most 64 passes");
        if (forced_group != g) field.valid = false;                 // (the next call computes the field again, with this group size)
        forced_group = g;
        return VF_OK;
    }
    template <typename Info> void info(Info *out) const             // what vf_flood_info and vf_spill_info name alike
    {
        out->enabled = enabled ? 1 : 0; out->mode = mode; out->count = (uint32_t)(xz.size() / 2u); out->depth_full = depth_full;
        for (int k = 0; k < 4; ++k) { out->shallow_rgba[k] = (uint8_t)(shallow_rgba >> (8 * k)); out->deep_rgba[k] = (uint8_t)(deep_rgba >> (8 * k)); }
        out->passes = passes; out->scans = field.scans; out->group = group();
    }
    void release() { field.release(); d_seeds.release(); d_ctl.release(); }
};
// A feature struct with a SeededFill `fill`, its other buffers released: gone, as if the handle never asked (the caller has
// synchronised); the scan counter and a forced group size stay
template <typename Feature> static void fill_reset(Feature &H)
{
    H.fill.release();
    const uint32_t scans = H.fill.field.scans, forced = H.fill.forced_group;
    H = Feature();
    H.fill.field.scans = scans; H.fill.forced_group = forced;
}
static uint32_t key_bits(float f) { uint32_t w; std::memcpy(&w, &f, sizeof w); return w; }
static std::vector<uint32_t> key_of(std::initializer_list<float> fs)
{
    std::vector<uint32_t> k;
    for (float f : fs) k.push_back(key_bits(f));
    return k;
}

// Diagnostics: the mean time in ms of `repeats` back-to-back launches on `s`, between two events behind one warm-up launch.
// launch(warm) queues one launch and returns its error; the first error ends the measurement and is returned.
template <typename F> static hipError_t time_launches(hipStream_t s, uint32_t repeats, float &ms, F &&launch)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t err = hipEventCreate(&e0);
    if (err == hipSuccess) err = hipEventCreate(&e1);
    if (err == hipSuccess) err = launch(true);
    if (err == hipSuccess) err = hipEventRecord(e0, s);
    for (uint32_t k = 0; k < repeats && err == hipSuccess; ++k) err = launch(false);
    if (err == hipSuccess) err = hipEventRecord(e1, s);
    if (err == hipSuccess) err = hipEventSynchronize(e1);
    float total = 0.0f;
    if (err == hipSuccess) err = hipEventElapsedTime(&total, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    ms = total / (float)repeats;
    return err;
}

// What plan_frame advances from frame to frame.  A plan queued ahead of its call and then thrown away puts the handle back by
// assigning a saved copy (vf_terrain::PrePlan, drop_preplan); so does the diagnostic frame of render_visibility for the motion part.
struct PlanCursor {
    uint32_t cur_set = 0;                // the plan state the next frame takes
    uint32_t frame_no = 0;
    uint32_t frames_since_reset = 0;     // frames planned since create / set_shard (the feedback arrays were cleared then)
    bool have_drawn = false, camera_moving = false, was_moving = false;
    float u_drawn[32] = {};              // view + proj of the frame planned last (is the camera moving?)
};

// What the caller sets and a frame is drawn from
struct FrameInputs {
    float u[44] = {};                    // the uniform block
    uint32_t shade_mode = 0;             // VF_SHADE_REFERENCE / VF_SHADE_SPEC_T32
    uint32_t precision = VF_PRECISION_FAST;   // fragment arithmetic
};

// Which instantiation of the tile kernel draws the frames -- with or without line groups in the raster's line loop (vf_kernels.h,
// raster_fast) -- is measured, like the frame plan: which one is faster depends on what the camera shows and on how the frame is
// cut (C4: groups -7 % on the top-down camera at any rank count, -1.5 % on one GPU at the default camera, +5 % on a rank of eight,
// whose items are narrow strips).  Never a difference in the picture.  The schedule and the decision: vf_line_loop.h.
struct LineLoop {
    int mode = -1;                       // -1 measure and choose, 0 / 1 fixed (vf_terrain_set_raster_groups)
    // A probe = two events around a frame's kernels on the draw stream (k_clear + the tile launches); a sample = the time between them.
    // (Round 4 sampled the frame PERIOD between two consecutive frames of one variant, in runs AAABBB: right for a camera at rest, but a
    //  moving camera's frames differ in cost by +-20 % from pose to pose and a run of three A's sat on other poses than the B's -- on the
    //  C5 orbit the handle kept the slower variant in the bench, 0.326 instead of 0.305 ms per pose.  Round 5: every probed frame is a
    //  sample of its own, the variants alternate ABBA ABBA ..., so any linear drift of the cost over the window cancels exactly.)
    struct Probe { hipEvent_t a = nullptr, b = nullptr; int variant = 0; uint32_t epoch = 0; bool pending = false; } probes[16];
    uint32_t head = 0, epoch_id = 0;
    float ms[2] = { 0.0f, 0.0f };        // frame period with each variant in this epoch (mean of the samples taken)
    uint32_t n[2] = { 0u, 0u };
    uint32_t epoch_frames = 0;           // frames since the epoch began (shard change, height upload, camera jump)
    int now = 1;                         // the variant of the frame rendered last

    // A new epoch: what was measured belongs to other heights, another layout or mode, or to the view before the camera started to
    // move.  (Samples of probes still in flight carry the old epoch's number and are dropped when they complete.)
    void reset()
    {
        epoch_frames = 0; epoch_id++;
        n[0] = n[1] = 0; ms[0] = ms[1] = 0.0f;
    }
    // probes that have completed (frames behind us: never a wait): every probed frame is a sample -- the time its kernels took on
    // the draw stream.  (hipEventQuery's "not ready" is cleared here: the plan launches' errors were collected by plan_frame.)
    void harvest()
    {
        for (Probe &g : probes)
            if (g.pending && hipEventQuery(g.b) == hipSuccess) {
                g.pending = false;
                float t = 0.0f;
                if (g.epoch == epoch_id && hipEventElapsedTime(&t, g.a, g.b) == hipSuccess && t > 0.0f) {
                    // the probe window's samples count alike; a later look weighs as much as all before it (the view may have drifted)
                    const uint32_t k = ++n[g.variant];
                    ms[g.variant] += (t - ms[g.variant]) / (float)(k <= 8u ? k : 2u);
                }
            }
        (void)hipGetLastError();
    }
    // The variant of this frame and whether it is probed.  guess: the variant by default; restart: what was measured describes another
    // layout or the view before the camera started to move (a camera that keeps moving keeps its choice and is looked at again).
    LoopPick choose(int guess, bool restart, bool has_tiles)
    {
        uint32_t e = 0;
        if (mode < 0) {
            harvest();
            if (restart) reset();
            e = epoch_frames++;
        }
        const LoopPick pick = line_loop_pick(mode, e, guess, ms, n, has_tiles);
        now = pick.variant;
        return pick;
    }
    // the first event of a probed frame, in front of its kernels on `s`; nullptr: the frame goes unmeasured (ring full, no events)
    Probe *arm(hipStream_t s)
    {
        Probe *g = &probes[head++ % 16];
        if (g->pending) return nullptr;
        if (!g->b && (hipEventCreate(&g->a) != hipSuccess || hipEventCreate(&g->b) != hipSuccess)) return nullptr;   // (made on first use: a one-shot handle never probes)
        if (!g->a || !g->b) return nullptr;
        (void)hipEventRecord(g->a, s);
        return g;
    }
    // ... and the second one, behind them
    void close(Probe *g, hipStream_t s)
    {
        (void)hipEventRecord(g->b, s);
        g->variant = now; g->epoch = epoch_id; g->pending = true;
    }
};

struct vf_terrain {
    vf_ctx *ctx = nullptr;
    uint32_t W = 0, H = 0, n = 0;        // W, H: the RASTER size -- what the terrain is drawn at, and with it the visibility, the tiles, the plan and every pass over them
    // Supersampling.  ss = 1: the raster is the frame, oW = W, oH = H, no sample buffer, nothing below is launched.
    // ss > 1: W = ss oW, H = ss oH; the terrain passes draw into d_samples, k_ss_resolve makes the oW x oH frame in d_rgba from it and the
    // overlays composite onto that.  d_rgba, its read-backs and the overlay pass deal in oW x oH, everything else in W x H.
    uint32_t ss = 1, oW = 0, oH = 0;
    uint32_t *d_samples = nullptr;       // ss > 1 only (in the slab): whole tiles of the raster
    uint32_t nb = 0, nblocks = 0;        // 8x8-cell blocks per side / in total
    uint32_t ntx = 0, nty = 0;           // 64x64 screen tiles
    // shard
    uint32_t rank = 0, nranks = 1, band_h = kTileH, local_rows = 0, skew = 0;
    uint32_t local_tiles = 0;            // tiles this handle renders (= ntx * local tile rows unless tile-sharded)
    uint32_t *d_tile_map = nullptr;      // tile shards: local tile -> tx | ty << 16
    uint8_t *d_stripe_owner = nullptr;   // tile shards with a registered stripe map: owner per column stripe (kMaxStripes bytes)
    bool use_map = false;
    bool shard_tiles = false;
    // inputs: the live ones, and those of the frame vf_terrain_render drew last (visibility, fragment diagnostics)
    FrameInputs inputs, drawn_inputs;
    bool have_uniforms = false;
    bool have_frame = false;             // drawn_inputs is valid: set by vf_terrain_render only, cleared when the shard layout changes
    uint32_t *d_rgba_scratch = nullptr;  // output of those diagnostic re-renders: the caller's frame is never overwritten
    uint32_t *d_diag = nullptr;          // [0] covered pixels (fragment-stage diagnostics)
    // device state
    float *d_xs = nullptr, *d_sinx = nullptr, *d_cosz = nullptr;
    int32_t *d_txi = nullptr, *d_tyj = nullptr;
    float *d_height_own = nullptr;       // Scene::set_height_from_r32f's copy (its own allocation: it is replaced when the size changes)
    float *d_height_dummy = nullptr;     // the 1x1 zero texture of TerrainSpike (in the slab)
    const float *d_height = nullptr;
    uint8_t *slab = nullptr;             // ONE device allocation behind every fixed-size buffer of the handle (round 5: construction was ~40 hipMallocs)
    uint32_t tw = 1, th = 1;
    bool bounds_dirty = true;
    float2 *d_bounds = nullptr;          // per block: min/max displaced height
    float *d_hblk = nullptr;             // displaced-height cache: 81 floats per block
    float *d_lut = nullptr;              // 256*3 linear floats
    uint32_t *d_rgba_own = nullptr;
    uint32_t *d_rgba = nullptr;
    uint32_t *d_vis = nullptr;           // only allocated for vf_terrain_read_visibility and for occluding overlay layers
    uint32_t *d_stats = nullptr;         // [0] (tile, block) pairs rasterised (stats_layout)
    // geometry buffers: made by the first call that needs them, reused, grown when a call asks for more
    DevBuf<uint8_t> d_gb;                // device planes behind vf_terrain_read_gbuffer
    DevBuf<uint8_t> d_pick;              // vf_terrain_pick: n pixels in, n records out
    // cast shadows: buffers made by the first shadowed frame or field read; the field is computed again only when
    // what it was made from has changed
    struct Shadows {
        bool enabled = false;
        float strength = 0.7f, softness = 0.02f, bias = 0.002f;
        VertexField lit;                 // key: sun (3), spacing, exaggeration, strength, softness, bias
        DevBuf<float> d_cmax;            // chunk maxima / carries of the scan: nchunks x nlines
    } sh;
    // ambient occlusion: the same rules; the sun, the camera and `strength` are not part of the field
    struct Ambient {
        bool enabled = false;
        float strength = VF_AMBIENT_STRENGTH, reach = VF_AMBIENT_REACH;
        uint32_t ndirs = VF_AMBIENT_DIRECTIONS;
        bool default_dirs = true;        // dirs holds the default set of ndirs directions (made when first needed)
        std::vector<float> dirs;         // ndirs x (ux, uz)
        VertexField sky;                 // key: spacing, exaggeration, reach, the length of dirs, dirs
    } am;
    // the draped image: everything is made by set_drape and freed by clear_drape; iw = 0: none
    struct Drape {
        uint32_t iw = 0, ih = 0;
        float extent[4] = { -1.5f, -1.5f, 1.5f, 1.5f }, opacity = 1.0f;
        int filter = VF_DRAPE_LINEAR;
        DevBuf<uint32_t> d_img;          // iw x ih RGBA8 words, row-major
        hipEvent_t copied = nullptr;     // behind set_drape_device's copy on the caller's stream: the frames' shade passes wait for it
    } dr;
    // its mip pyramid: enabled and bias are the handle's and survive set_drape / clear_drape; the rest belongs to the
    // image held and exists only while a drape is held and mipmaps are on
    struct DrapeMipState {
        bool enabled = false;
        float bias = 0.0f;
        uint32_t aniso = 1;              // the largest anisotropy A: the handle's as bias is; 1: 4k's one sample
        DevBuf<uint2> d_pyr;            // levels 1 ... levels - 1, one after the other, each from an even texel index (16-byte aligned)
        bool stale = true;               // d_pyr does not hold the pyramid of the image held
        uint32_t builds = 0;             // times a pyramid was built (vf_terrain_drape_mip_info)
    } dm;
    // viewshed analysis: buffers made by the first tinted frame or field read; the field is computed again only when
    // what it was made from has changed (not for the colours, the radius or a spacing that leaves the observer's vertex where it was)
    struct Viewshed {
        bool enabled = false, have_observer = false;
        float ox = 0.0f, oz = 0.0f;      // the observer in the overlays' world frame
        float eye_height = VF_VIEWSHED_EYE_HEIGHT, target_height = VF_VIEWSHED_TARGET_HEIGHT, radius = 0.0f;
        float softness = VF_VIEWSHED_SOFTNESS, bias = VF_VIEWSHED_BIAS;
        uint32_t visible_rgba = VF_VIEWSHED_VISIBLE_RGBA, hidden_rgba = VF_VIEWSHED_HIDDEN_RGBA;   // r | g << 8 | b << 16 | a << 24
        bool tinted = false;             // enabled once since the observer was set (vf_terrain_debug_viewshed_stage asks for it)
        VertexField seen;                // key: exaggeration, eye_height, target_height, softness, bias, the observer's vertex (i, j)
        DevBuf<float> d_cmax;            // chunk maxima / carries of the scan: 4 quadrants x nchunks x nlines
    } vs;
    // cumulative viewsheds: buffers made by the first tinted frame or field read; the sums are formed again only when
    // what they were made from has changed (not for the colours, the camera or the sun)
    struct CumulativeViewshed {
        bool enabled = false;
        std::vector<float> xz;           // the observers in the overlays' world frame, (x, z) each; empty: none set
        float eye_height = VF_VIEWSHED_EYE_HEIGHT, target_height = VF_VIEWSHED_TARGET_HEIGHT, radius = 0.0f;
        float softness = VF_VIEWSHED_SOFTNESS, bias = VF_VIEWSHED_BIAS;
        // the count: total = N; key: exaggeration, eye_height, target_height, softness, bias, Rc (-1: no radius), the length of the
        // vertex list, the observers' vertices (i, j) each
        SummedField sum{ VF_CUMULATIVE_VIEWSHED_HIGH_RGBA, VF_CUMULATIVE_VIEWSHED_LOW_RGBA };
        DevBuf<float> d_cmax;            // carries of a batch: B x 4 quadrants x nchunks x nlines
        DevBuf<ViewshedPlan> d_plans;    // one per observer
        std::vector<ViewshedPlan> plans; // the host's copy of d_plans (the source of its upload)
    } cv;
    // sun exposure: buffers made by the first tinted frame or field read; the sums are formed again only when what they
    // were made from has changed (not for the colours, the camera or the handle's own sun)
    struct SunExposure {
        bool enabled = false, incidence = false;
        std::vector<float> suns;         // the sun vectors as given, (x, y, z) each; empty: none set
        std::vector<float> weights;      // one per sun
        uint32_t counted = 0;            // suns with sy > 0
        float wtot = 0.0f;               // the sum of their weights, in list order
        float softness = VF_SHADOW_SOFTNESS, bias = VF_SHADOW_BIAS;
        // the exposure: total = wtot; key: spacing, exaggeration, softness, bias, incidence, the length of the list, the suns (x, y, z)
        // each, the weights
        SummedField sum{ VF_SUN_EXPOSURE_HIGH_RGBA, VF_SUN_EXPOSURE_LOW_RGBA };
        DevBuf<float2> d_slope;          // n x n (px, pz); only with incidence
        DevBuf<float> d_cmax;            // carries of a batch: B x nchunks x (2n - 1)
        DevBuf<ExposureSun> d_suns;      // the suns that add something: x-major scans, z-major scans, degenerate ones
        std::vector<ExposureSun> recs;   // the host's copy of d_suns (the source of its upload)
    } se;
    // atmospheric haze: a setting of the handle, no cached field; the plane is made by the first opacity read
    struct Haze {
        bool enabled = false, background = false;
        float density = 0.0f, start = 0.0f, falloff = 0.0f /* 0: uniform */, base = 0.0f, max_opacity = 1.0f;
        uint32_t rgba = VF_HAZE_RGBA;    // r | g << 8 | b << 16 | a << 24
        DevBuf<float> d_plane;           // (H, W) opacities behind vf_terrain_read_haze_opacity
    } hz;
    // flood analysis: buffers made by the first tinted frame or field read; the field is computed again only when what
    // it was made from has changed (not for the colours, depth_full, the camera, the sun or the exaggeration)
    struct Flood {
        // the depth; key: the bits of level, then key_tail; the counts behind d_ctl's `changed` words: flooded, wettable (one 64-bit word)
        SeededFill fill{ VF_FLOOD_EVERYWHERE, VF_FLOOD_SHALLOW_RGBA, VF_FLOOD_DEEP_RGBA, VF_FLOOD_DEPTH_FULL };
        float level = 0.0f;
        DevBuf<uint64_t> d_wet, d_fl;    // the masks, tile-major (vf_flood.h); they and d_wd stand as long as the field does: the tint reads them
        DevBuf<float> d_wd;              // level - h, n x n
        uint32_t flooded = 0, wettable = 0;      // of the last computation
    } fd;
    // spill analysis: buffers made by the first tinted frame or field read; the field is computed again only when what
    // it was made from has changed (not for the colours or depth_full)
    struct Spill {
        // the spill; key: key_tail alone; the counts behind d_ctl's `changed` words: reached, sinks (one 64-bit word), then tile_runs
        SeededFill fill{ VF_SPILL_EDGES, VF_SPILL_SHALLOW_RGBA, VF_SPILL_DEEP_RGBA, VF_SPILL_DEPTH_FULL };
        DevBuf<float> d_sd;              // spill - h, n x n; stands as long as the field does: the tint and the sink-depth read take it
        DevBuf<uint32_t> d_hk, d_w;      // the keys of h and of the spill, tile-major (vf_spill.h)
        DevBuf<uint32_t> d_act;          // the activity words: two arrays of one word per tile
        bool no_flags = false;           // vf_terrain_debug_spill_group with VF_SPILL_GROUP_NO_FLAGS: every tile runs in every pass
        uint32_t reached = 0, sinks = 0, tile_runs = 0;   // of the last computation
    } sp;
    uint64_t height_gen = 1;             // counts height uploads
    // vf_terrain_render_batch_host: a ring of device frames the poses are drawn into while earlier ones travel to the host
    static constexpr uint32_t kBatchRing = 3;
    uint32_t *d_batch[kBatchRing] = { nullptr, nullptr, nullptr };
    hipEvent_t batch_drawn[kBatchRing] = { nullptr, nullptr, nullptr }, batch_copied[kBatchRing] = { nullptr, nullptr, nullptr };
    hipStream_t copy_stream = nullptr;
    // read-backs
    uint8_t *d_png = nullptr, *h_png = nullptr;   // PNG scanlines of the last frame: device, pinned host
    uint8_t *h_stage = nullptr;                   // kStageSlots x kStageChunk pinned bytes: device -> pageable host copies go through here
    hipEvent_t stage_ev[4] = { nullptr, nullptr, nullptr, nullptr };
    // Per-frame plan state, kPlanStates times: frame f uses set f % kPlanStates.  The plan kernels of a frame run on `side` and touch
    // nothing else, so they overlap the previous frames' tile kernels (which still read the other sets) instead of waiting for them.
    // (Round 4's experiment with three states and consecutive frames on alternating streams and output buffers, whose tile kernels
    //  then overlap, was not kept -- EXPERIMENTS.md; tools/experiments/frame_path_hooks.patch brings its switches back.)
    static constexpr uint32_t kPlanStates = 2;
    struct PlanState {
        PixelBox *ranges = nullptr;      // per block: conservative pixel rectangle (from the block's height bounds)
        VertexRec *vtx = nullptr;        // per block 81 x {X, Y, 1/w, h} (k_block_setup)
        BlockRec *recs = nullptr;        // per block: alive masks, exact pixel box
        ulonglong2 *gen = nullptr;       // per block: primitives that need the generic path (valid where the record says so)
        ulonglong2 *band = nullptr;      // per block kBandSlots x {even, odd}: the alive masks per row of tiles (k_block_setup, with the records)
        uint32_t *seg_list = nullptr;    // 16-block segments with a block that reaches this shard's pixels (+ [nsegs] = their number)
        PixelBox *row_ranges = nullptr;  // per block row
        float4 *cap_seg = nullptr;       // per block: capsule axis (screen space)
        float *cap_rad = nullptr;        // per block: capsule radius
        uint32_t *rc = nullptr;          // per (tile column, block row): [lo | hi) block-column range, 2 * nb * ntx words
        uint2 *work = nullptr;           // busy tiles of the frame: (item, weight) as k_plan lists them
        uint2 *work_sorted = nullptr;    // ... heaviest first (k_plan_sort; the second half of the same allocation): what the tile kernel pulls from
        uint32_t *work_count = nullptr;  // [0] work items, [1] split budget used, [2] queue head, [3] items handed to the complete tile kernel
        uint32_t *redo = nullptr;        // those items (indices into work)
        uint32_t *background = nullptr;  // per local tile: bit 0 = no block row reaches it; bits 8.. = log2 of the strips it is cut into
        uint32_t *flags_new = nullptr;   // the same words as k_plan writes them; k_plan_sort moves them into `background`
        uint32_t *feedback = nullptr;    // time (10 ns ticks) per tile, added by this set's tile kernel, read two frames later; [ntiles] = split quantum;
                                         // then 64 words per tile: the time of each of its pieces (strip x slice)
        hipEvent_t planned = nullptr, drawn = nullptr, boxed = nullptr, set_up = nullptr;
        hipEvent_t pev[3] = { nullptr, nullptr, nullptr };   // timing: plan start, behind the block boxes, behind the plan (on the plan's stream), of this set's LAST plan
        bool pev_valid = false;
        uint8_t *slab = nullptr;         // one allocation per plan state
        float u_used[32] = {};           // view + proj of the frame whose tile times sit in `feedback` (the plan looks them up through the camera motion)
        bool have_u_used = false;
        // the stamp: geom_gen / height_gen the boxes, ranges, segment list, records, masks, band masks and vertex records were built from (0: none --
        // never filled, or left half-written).  While both equal the live generations the plan reuses them (plan_frame).
        uint64_t geom_stamp = 0, height_stamp = 0;
        // PER-TILE CANDIDATE LISTS (k_tile_lists): built once from this state's records while they stand, off the frames'
        // chain.  list_stamp: the geom_stamp of the records they were built from (0: none); whatever rebuilds the records zeroes it.
        // `listed` is recorded behind the builder: a frame that reads the lists waits for it, and so does a rebuild of the records.
        uint4 *tl_ent = nullptr, *tl_hdr = nullptr;  // the shared entry buffer (tl_units x 16 B), one header per local tile
        uint32_t *tl_ctl = nullptr;      // the bump cursor (64 bits), tiles with a list, tiles fallen back, entries listed
        uint32_t tl_units = 0, tl_cap = 0;           // allocated / handed to the last builder (vf_terrain_debug_set_tile_list_capacity)
        uint64_t list_stamp = 0;
        hipEvent_t listed = nullptr;
    } ps[kPlanStates];
    // ... for a caller that waits for its frames the builder must not stand in front of one: the state drawn last is noted here and its
    // lists are queued behind the next read-back's copy, as the plan made ahead is (or behind the next frame's kernels).
    struct ListJob { bool pending = false; uint32_t set = 0; uint64_t geom = 0; FrameParams P; } tl_job;
    bool tl_off = false;                 // VF_NO_TILE_LISTS=1 at handle creation: never build one
    uint32_t tl_cap_debug = 0xFFFFFFFFu; // vf_terrain_debug_set_tile_list_capacity (0xFFFFFFFF: the buffer's size)
    bool tl_failed = false;              // the list buffers could not be allocated: the handle goes without
    PlanCursor cursor;
    uint32_t last_set = 0;               // the set of the frame rendered last
    uint32_t last_plan_mode = 0;         // VF_PLAN_* bits of the frame rendered last (vf_terrain_debug_plan_mode)
    hipStream_t side = nullptr;          // k_block_boxes -> k_plan -> k_plan_sort
    hipStream_t side2 = nullptr;         // k_block_setup (needs the block boxes only): beside the plan chain, both under the previous frame
    hipEvent_t entry = nullptr;          // caller's stream at render entry (orders a height-cache rebuild after the caller's work)
    // behind the last height-cache rebuild, on the stream `cached_on`: a plan chain that starts on another stream waits for it first.
    // (A handle's first frame builds the cache on the caller's stream; the second frame's chain, on the plan streams, has no event of
    //  its plan state to wait for yet and used to read the bounds and the cache while they were being written -- a wrong second frame
    //  that the fourth frame used to paint over, and that reuse would keep.)
    hipEvent_t cached = nullptr;
    hipStream_t cached_on = nullptr;
    hipStream_t last_stream = nullptr;
    bool rendered = false;
    // THE NEXT FRAME'S PLAN, QUEUED AHEAD (round 5).  A camera at rest draws the same plan again and again, and a caller that waits for
    // each frame (render_png, render_rgba: every call of the reference's API) used to pay the plan chain -- block boxes, set-up pass,
    // plan, sort: 0.2 ms at C4 -- in front of every tile kernel, because nothing is left to hide it under once the caller has waited.
    // So when a frame was drawn with the very inputs of the frame before it, the first half of the NEXT frame (plan_frame) is queued
    // right behind it: by the time the caller comes back the plan is there.  `inputs_gen` counts everything a picture depends on (uniforms,
    // heights, shard, shade mode, features), `geom_gen` below what a plan depends on; a plan made ahead is used only for the geometry
    // generation it was made for, and otherwise thrown away: the bookkeeping it advanced is rolled back and the frame is planned again (its kernels queue behind the stale ones).
    uint64_t inputs_gen = 1;
    // Two generations.  `inputs_gen` means "the same picture"; `geom_gen` means "the same geometry": it counts the changes of what
    // k_block_boxes and k_block_setup read -- view, projection, spacing (u[36]) and exaggeration (u[38]) of the uniform block, compared
    // bit for bit; the heights; the shard layout (the frame and grid sizes are the handle's for life).  The sun, exposure, height range,
    // shade mode, precision, shadows, ambient occlusion, drape and overlays move inputs_gen alone.  A counter, not a hash: camera
    // A -> B -> A is two changes.  A plan state's boxes and records (PlanState::geom_stamp) and a plan made ahead (PrePlan::geom) hold
    // for one geometry generation; a plan made ahead that meets new shading inputs has the shading fields of its K.P refreshed.
    uint64_t geom_gen = 1;
    struct PrePlan {
        bool valid = false;
        FramePlan K;
        uint64_t gen = 0, geom = 0;      // inputs_gen / geom_gen it was made for
        PlanCursor before;               // where the handle stood before plan_frame advanced it (restored when the plan is thrown away)
    } pre;
    uint64_t last_drawn_geom = 0;        // geom_gen of the frame drawn last (SAME GEOMETRY: two frames of one generation -- the camera is at rest, whatever the light does)
    bool replan_fresh = false;           // a plan queued ahead was thrown away: the next plan takes the previous frame's tile times (drop_preplan)
    // Round 6: a caller that WAITS for every frame (every call of the reference's API) never makes the context's two plan streams (17-20 ms
    // once per process, which its second call used to pay): its plans run on its own stream, and the plan made ahead for a camera at
    // rest is queued BEHIND THE NEXT READ-BACK'S COPY (flush_preplan) -- it runs while the host unpacks / deflates / returns, not in
    // front of the copy the caller waits for.  The plan streams are made when a frame arrives while the previous one is still in
    // flight: a caller that streams frames, which is what they are for.
    bool preplan_pending = false;
    // ... unless that caller comes back faster than the plan runs: a tight loop of synchronous frames with nothing between them finds
    // the plan made ahead still running behind the copy (C4 render_rgba 2.0 -> 2.2 ms, C2 0.10 -> 0.14), where the plan streams would
    // have run it UNDER the frame.  Three such calls in a row and the handle takes the plan streams after all (17-20 ms, once).
    uint32_t tight_calls = 0;
    bool want_plan_streams = false;
    hipEvent_t copied = nullptr;         // behind a read-back's copy: the host waits for this, not for the stream (the plan made ahead follows it)
    // timing: a ring of events on the draw stream, one pair per timed frame (the plan's events live with its plan state: pev)
    static constexpr int kTimingRing = 64;
    bool timing = false;
    bool stats_on = false;               // per-item statistics as well (vf_terrain_enable_timing(t, 1)); 2 = device times only
    uint32_t timing_every = 1;           // 3 = device times of every 4th frame only: two event records on the draw stream cost a frame 2 % (tools/exp_timing_cost.py)
    struct FrameEvents { hipEvent_t begin = nullptr, end = nullptr; } ev[kTimingRing];   // before the clear, after the tile kernels (caller's stream)
    uint32_t timed_frames = 0;           // frames recorded since timing was enabled
    LineLoop loop;
    // vf_dist_exchange_bands: the chunks this rank receives in the all-to-all ([nranks][chunk_tiles] tile slots) and the band it stitches from them
    uint8_t *d_xrecv = nullptr, *d_xband = nullptr;
    size_t xrecv_bytes = 0, xband_bytes = 0;
    // Overlays (vf_terrain_add_points / _add_lines, vf_overlay.h): made by the first add, freed by vf_terrain_clear_overlays -- a handle
    // without overlays holds none of it and launches nothing for them.
    struct Overlays {
        uint32_t nprims = 0, features = 0;
        DevBuf<OvIn> in;                     // [nprims] primitives as added, in feature order
        DevBuf<OvPrim> prim;                 // [nprims] ... as the frame sees them (k_ov_setup)
        DevBuf<uint2> box;                   // [nprims] bin rectangle
        uint32_t *d_cnt = nullptr;           // [nbins] pairs per bin (zero between frames)
        uint32_t *d_start = nullptr;         // [nbins + 1] each bin's slice of the pair list; [nbins] = pairs in all
        DevBuf<uint32_t> list;               // pair list (primitive indices)
        uint32_t *h_total = nullptr;         // pinned: the frame's pair count (the list is sized by it); [2..3] the mask words (fills)
        hipEvent_t counted = nullptr;
        // polygon fills (vf_terrain_add_polygons): made by the first polygon layer
        uint32_t nfill = 0;                  // fill features (each: one header record and two slots per ring edge)
        uint32_t pg_lo = 0, pg_hi = 0;       // record index range that holds every fill record
        DevBuf<uint32_t> pg_hdr;             // [nfill] each fill feature's header record index
        DevBuf<uint4> pg_fbox;               // [nfill] folded feature box (zero between frames)
        DevBuf<uint4> pg_fbin;               // [nfill] the frame's mask base and bin box of each fill feature
        DevBuf<unsigned long long> pg_total; // [1] the frame's mask words (zero between frames)
        DevBuf<uint32_t> mask;               // (feature, bin) backdrop masks, bit r: parity of row r's crossings right of the bin
        // occlusion (vf_terrain_set_layer_occlusion)
        struct Layer { uint32_t lo, hi; bool polygon, occlude; bool haze = false; };
        std::vector<Layer> layer;            // each layer's record range; a layer's id is its index
        uint32_t occluding = 0;              // layers with occlusion on: the frame stores its visibility and composites with depth
        DevBuf<float4> dep;                  // [nprims] per primitive (rw_a, rw_b - rw_a, kb, 0) of occluding primitives (k_ov_setup)
        // hazed layers (vf_terrain_set_layer_haze)
        uint32_t hazed = 0;                  // layers that take the haze: a frame with haze enabled composites them under it
        DevBuf<float4> hzrec;                // [nprims] per primitive (rw_a, rw_b - rw_a, yq_a or y_c, yq_b - yq_a or ah) (k_ov_haze_setup); made by the first hazed layer
    } ov;
    // Contour extraction (vf_terrain_add_contours / vf_terrain_height_bounds, vf_contour.h): made by the first such call, freed with the
    // overlays -- a handle that never asks for contours holds none of it and launches nothing for them.
    struct Contours {
        DevBuf<float> levels;                // the call's level list
        DevBuf<uint32_t> count;              // [nblocks] segments per block, then their exclusive offsets
        DevBuf<unsigned long long> total;    // [1] segments in all
        DevBuf<float2> bounds;               // [1] vf_terrain_height_bounds
    } ct;
};

// Sizes that more than one place must agree on, in 32-bit words.
// d_stats: four counters, four words per possible work item, the phase cycle counts (64-bit), one bit per block (drawn this frame?)
struct StatsLayout { size_t phases, block_bits, words; };
static StatsLayout stats_layout(const vf_terrain *t)
{
    const size_t phases = 4 + 4 * ((size_t)t->ntx * t->nty + kSplitBudget), block_bits = phases + 2 * kPhaseSlots;
    return { phases, block_bits, block_bits + (t->nblocks + 31) / 32 };
}
// a plan state's tile times: one word per tile, the split quantum, 64 words per tile for its pieces
static size_t feedback_words(const vf_terrain *t) { return (size_t)t->ntx * t->nty * 65 + 1; }
// 16-block segments of the grid's block rows
static uint32_t grid_segments(const vf_terrain *t) { return t->nb * ((t->nb + kSegBlocks - 1) / kSegBlocks); }
// the pitch of the grid's vertices (FrameParams::step) and the spacing of a uniform block (terrain.wgsl:46)
static float grid_step(const vf_terrain *t) { return (2.0f * 1.5f) / ((float)t->n - 1.0f); }
static float spacing_of(const float *u) { return std::fmax(u[36], 1e-8f); }

int VertexField::prepare(const vf_terrain *t, const std::vector<uint32_t> &k, bool force, const char *nomem, bool *current)
{
    if (!d.p) {
        const size_t nv = (size_t)t->n * t->n;
        if (d.reserve(nv, nv) != hipSuccess) { (void)hipGetLastError(); return fail(VF_ERR_NOMEM, nomem); }
        valid = false;
    }
    *current = !force && valid && height_gen == t->height_gen && key == k;
    if (!*current) valid = false;
    return VF_OK;
}

void VertexField::computed(const vf_terrain *t, std::vector<uint32_t> &k)
{
    key.swap(k);
    height_gen = t->height_gen; valid = true; scans++;
}

extern "C" {

const char *vf_last_error(void) { return g_err.c_str(); }

int vf_device_count(int *count)
{
    if (!count) return fail(VF_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(VF_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
    *count = n;
    return VF_OK;
}

static void fill_info(int ordinal, const hipDeviceProp_t &p, vf_device_info *out)
{
    std::memset(out, 0, sizeof *out);
    std::snprintf(out->name, sizeof out->name, "%s", p.name);
    std::snprintf(out->arch, sizeof out->arch, "%s", p.gcnArchName);
    out->device_ordinal = ordinal;
    out->compute_units = p.multiProcessorCount;
    out->wavefront_size = p.warpSize;
    out->clock_khz = p.clockRate;
    out->total_mem_bytes = p.totalGlobalMem;
    out->lds_bytes_per_cu = p.maxSharedMemoryPerMultiProcessor;
    out->pci_bus_id = p.pciBusID;
    out->pci_device_id = p.pciDeviceID;
}

int vf_device_query(int device_ordinal, vf_device_info *out)
{
    if (!out) return fail(VF_ERR_INVALID, "out is NULL");
    int n = 0;
    int rc = vf_device_count(&n);
    if (rc != VF_OK) return rc;
    if (device_ordinal < 0 || device_ordinal >= n) return fail(VF_ERR_NO_DEVICE, "No suitable GPU adapter");
    hipDeviceProp_t p;
    VF_HIP_TRY(hipGetDeviceProperties(&p, device_ordinal));
    fill_info(device_ordinal, p, out);
    return VF_OK;
}

int vf_ctx_create(int device_ordinal, vf_ctx **out)
{
    if (!out) return fail(VF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0 || device_ordinal < 0 || device_ordinal >= n)
        return fail(VF_ERR_NO_DEVICE, "No suitable GPU adapter");   // reference string, src/terrain/mod.rs:285
    vf_ctx *c = new (std::nothrow) vf_ctx;
    if (!c) return fail(VF_ERR_NOMEM, "out of host memory");
    c->device = device_ordinal;
    hipError_t err = hipSetDevice(device_ordinal);
    if (err == hipSuccess) err = hipGetDeviceProperties(&c->prop, device_ordinal);
    if (err == hipSuccess) err = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    static_assert(offsetof(SrgbTables, decode) == 0 && offsetof(SrgbTables, thresh) == 256 * sizeof(float) && sizeof(SrgbTables) == 512 * sizeof(float),
                  "both tables go up in one copy");
    if (err == hipSuccess) err = hipMalloc(&c->d_decode, sizeof(SrgbTables));
    if (err == hipSuccess) err = hipMemcpy(c->d_decode, &tables(), sizeof(SrgbTables), hipMemcpyHostToDevice);
    if (err == hipSuccess) c->d_thresh = c->d_decode + 256;
    if (err != hipSuccess) {
        std::string m = std::string("context creation failed: ") + hipGetErrorString(err);
        vf_ctx_destroy(c);
        return fail(VF_ERR_HIP, m);
    }
    *out = c;
    return VF_OK;
}

void vf_ctx_destroy(vf_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->d_decode) (void)hipFree(c->d_decode);
    if (c->d_maps) (void)hipFree(c->d_maps);
    for (hipStream_t q : { c->side, c->side2, c->copy }) if (q) (void)hipStreamDestroy(q);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int vf_ctx_device_info(const vf_ctx *ctx, vf_device_info *out)
{
    if (!ctx || !out) return fail(VF_ERR_INVALID, "NULL argument");
    fill_info(ctx->device, ctx->prop, out);
    return VF_OK;
}

int vf_ctx_stream(const vf_ctx *ctx, void **stream)
{
    if (!ctx || !stream) return fail(VF_ERR_INVALID, "NULL argument");
    *stream = (void *)ctx->stream;
    return VF_OK;
}

// ------------------------------------------------------------------------------------------------

static uint32_t compute_local_rows(uint32_t H, uint32_t rank, uint32_t nranks, uint32_t band_h)
{
    if (nranks <= 1) return H;
    uint32_t rows = 0;
    for (uint32_t b = 0; b * band_h < H; ++b)
        if (b % nranks == rank) rows += (b + 1) * band_h <= H ? band_h : H - b * band_h;
    return rows;
}

static AxisTables axis(const vf_terrain *t)
{
    AxisTables A;
    A.xs = t->d_xs; A.sinx = t->d_sinx; A.cosz = t->d_cosz; A.txi = t->d_txi; A.tyj = t->d_tyj;
    return A;
}

// Buffers carved out of one device allocation, 256-byte aligned; those that must start at zero lie first and share one memset.
namespace {
struct Carver {
    struct Item { void **p; size_t bytes; };
    std::vector<Item> zeroed, plain;
    void add(void **p, size_t bytes, bool zero = false) { (zero ? zeroed : plain).push_back({ p, (bytes + 255u) & ~(size_t)255u }); }
    hipError_t commit(uint8_t **base, hipStream_t s)
    {
        size_t zero_bytes = 0, total = 0;
        for (const Item &i : zeroed) zero_bytes += i.bytes;
        total = zero_bytes;
        for (const Item &i : plain) total += i.bytes;
        hipError_t e = hipMalloc((void **)base, total);
        if (e != hipSuccess) return e;
        size_t off = 0;
        for (const Item &i : zeroed) { *i.p = *base + off; off += i.bytes; }
        for (const Item &i : plain) { *i.p = *base + off; off += i.bytes; }
        return zero_bytes ? hipMemsetAsync(*base, 0, zero_bytes, s) : hipSuccess;
    }
};
} // namespace

static hipError_t sync_sides(const vf_terrain *t)            // (the side streams exist from the handle's second frame on)
{
    hipError_t e = t->side ? hipStreamSynchronize(t->side) : hipSuccess;
    if (e == hipSuccess && t->side2) e = hipStreamSynchronize(t->side2);
    return e;
}

// the frame in flight (on the caller's stream, else the handle's own) has finished: what it reads may change now
static hipError_t wait_frame(const vf_terrain *t)
{
    const hipError_t e = hipSetDevice(t->ctx->device);
    return e != hipSuccess ? e : hipStreamSynchronize(t->last_stream ? t->last_stream : t->ctx->stream);
}

// A plan queued ahead of its frame (vf_terrain::pre) is thrown away: back to where the handle stood before it, and that set's segment list
// starts empty again (the stale k_block_boxes filled it; its k_clear, which would have emptied it, never runs).
static hipError_t drop_preplan(vf_terrain *t, hipStream_t next_plan_on = nullptr)
{
    t->preplan_pending = false;
    if (!t->pre.valid) return hipSuccess;
    const vf_terrain::PrePlan &R = t->pre;
    t->pre.valid = false;
    t->cursor = R.before;
    // The stale plan's k_plan_sort has already zeroed this set's tile times and replaced its flag words: the frame that is planned in
    // its place reads the PREVIOUS frame's (complete: the caller was idle when the plan went out) -- plan_frame's `fresh` mode.
    t->replan_fresh = true;
    // The stale chain ran on `side`, the stale set-up pass on `side2` (a waiting caller's: both on the stream of its last read-back):
    // the frame planned next rewrites this set's block boxes, records and segment list, and must not do so while the stale set-up pass
    // still reads and writes them -- the stream its plan starts on waits for both.
    hipStream_t on = t->side ? t->side : (next_plan_on ? next_plan_on : (t->last_stream ? t->last_stream : t->ctx->stream));
    hipError_t e = hipStreamWaitEvent(on, t->ps[R.K.set].set_up, 0);
    if (e == hipSuccess) e = hipStreamWaitEvent(on, t->ps[R.K.set].planned, 0);
    if (e == hipSuccess) e = hipMemsetAsync(R.K.seg_count, 0, sizeof(uint32_t), on);
    return e;
}

// A plan state's buffers and events, made when the state is first used (frame 0: at construction; frame 1: by that frame).
static hipError_t ensure_plan_state(vf_terrain *t, uint32_t k, hipStream_t zero_on)
{
    vf_terrain::PlanState &S = t->ps[k];
    if (S.slab) return hipSuccess;
    const size_t all_tiles = (size_t)t->ntx * t->nty;
    Carver C;
    C.add((void **)&S.seg_list, ((size_t)grid_segments(t) + 1) * sizeof(uint32_t), true);
    C.add((void **)&S.feedback, feedback_words(t) * sizeof(uint32_t), true);
    C.add((void **)&S.background, all_tiles * sizeof(uint32_t), true);
    C.add((void **)&S.ranges, t->nblocks * sizeof(PixelBox));
    C.add((void **)&S.vtx, (size_t)t->nblocks * kBlockStride * sizeof(VertexRec));
    C.add((void **)&S.recs, (size_t)t->nblocks * sizeof(BlockRec));
    C.add((void **)&S.band, (size_t)t->nblocks * kBandSlots * sizeof(ulonglong2));
    C.add((void **)&S.gen, (size_t)t->nblocks * sizeof(ulonglong2));
    C.add((void **)&S.row_ranges, t->nb * sizeof(PixelBox));
    C.add((void **)&S.cap_seg, t->nblocks * sizeof(float4));
    C.add((void **)&S.cap_rad, t->nblocks * sizeof(float));
    C.add((void **)&S.rc, 2 * (size_t)t->nb * t->ntx * sizeof(uint32_t));
    C.add((void **)&S.work, 2 * (all_tiles + kSplitBudget + 16) * sizeof(uint2));   // tiles + strips created by splitting: as planned, and (second half) ordered
    C.add((void **)&S.work_count, 4 * sizeof(uint32_t));
    C.add((void **)&S.redo, (all_tiles + kSplitBudget) * sizeof(uint32_t));
    C.add((void **)&S.flags_new, all_tiles * sizeof(uint32_t));
    hipError_t err = C.commit(&S.slab, zero_on);          // (the stream of the state's first user: the plan chain)
    if (err != hipSuccess) { S.slab = nullptr; return err; }
    S.geom_stamp = S.height_stamp = 0;                     // a fresh slab holds no geometry
    S.list_stamp = 0;
    S.work_sorted = S.work + (all_tiles + kSplitBudget + 16);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&S.planned, hipEventDisableTiming);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&S.drawn, hipEventDisableTiming);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&S.boxed, hipEventDisableTiming);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&S.set_up, hipEventDisableTiming);
    return err;
}

static int refresh_tables(vf_terrain *t, hipStream_t s)
{
    hipLaunchKernelGGL(k_axis_tables, dim3((t->n + 255) / 256), dim3(256), 0, s, t->n, t->tw, t->th, t->d_xs, t->d_sinx,
                       t->d_cosz, t->d_txi, t->d_tyj);
    VF_HIP_TRY(hipGetLastError());
    t->bounds_dirty = true;
    return VF_OK;
}

// the overlay state: gone, as if the handle never had overlays (the caller has synchronised)
static void ov_release(vf_terrain *t)
{
    vf_terrain::Overlays &O = t->ov;
    void *ptrs[] = { O.d_cnt, O.d_start };
    for (void *p : ptrs) if (p) (void)hipFree(p);
    O.in.release(); O.prim.release(); O.box.release(); O.list.release(); O.dep.release(); O.hzrec.release();
    O.pg_hdr.release(); O.pg_fbox.release(); O.pg_fbin.release(); O.pg_total.release(); O.mask.release();
    if (O.h_total) (void)hipHostFree(O.h_total);
    if (O.counted) (void)hipEventDestroy(O.counted);
    O = vf_terrain::Overlays();
    t->ct.levels.release(); t->ct.count.release(); t->ct.total.release(); t->ct.bounds.release();
}

// the draped image: gone, as if the handle never had one (the caller has synchronised)
static void drape_release(vf_terrain *t)
{
    vf_terrain::Drape &D = t->dr;
    D.d_img.release();
    if (D.copied) (void)hipEventDestroy(D.copied);
    D = vf_terrain::Drape();
    t->dm.d_pyr.release(); t->dm.stale = true;              // (the pyramid goes with its image; the setting stays)
}

// the shadow and sky-view fields with the scan's carries (their settings stay)
static void shadow_release(vf_terrain *t) { t->sh.lit.release(); t->sh.d_cmax.release(); }
static void ambient_release(vf_terrain *t) { t->am.sky.release(); }

// the viewshed: gone, as if the handle never had an observer (the caller has synchronised); the scan counter stays
static void viewshed_release(vf_terrain *t)
{
    vf_terrain::Viewshed &H = t->vs;
    H.seen.release(); H.d_cmax.release();
    const uint32_t scans = H.seen.scans;
    H = vf_terrain::Viewshed();
    H.seen.scans = scans;
}

// the cumulative viewshed and sun exposure: gone as summed_reset says
static void cumulative_release(vf_terrain *t)
{
    t->cv.d_cmax.release(); t->cv.d_plans.release();
    summed_reset(t->cv);
}
static void exposure_release(vf_terrain *t)
{
    t->se.d_slope.release(); t->se.d_cmax.release(); t->se.d_suns.release();
    summed_reset(t->se);
}

// the flood and the spill: gone as fill_reset says; the spill's other group setting stays too
static void flood_release(vf_terrain *t)
{
    t->fd.d_wet.release(); t->fd.d_fl.release(); t->fd.d_wd.release();
    fill_reset(t->fd);
}
static void spill_release(vf_terrain *t)
{
    t->sp.d_sd.release(); t->sp.d_hk.release(); t->sp.d_w.release(); t->sp.d_act.release();
    const bool no_flags = t->sp.no_flags;
    fill_reset(t->sp);
    t->sp.no_flags = no_flags;
}

int vf_terrain_create(vf_ctx *ctx, uint32_t width, uint32_t height, uint32_t grid, const uint8_t lut_rgba8[1024],
                      int lut_is_srgb, vf_terrain **out)
{
    return vf_terrain_create_supersampled(ctx, width, height, grid, lut_rgba8, lut_is_srgb, 1u, out);
}

// (width, height: the frame handed out; the handle's W, H are the raster's, `factor` times as large)
int vf_terrain_create_supersampled(vf_ctx *ctx, uint32_t out_width, uint32_t out_height, uint32_t grid, const uint8_t lut_rgba8[1024],
                                   int lut_is_srgb, uint32_t factor, vf_terrain **out)
{
    if (!ctx || !out || !lut_rgba8) return fail(VF_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (out_width == 0 || out_height == 0 || out_width > 16384 || out_height > 16384) return fail(VF_ERR_INVALID, "width/height must be in 1..16384");
    if (factor < 1u || factor > (uint32_t)VF_SUPERSAMPLE_MAX)
        return fail(VF_ERR_INVALID, "supersampling factor " + std::to_string(factor) + " is outside 1.." + std::to_string(VF_SUPERSAMPLE_MAX));
    if (factor * out_width > 16384u || factor * out_height > 16384u)
        return fail(VF_ERR_INVALID, "supersampling: " + std::to_string(factor) + " x (" + std::to_string(out_width) + " x " + std::to_string(out_height) +
                                    ") samples exceed the 16384 x 16384 frame limit");
    const uint32_t width = factor * out_width, height = factor * out_height;
    uint32_t n = grid < 2 ? 2 : grid;   // `.max(2)`, src/terrain/mod.rs:260
    if (n > 8192) return fail(VF_ERR_INVALID, "grid must be <= 8192");
    VF_HIP_TRY(hipSetDevice(ctx->device));
    vf_terrain *t = new (std::nothrow) vf_terrain;
    if (t) { const char *e = std::getenv("VF_NO_TILE_LISTS"); t->tl_off = e && *e && std::strcmp(e, "0") != 0; }
    if (!t) return fail(VF_ERR_NOMEM, "out of host memory");
    t->ctx = ctx; t->W = width; t->H = height; t->n = n;
    t->ss = factor; t->oW = out_width; t->oH = out_height;
    t->nb = (n - 1 + kBlockCells - 1) / kBlockCells;
    t->nblocks = t->nb * t->nb;
    t->ntx = (width + kTileW - 1) / kTileW;
    t->nty = (height + kTileH - 1) / kTileH;
    t->local_rows = height;
    t->local_tiles = t->ntx * t->nty;

    // linear LUT as the kernels stage it: 257 x {r, g, b, 0}, entry 256 = entry 255
    float lut[kLutFloats];
    for (int i = 0; i <= 256; ++i) {
        const int k = i < 256 ? i : 255;
        for (int ch = 0; ch < 3; ++ch)
            lut[kLutStride * i + ch] = lut_is_srgb ? tables().decode[lut_rgba8[4 * k + ch]] : (float)lut_rgba8[4 * k + ch] / 255.0f;
        lut[kLutStride * i + 3] = 0.0f;
    }
    // ONE device allocation for the handle's fixed-size buffers (the buffers that must start at zero lie first: one memset), one more per
    // plan state when that state is first used (ensure_plan_state) -- construction was ~40 hipMallocs and 4 memsets (round 4: unmeasured).
    hipError_t err = hipSuccess;
    const size_t all_tiles = (size_t)t->ntx * t->nty;
    Carver C;
    C.add((void **)&t->d_height_dummy, sizeof(float), true);      // 1x1 zero texture, src/terrain/mod.rs:342-378
    C.add((void **)&t->d_stats, stats_layout(t).words * sizeof(uint32_t), true);   // (only [0..4) must be zero)
    C.add((void **)&t->d_xs, n * sizeof(float));
    C.add((void **)&t->d_sinx, n * sizeof(float));
    C.add((void **)&t->d_cosz, n * sizeof(float));
    C.add((void **)&t->d_txi, n * sizeof(int32_t));
    C.add((void **)&t->d_tyj, n * sizeof(int32_t));
    C.add((void **)&t->d_bounds, t->nblocks * sizeof(float2));
    C.add((void **)&t->d_hblk, (size_t)t->nblocks * kBlockStride * sizeof(float));
    C.add((void **)&t->d_lut, sizeof lut);
    if (factor == 1u) C.add((void **)&t->d_rgba_own, all_tiles * kTileW * kTileH * sizeof(uint32_t));   // whole tiles: tile-major shards need the padding
    else {                                                        // (the samples take the frame's place under the terrain passes)
        C.add((void **)&t->d_samples, all_tiles * kTileW * kTileH * sizeof(uint32_t));
        C.add((void **)&t->d_rgba_own, (size_t)out_width * out_height * sizeof(uint32_t));
    }
    C.add((void **)&t->d_tile_map, all_tiles * sizeof(uint32_t));
    C.add((void **)&t->d_stripe_owner, kMaxStripes);
    err = C.commit(&t->slab, ctx->stream);
    // (the two side streams are made by the handle's SECOND frame: a stream costs ~2 ms to create and as much to destroy, and a
    //  handle's first frame -- the only one of the reference's construct / render_png once usage -- has nothing to overlap with)
    if (err == hipSuccess) err = hipMemcpyAsync(t->d_lut, lut, sizeof lut, hipMemcpyHostToDevice, ctx->stream);   // (pageable source: returns when the copy is staged)
    if (err == hipSuccess) err = hipEventCreateWithFlags(&t->entry, hipEventDisableTiming);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&t->cached, hipEventDisableTiming);
    // (both plan states now: a device allocation costs 0.03 ms whatever its size -- measured, round 5 -- while making the second one
    //  inside the handle's second frame cost that frame 0.7 ms)
    for (uint32_t k = 0; k < vf_terrain::kPlanStates && err == hipSuccess; ++k) err = ensure_plan_state(t, k, ctx->stream);
    if (err != hipSuccess) {
        std::string m = std::string("terrain allocation failed: ") + hipGetErrorString(err);
        vf_terrain_destroy(t);
        return fail(err == hipErrorOutOfMemory ? VF_ERR_NOMEM : VF_ERR_HIP, m);
    }
    t->d_rgba = t->d_rgba_own;
    t->d_height = t->d_height_dummy; t->tw = 1; t->th = 1;
    int rc = refresh_tables(t, ctx->stream);
    if (rc == VF_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(VF_ERR_HIP, "table setup failed");
    if (rc != VF_OK) { std::string keep = g_err; vf_terrain_destroy(t); g_err = keep; return rc; }
    *out = t;
    return VF_OK;
}

void vf_terrain_destroy(vf_terrain *t)
{
    if (!t) return;
    (void)hipSetDevice(t->ctx->device);
    (void)hipDeviceSynchronize();
    void *ptrs[] = { t->slab, t->d_height_own, t->d_vis, t->d_rgba_scratch, t->d_diag, t->d_xrecv, t->d_xband, t->d_batch[0], t->d_batch[1], t->d_batch[2] };
    for (void *p : ptrs) if (p) (void)hipFree(p);
    t->d_gb.release(); t->d_pick.release(); t->hz.d_plane.release();
    shadow_release(t); ambient_release(t); viewshed_release(t); cumulative_release(t); exposure_release(t); flood_release(t); spill_release(t);
    drape_release(t);
    for (auto &e : t->batch_drawn) if (e) (void)hipEventDestroy(e);
    for (auto &e : t->batch_copied) if (e) (void)hipEventDestroy(e);

    for (auto &S : t->ps) {
        if (S.slab) (void)hipFree(S.slab);
        if (S.planned) (void)hipEventDestroy(S.planned);
        if (S.drawn) (void)hipEventDestroy(S.drawn);
        if (S.boxed) (void)hipEventDestroy(S.boxed);
        if (S.set_up) (void)hipEventDestroy(S.set_up);
        if (S.listed) (void)hipEventDestroy(S.listed);
        if (S.tl_ent) (void)hipFree(S.tl_ent);
        if (S.tl_hdr) (void)hipFree(S.tl_hdr);
        for (auto &e : S.pev) if (e) (void)hipEventDestroy(e);
    }
    // (side / side2 / copy_stream belong to the context)
    pinned_free(t->h_stage);
    for (auto &e : t->stage_ev) if (e) (void)hipEventDestroy(e);
    if (t->d_png) (void)hipFree(t->d_png);
    pinned_free(t->h_png);
    for (auto &f : t->ev) { if (f.begin) (void)hipEventDestroy(f.begin); if (f.end) (void)hipEventDestroy(f.end); }
    if (t->entry) (void)hipEventDestroy(t->entry);
    if (t->cached) (void)hipEventDestroy(t->cached);
    if (t->copied) (void)hipEventDestroy(t->copied);
    for (auto &g : t->loop.probes) { if (g.a) (void)hipEventDestroy(g.a); if (g.b) (void)hipEventDestroy(g.b); }
    ov_release(t);
    delete t;
}

// The geometry fields of a uniform block: what k_block_boxes, k_block_setup, vertex_shader and grid_coord read of the FrameParams that
// build_params makes from it -- view (u[0..16)), proj (u[16..32)), spacing (u[36]) and exag (u[38]); hw, hh, step, n, nm1, nb, W, H and
// ntx come from the handle's sizes, the shard fields from the layout.  The sun u[32..35), exposure u[35] and the height range u[37]
// (Lx..Lz, exposure, h_range / inv2hr) are shading.  Bits are compared, not values: -0 is not +0 and a NaN equals itself.
static bool same_geometry(const float *a, const float *b)
{
    return std::memcmp(a, b, 32 * sizeof(float)) == 0 && std::memcmp(a + 36, b + 36, sizeof(float)) == 0 && std::memcmp(a + 38, b + 38, sizeof(float)) == 0;
}

// a new uniform block becomes the live one (vf_terrain_set_uniforms and the batch entry point): which generations move
static void take_uniforms(vf_terrain *t, const float *uniforms)
{
    if (!t->have_uniforms || std::memcmp(t->inputs.u, uniforms, sizeof t->inputs.u) != 0) t->inputs_gen++;     // another picture
    if (!t->have_uniforms || !same_geometry(t->inputs.u, uniforms)) t->geom_gen++;                             // ... of other geometry
    std::memcpy(t->inputs.u, uniforms, sizeof t->inputs.u);
    t->have_uniforms = true;
}

int vf_terrain_set_uniforms(vf_terrain *t, const float uniforms[44])
{
    if (!t || !uniforms) return fail(VF_ERR_INVALID, "NULL argument");
    take_uniforms(t, uniforms);
    return VF_OK;
}

static int set_height_common(vf_terrain *t, uint32_t tw, uint32_t th)
{
    t->inputs_gen++;
    t->geom_gen++;                                         // (the height cache and the block bounds are geometry inputs; so are tw / th through the axis tables)
    t->height_gen++;
    VF_HIP_TRY(drop_preplan(t));
    t->loop.reset();                                       // other heights: which line loop is faster is measured again
    bool resized = tw != t->tw || th != t->th;
    t->tw = tw; t->th = th;
    if (resized) return refresh_tables(t, t->ctx->stream);
    t->bounds_dirty = true;
    return VF_OK;
}

int vf_terrain_set_height(vf_terrain *t, const float *host_height, uint32_t tw, uint32_t th)
{
    if (!t || !host_height) return fail(VF_ERR_INVALID, "NULL argument");
    if (tw == 0 || th == 0 || tw > 32768 || th > 32768) return fail(VF_ERR_INVALID, "height texture size must be in 1..32768");
    VF_HIP_TRY(wait_frame(t));
    VF_HIP_TRY(sync_sides(t));
    size_t bytes = (size_t)tw * th * sizeof(float);
    if ((size_t)t->tw * t->th != (size_t)tw * th || t->d_height != t->d_height_own) {
        float *fresh = nullptr;                            // allocate first: a failure leaves the handle as it was
        hipError_t e = hipMalloc(&fresh, bytes);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? VF_ERR_NOMEM : VF_ERR_HIP, std::string("height texture allocation failed: ") + hipGetErrorString(e));
        if (t->d_height_own) (void)hipFree(t->d_height_own);
        t->d_height_own = fresh;
    }
    t->d_height = t->d_height_own;
    VF_HIP_TRY(hipMemcpyAsync(t->d_height_own, host_height, bytes, hipMemcpyHostToDevice, t->ctx->stream));
    int rc = set_height_common(t, tw, th);
    if (rc == VF_OK) {
        // the per-block height cache and bounds depend on the texture alone: built here, behind the upload, not by the first frame
        // (a texture handed over in device memory may still be written by the caller's stream: that one is cached by the next frame)
        hipLaunchKernelGGL(k_height_blocks, dim3(t->nblocks), dim3(64), 0, t->ctx->stream, t->n, t->nb, t->tw, axis(t), t->d_height, t->d_hblk, t->d_bounds);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) rc = fail(VF_ERR_HIP, std::string("k_height_blocks: ") + hipGetErrorString(le));   // (bounds stay dirty)
        else t->bounds_dirty = false;
    }
    VF_HIP_TRY(hipStreamSynchronize(t->ctx->stream));   // host buffer is only borrowed for this call
    return rc;
}

int vf_terrain_set_height_device(vf_terrain *t, const float *dev_height, uint32_t tw, uint32_t th)
{
    if (!t || !dev_height) return fail(VF_ERR_INVALID, "NULL argument");
    if (tw == 0 || th == 0 || tw > 32768 || th > 32768) return fail(VF_ERR_INVALID, "height texture size must be in 1..32768");
    // a frame still in flight (caller's stream, or the plan / height-cache kernels on the side stream) reads the axis tables
    // and the old texture: let it finish before either changes
    VF_HIP_TRY(wait_frame(t));
    VF_HIP_TRY(sync_sides(t));
    t->d_height = dev_height;
    int rc = set_height_common(t, tw, th);
    if (rc != VF_OK) return rc;
    VF_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
    return VF_OK;
}

int vf_terrain_set_shade_mode(vf_terrain *t, int mode)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (mode != VF_SHADE_REFERENCE && mode != VF_SHADE_SPEC_T32) return fail(VF_ERR_INVALID, "unknown shade mode");
    if (t->inputs.shade_mode != (uint32_t)mode) t->inputs_gen++;
    t->inputs.shade_mode = (uint32_t)mode;
    return VF_OK;
}

int vf_terrain_set_shade_precision(vf_terrain *t, int precision)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (precision != VF_PRECISION_EXACT && precision != VF_PRECISION_FAST) return fail(VF_ERR_INVALID, "unknown shade precision");
    if (t->inputs.precision != (uint32_t)precision) t->inputs_gen++;
    t->inputs.precision = (uint32_t)precision;
    return VF_OK;
}

int vf_terrain_set_raster_groups(vf_terrain *t, int mode)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (mode < -1 || mode > 1) return fail(VF_ERR_INVALID, "mode must be -1 (measure and choose), 0 or 1");
    t->loop.mode = mode;
    t->loop.reset();
    return VF_OK;
}

int vf_terrain_raster_groups(const vf_terrain *t, int *in_use, float ms[2])
{
    if (!t || !in_use) return fail(VF_ERR_INVALID, "NULL argument");
    *in_use = t->loop.now;
    if (ms) { ms[0] = t->loop.n[0] ? t->loop.ms[0] : 0.0f; ms[1] = t->loop.n[1] ? t->loop.ms[1] : 0.0f; }
    return VF_OK;
}

// ---- the passes behind the tile kernel -----------------------------------------------------------------------
// Every pass that rewrites the terrain's pixels from the stored visibility (vf_visible.h), in the order a frame draws them behind its
// tile kernels: light on the surface, what lies on it (the image, the water, the sinks), the analysis tints with the single observer's
// on top, the air in front of it all.  Each needs the whole frame on one handle and the frame's own inputs, so a handle that has one
// on is not sharded and draws no batches.  A new pass is a row here and a place in kRefusalOrder.
using FramePassRun = int(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba);
static int relight_pass(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba, Relight pass,
                        bool shadows, bool ambient);
static FramePassRun viewshed_pass, cumulative_pass, exposure_pass, haze_pass, flood_pass, spill_pass;

// The drape's shade pass as the handle's settings choose it: through the mip pyramid when mipmaps are on, and with
// anisotropic taps when the largest anisotropy is above 1 as well (4p); the frames and the drape diagnostics both ask here
static Relight drape_pass_of(const vf_terrain *t) { return !t->dm.enabled ? kDrape : t->dm.aniso > 1u ? kDrapeAniso : kDrapeMip; }

// cast shadows and ambient occlusion are one pass of the relight kernel, whichever of them is on
static int light_pass(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba)
{
    return relight_pass(t, s, P, V, redo, rgba, t->am.enabled ? kAmbient : kShadow, t->sh.enabled, t->am.enabled);
}
static int drape_pass(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba)
{
    return relight_pass(t, s, P, V, redo, rgba, drape_pass_of(t), t->sh.enabled, t->am.enabled);
}

struct FramePass {
    bool (*on)(const vf_terrain *);
    FramePassRun *run;
    const char *sharded, *batched;       // why a handle that has it on is not sharded / draws no batch
};
enum { kPassShadows, kPassAmbient, kPassDrape, kPassFlood, kPassSpill, kPassExposure, kPassCumulative, kPassViewshed, kPassHaze, kFramePasses };
static const FramePass kFramePassTable[kFramePasses] = {
    { [](const vf_terrain *t) { return t->sh.enabled; }, light_pass, "the handle has shadows enabled: shadows need a whole-frame handle",
      "render_batch on a handle with shadows enabled is not supported: a sun per pose would need a shadow field per pose" },
    // (with shadows on, their row draws both and, tested first, refuses for both)
    { [](const vf_terrain *t) { return t->am.enabled && !t->sh.enabled; }, light_pass, "the handle has ambient occlusion enabled: it needs a whole-frame handle",
      "render_batch on a handle with ambient occlusion enabled is not supported" },
    { [](const vf_terrain *t) { return t->dr.iw != 0u; }, drape_pass, "the handle holds a draped image: it needs a whole-frame handle",
      "render_batch on a handle that holds a draped image is not supported" },                    // (4j: behind the shadow / ambient pass)
    { [](const vf_terrain *t) { return t->fd.fill.enabled; }, flood_pass, "the handle has a flood enabled: it needs a whole-frame handle",
      "render_batch on a handle with a flood enabled is not supported" },                         // (4s: on the surface, under the analysis tints)
    { [](const vf_terrain *t) { return t->sp.fill.enabled; }, spill_pass, "the handle has the spill enabled: it needs a whole-frame handle",
      "render_batch on a handle with the spill enabled is not supported" },                       // (4t: directly behind the flood's water)
    { [](const vf_terrain *t) { return t->se.enabled; }, exposure_pass, "the handle has sun exposure enabled: it needs a whole-frame handle",
      "render_batch on a handle with sun exposure enabled is not supported" },                    // (4n: behind both viewshed tints)
    { [](const vf_terrain *t) { return t->cv.enabled; }, cumulative_pass, "the handle has a cumulative viewshed enabled: it needs a whole-frame handle",
      "render_batch on a handle with a cumulative viewshed enabled is not supported" },           // (4m: behind the single observer's)
    { [](const vf_terrain *t) { return t->vs.enabled; }, viewshed_pass, "the handle has a viewshed enabled: it needs a whole-frame handle",
      "render_batch on a handle with a viewshed enabled is not supported" },                      // (4l)
    { [](const vf_terrain *t) { return t->hz.enabled; }, haze_pass, "the handle has haze enabled: it needs a whole-frame handle",
      "render_batch on a handle with haze enabled is not supported" },                            // (4q: between the eye and the painted surface)
};
// The refusals are tested in the order the features came, which decides the message when several are on.  Supersampling (4o) is no
// row -- its resolve rewrites the frame, not the samples -- but is refused among them, behind the first `ss_at` rows.  batch: for
// render_batch and render_batch_host, else for the shard calls.  NULL: nothing is refused.
static const int kRefusalOrder[kFramePasses] = { kPassShadows, kPassAmbient, kPassDrape, kPassViewshed, kPassCumulative, kPassExposure, kPassHaze,
                                                 kPassFlood, kPassSpill };
static const char *pass_refusal(const vf_terrain *t, bool batch, int ss_at = kFramePasses)
{
    for (int k = 0; k < kFramePasses && !(k == ss_at && t->ss > 1u); ++k) {
        const FramePass &R = kFramePassTable[kRefusalOrder[k]];
        if (R.on(t)) return batch ? R.batched : R.sharded;
    }
    if (t->ss <= 1u) return nullptr;
    return batch ? "render_batch on a supersampled handle is not supported: render the poses one by one (vf_terrain_render)"
                 : "the handle is supersampled: the resolve needs a whole-frame handle";
}

// The shard layout has changed (the caller has waited for the frame in flight): nothing rendered under the new one yet, and the tile
// numbering is another -- forget the scheduling feedback of the previous layout
static int reset_layout_feedback(vf_terrain *t)
{
    t->rendered = false; t->have_frame = false;
    t->cursor.frames_since_reset = 0;
    VF_HIP_TRY(sync_sides(t));
    for (auto &S : t->ps) {
        if (!S.slab) continue;                             // (a state not used yet starts at zero when it is made)
        VF_HIP_TRY(hipMemset(S.feedback, 0, feedback_words(t) * sizeof(uint32_t)));
        VF_HIP_TRY(hipMemset(S.background, 0, (size_t)t->ntx * t->nty * sizeof(uint32_t)));
        S.have_u_used = false;
    }
    for (auto &S : t->ps) { S.geom_stamp = S.height_stamp = 0; S.list_stamp = 0; }   // (k_block_boxes dropped the blocks of the other layout's tiles)
    return VF_OK;
}

int vf_terrain_set_shard(vf_terrain *t, uint32_t rank, uint32_t nranks, uint32_t band_h)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (nranks == 0 || rank >= nranks) return fail(VF_ERR_INVALID, "rank must be < nranks");
    if (!is_pow2(band_h) || band_h < (uint32_t)kTileH) return fail(VF_ERR_INVALID, "band_h must be a power of two >= 64 (the tile height)");
    if (!t->ov.layer.empty()) return fail(VF_ERR_INVALID, "the handle has overlays: sharded compositing is not supported (vf_terrain_clear_overlays first)");
    if (const char *why = nranks != 1 ? pass_refusal(t, false, 6) : nullptr) return fail(VF_ERR_INVALID, why);   // (supersampling: behind sun exposure)
    VF_HIP_TRY(wait_frame(t));
    t->inputs_gen++;
    t->geom_gen++;                                         // (rank, nranks and the band height decide which blocks k_block_boxes keeps)
    VF_HIP_TRY(drop_preplan(t));
    t->rank = rank; t->nranks = nranks; t->band_h = band_h;
    t->shard_tiles = false; t->use_map = false;
    t->local_rows = compute_local_rows(t->H, rank, nranks, band_h);
    t->local_tiles = t->ntx * ((t->local_rows + kTileH - 1) / kTileH);
    return reset_layout_feedback(t);
}

int vf_tile_layout(uint32_t width, uint32_t height, uint32_t rank, uint32_t nranks, uint32_t skew, uint32_t *tiles, uint32_t capacity,
                   uint32_t *count)
{
    if (!count) return fail(VF_ERR_INVALID, "NULL argument");
    if (width == 0 || height == 0 || nranks == 0 || rank >= nranks) return fail(VF_ERR_INVALID, "empty frame or rank >= nranks");
    if (!layout_valid(skew)) return fail(VF_ERR_INVALID, "layout word is neither VF_TILE_LAYOUT(skew < 65536, stripe_log2 <= 15) nor a registered stripe map");
    const uint32_t ntx = (width + kTileW - 1) / kTileW, nty = (height + kTileH - 1) / kTileH;
    if (ntx > 0xFFFFu || nty > 0xFFFFu) return fail(VF_ERR_INVALID, "frame too large");
    const StripeMap *m = layout_map(skew);
    if (m && (m->nranks != nranks || ((ntx - 1u) >> m->shift) >= m->owner.size()))
        return fail(VF_ERR_INVALID, "the registered stripe map was made for another number of ranks or a narrower frame");
    uint32_t n = 0;
    for (uint32_t ty = 0; ty < nty; ++ty)
        for (uint32_t tx = 0; tx < ntx; ++tx)
            if (layout_owner(skew, m, tx, ty, nranks) == rank) {
                if (tiles && n < capacity) tiles[n] = tx | (ty << 16);
                ++n;
            }
    *count = n;
    return VF_OK;
}

int vf_tile_layout_register_map(const uint8_t *stripe_owner, uint32_t nstripes, uint32_t stripe_log2, uint32_t nranks, uint32_t *layout)
{
    if (!stripe_owner || !layout) return fail(VF_ERR_INVALID, "NULL argument");
    if (nstripes == 0 || nstripes > kMaxStripes || stripe_log2 > 15u || nranks == 0 || nranks > 255u) return fail(VF_ERR_INVALID, "1..256 stripes, stripe_log2 <= 15, 1..255 ranks");
    for (uint32_t k = 0; k < nstripes; ++k) if (stripe_owner[k] >= nranks) return fail(VF_ERR_INVALID, "a stripe's owner is not a rank");
    std::lock_guard<std::mutex> lk(g_maps_mu);
    g_maps.reserve(kMaxStripeMaps);                        // (never reallocated: layout_map hands out pointers)
    for (uint32_t id = 0; id < g_maps.size(); ++id)        // the same table again: the same word (every rank registers its own copy)
        if (g_maps[id].shift == stripe_log2 && g_maps[id].nranks == nranks && g_maps[id].owner.size() == nstripes &&
            std::memcmp(g_maps[id].owner.data(), stripe_owner, nstripes) == 0) { *layout = kLayoutMapBit | (id << 21) | (stripe_log2 << 16); return VF_OK; }
    if (g_maps.size() >= kMaxStripeMaps) return fail(VF_ERR_INVALID, "too many registered stripe maps (64 per process)");
    StripeMap m;
    m.owner.assign(stripe_owner, stripe_owner + nstripes); m.shift = stripe_log2; m.nranks = nranks;
    g_maps.push_back(std::move(m));
    *layout = kLayoutMapBit | ((uint32_t)(g_maps.size() - 1u) << 21) | (stripe_log2 << 16);
    return VF_OK;
}

int vf_balance_stripes(const float *stripe_ms, uint32_t nstripes, uint32_t nranks, uint8_t *stripe_owner)
{
    if (!stripe_ms || !stripe_owner) return fail(VF_ERR_INVALID, "NULL argument");
    if (nranks == 0 || nranks > 255u || nstripes == 0 || nstripes > kMaxStripes || nstripes % nranks) return fail(VF_ERR_INVALID, "the stripes must divide evenly among 1..255 ranks");
    // Heaviest stripe first, each to the least loaded rank that still has room (every rank ends up with nstripes / nranks stripes: the
    // slabs and the exchange's chunks keep their sizes); then stripes of the most loaded rank are swapped against lighter ones of the
    // others for as long as that lowers the heavier of the two loads; and the round-robin deal itself is kept when nothing beat it.
    // Ties by stripe number / rank number: the same input gives the same table on every rank.  Times that are not finite count as zero.
    std::vector<uint32_t> order(nstripes);
    for (uint32_t k = 0; k < nstripes; ++k) order[k] = k;
    auto cost = [&](uint32_t k) { const float v = stripe_ms[k]; return std::isfinite(v) && v > 0.0f ? (double)v : 0.0; };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost(a) > cost(b); });
    std::vector<double> load(nranks, 0.0);
    std::vector<uint32_t> have(nranks, 0u);
    std::vector<uint8_t> own(nstripes, 0);
    const uint32_t room = nstripes / nranks;
    for (uint32_t k : order) {
        uint32_t best = nranks;
        for (uint32_t r = 0; r < nranks; ++r)
            if (have[r] < room && (best == nranks || load[r] < load[best])) best = r;
        own[k] = (uint8_t)best; load[best] += cost(k); have[best]++;
    }
    for (uint32_t round = 0; round < 4u * nstripes; ++round) {
        uint32_t hot = 0;
        for (uint32_t r = 1; r < nranks; ++r) if (load[r] > load[hot]) hot = r;
        double gain = 1e-12 * (load[hot] + 1.0);
        uint32_t sa = nstripes, sb = nstripes;
        for (uint32_t a = 0; a < nstripes; ++a) {
            if (own[a] != hot) continue;
            for (uint32_t b = 0; b < nstripes; ++b) {
                const uint32_t r = own[b];
                if (r == hot || !(cost(b) < cost(a))) continue;
                const double d = cost(a) - cost(b);         // moves from the hot rank to r
                const double worst = std::fmax(load[hot] - d, load[r] + d);
                if (load[hot] - worst > gain) { gain = load[hot] - worst; sa = a; sb = b; }
            }
        }
        if (sa == nstripes) break;
        const uint32_t r = own[sb];
        const double d = cost(sa) - cost(sb);
        load[hot] -= d; load[r] += d; own[sa] = (uint8_t)r; own[sb] = (uint8_t)hot;
    }
    std::vector<double> rr(nranks, 0.0);
    for (uint32_t k = 0; k < nstripes; ++k) rr[k % nranks] += cost(k);
    const bool keep_round_robin = *std::max_element(rr.begin(), rr.end()) <= *std::max_element(load.begin(), load.end());
    for (uint32_t k = 0; k < nstripes; ++k) stripe_owner[k] = keep_round_robin ? (uint8_t)(k % nranks) : own[k];
    return VF_OK;
}

int vf_terrain_tile_times(vf_terrain *t, float *ms, uint32_t capacity, uint32_t *count)
{
    if (!t || !count) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->rendered) return fail(VF_ERR_INVALID, "nothing rendered yet");
    int rc = vf_terrain_sync(t);
    if (rc != VF_OK) return rc;
    const uint32_t n = std::min(capacity, t->local_tiles);
    std::vector<uint32_t> ticks(n);
    if (n && ms) {
        VF_HIP_TRY(hipMemcpy(ticks.data(), t->ps[t->last_set].feedback, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < n; ++k) ms[k] = (float)ticks[k] * 1e-5f;      // 10 ns ticks of the 100 MHz clock
    }
    *count = t->local_tiles;
    return VF_OK;
}

int vf_terrain_set_tile_shard(vf_terrain *t, uint32_t rank, uint32_t nranks, uint32_t skew)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (nranks == 0 || rank >= nranks) return fail(VF_ERR_INVALID, "rank must be < nranks");
    if (!layout_valid(skew)) return fail(VF_ERR_INVALID, "layout word is neither VF_TILE_LAYOUT(skew < 65536, stripe_log2 <= 15) nor a registered stripe map");
    if (!t->ov.layer.empty()) return fail(VF_ERR_INVALID, "the handle has overlays: sharded compositing is not supported (vf_terrain_clear_overlays first)");
    if (const char *why = pass_refusal(t, false, 4)) return fail(VF_ERR_INVALID, why);      // (supersampling: behind the viewshed)
    VF_HIP_TRY(wait_frame(t));
    std::vector<uint32_t> map((size_t)t->ntx * t->nty);
    uint32_t n = 0;
    int rc = vf_tile_layout(t->W, t->H, rank, nranks, skew, map.data(), (uint32_t)map.size(), &n);
    if (rc != VF_OK) return rc;
    VF_HIP_TRY(sync_sides(t));                                // (k_block_boxes of a frame in flight reads the owner table)
    const StripeMap *sm = layout_map(skew);
    t->geom_gen++;                                            // before the first byte of the owner table changes: k_block_boxes reads the table, the stripe width, the skew and the rank
    if (sm) VF_HIP_TRY(hipMemcpy(t->d_stripe_owner, sm->owner.data(), sm->owner.size(), hipMemcpyHostToDevice));
    t->use_map = sm != nullptr;
    if (n) VF_HIP_TRY(hipMemcpy(t->d_tile_map, map.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    t->inputs_gen++;
    VF_HIP_TRY(drop_preplan(t));
    t->shard_tiles = true; t->local_tiles = n;
    t->rank = rank; t->nranks = nranks; t->skew = skew;
    t->local_rows = 0;                                   // row-oriented accessors do not apply to a tile-major buffer
    return reset_layout_feedback(t);
}

int vf_terrain_local_tiles(const vf_terrain *t, uint32_t *tiles)
{
    if (!t || !tiles) return fail(VF_ERR_INVALID, "NULL argument");
    *tiles = t->local_tiles;
    return VF_OK;
}

int vf_terrain_read_tiles(vf_terrain *t, uint8_t *dst, uint32_t first, uint32_t count)
{
    if (!t || !dst) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->shard_tiles) return fail(VF_ERR_INVALID, "handle is not tile-sharded");
    if (!t->rendered) return fail(VF_ERR_INVALID, "nothing rendered yet");
    if ((uint64_t)first + count > t->local_tiles) return fail(VF_ERR_INVALID, "tile range outside the local tiles");
    int rc = vf_terrain_sync(t);
    if (rc != VF_OK) return rc;
    const size_t tile_px = (size_t)kTileW * kTileH;
    VF_HIP_TRY(hipMemcpy(dst, t->d_rgba + first * tile_px, count * tile_px * 4, hipMemcpyDeviceToHost));
    return VF_OK;
}

int vf_terrain_local_rows(const vf_terrain *t, uint32_t *rows)
{
    if (!t || !rows) return fail(VF_ERR_INVALID, "NULL argument");
    *rows = t->ss > 1u ? t->oH : t->local_rows;             // rows of the frame handed out (a supersampled handle is a whole-frame handle)
    return VF_OK;
}

int vf_terrain_set_output_device(vf_terrain *t, void *dev_rgba)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    t->d_rgba = dev_rgba ? (uint32_t *)dev_rgba : t->d_rgba_own;
    return VF_OK;
}

int vf_terrain_rgba_device(const vf_terrain *t, void **dev_rgba)
{
    if (!t || !dev_rgba) return fail(VF_ERR_INVALID, "NULL argument");
    *dev_rgba = t->d_rgba;
    return VF_OK;
}

static void build_params(const vf_terrain *t, const FrameInputs &in, FrameParams &P)
{
    const float *u = in.u;
    std::memcpy(P.view, u, 64);
    std::memcpy(P.proj, u + 16, 64);
    P.spacing = spacing_of(u);       // terrain.wgsl:46
    P.exag = u[38];
    P.h_range = std::fmax(u[37], 1e-8f);       // terrain.wgsl:71
    P.exposure = u[35];
    {   // L = normalize(sun), terrain.wgsl:83 -- uniform per frame, evaluated once with the same IEEE ops
        float sx = u[32], sy = u[33], sz = u[34];
        float inv = 1.0f / std::sqrt(std::fmaf(sz, sz, std::fmaf(sy, sy, sx * sx)));
        P.Lx = sx * inv; P.Ly = sy * inv; P.Lz = sz * inv;
    }
    P.hw = 0.5f * (float)t->W; P.hh = 0.5f * (float)t->H;
    P.step = grid_step(t);
    P.n = t->n; P.nm1 = t->n - 1; P.nb = t->nb;
    P.W = t->W; P.H = t->H; P.ntx = t->ntx; P.nty = t->nty; P.tw = t->tw; P.th = t->th;
    P.rank = t->rank; P.nranks = t->nranks; P.band_h = t->band_h; P.band_shift = ilog2(t->band_h);
    P.local_rows = t->local_rows;
    P.shard_tiles = t->shard_tiles ? 1u : 0u; P.tile_map = t->d_tile_map; P.skew = layout_skew(t->skew); P.stripe_shift = layout_shift(t->skew);
    P.stripe_owner = t->shard_tiles && t->use_map ? t->d_stripe_owner : nullptr;
    P.shade_mode = in.shade_mode; P.tex = t->d_height;
    P.inv2hr = 1.0f / (2.0f * P.h_range);
    {   // cell / nm1 as mulhi(cell, m) >> s, exact for cell < 2^26 (nm1 < 2^13): s = 31 + ceil(log2 nm1) - 32, m = ceil(2^(s + 32) / nm1)
        const uint32_t d = P.nm1;
        if (d <= 1u) { P.div_m = 0u; P.div_s = 0u; }       // one cell: row 0
        else {
            const uint32_t L = ilog2(d);                   // ceil(log2 d)
            P.div_s = L - 1u;
            P.div_m = (uint32_t)((((uint64_t)1 << (31u + L)) + d - 1u) / d);
        }
    }
    const SrgbTables &T = tables();
    P.clear_rgba = T.encode(0.02f) | (T.encode(0.02f) << 8) | (T.encode(0.03f) << 16) | 0xFF000000u;   // src/terrain/mod.rs:421
}

// How far, in pixels, the terrain's footprint moved on the screen between two cameras (corners of the xz square at y = 0).
// Scheduling feedback is per screen tile: once the picture has moved by about a tile, an older frame's tile times describe
// other content.  A corner behind either camera counts as "moved".
static float camera_shift_px(const vf_terrain *t, const float *a, const float *b)
{
    const float ext = 1.5f * spacing_of(t->inputs.u);
    float worst = 0.0f;
    for (int c = 0; c < 4; ++c) {
        const float p[4] = { (c & 1) ? ext : -ext, 0.0f, (c & 2) ? ext : -ext, 1.0f };
        float xy[2][2];
        for (int k = 0; k < 2; ++k) {
            const float *u = k ? b : a;                    // column-major view (u[0..16)) and proj (u[16..32))
            float v[4], q[4];
            for (int r = 0; r < 4; ++r) v[r] = u[r] * p[0] + u[4 + r] * p[1] + u[8 + r] * p[2] + u[12 + r] * p[3];
            for (int r = 0; r < 4; ++r) q[r] = u[16 + r] * v[0] + u[20 + r] * v[1] + u[24 + r] * v[2] + u[28 + r] * v[3];
            if (!(q[3] > 1e-6f)) return 1e9f;
            xy[k][0] = q[0] / q[3] * 0.5f * (float)t->W; xy[k][1] = q[1] / q[3] * 0.5f * (float)t->H;
        }
        worst = std::fmax(worst, std::fmax(std::fabs(xy[0][0] - xy[1][0]), std::fabs(xy[0][1] - xy[1][1])));
    }
    return worst;
}
// Homography of the ground plane y = 0 from the screen of camera `now` to the screen of camera `then` (both: view u[0..16), proj
// u[16..32), column-major; pixels): a point (X, 0, Z) of the plane projects to A G (X, Z, 1) with G the columns x, z, w / rows x, y, w
// of proj * view and A the viewport; the map is (A G_then) (A G_now)^-1.  False when the plane is (nearly) edge-on for `now`.
static bool motion_map(const vf_terrain *t, const float *then, const float *now, MotionMap &M)
{
    const double hw = 0.5 * t->W, hh = 0.5 * t->H;
    auto plane = [&](const float *u, double g[9]) {
        double vp[16];                                     // proj * view, column-major
        for (int c = 0; c < 4; ++c)
            for (int r = 0; r < 4; ++r) {
                double a = 0.0;
                for (int k = 0; k < 4; ++k) a += (double)u[16 + 4 * k + r] * (double)u[4 * c + k];
                vp[4 * c + r] = a;
            }
        const int cols[3] = { 0, 2, 3 };
        for (int j = 0; j < 3; ++j) {
            const double cx = vp[4 * cols[j] + 0], cy = vp[4 * cols[j] + 1], cw = vp[4 * cols[j] + 3];
            g[0 + j] = hw * cx + hw * cw; g[3 + j] = -hh * cy + hh * cw; g[6 + j] = cw;      // row-major 3 x 3
        }
    };
    double a[9], b[9];
    plane(then, a); plane(now, b);
    const double det = b[0] * (b[4] * b[8] - b[5] * b[7]) - b[1] * (b[3] * b[8] - b[5] * b[6]) + b[2] * (b[3] * b[7] - b[4] * b[6]);
    double scale = 0.0;
    for (double v : b) scale = std::fmax(scale, std::fabs(v));
    if (!(std::fabs(det) > 1e-12 * scale * scale * scale)) return false;
    const double inv[9] = { (b[4] * b[8] - b[5] * b[7]) / det, (b[2] * b[7] - b[1] * b[8]) / det, (b[1] * b[5] - b[2] * b[4]) / det,
                            (b[5] * b[6] - b[3] * b[8]) / det, (b[0] * b[8] - b[2] * b[6]) / det, (b[2] * b[3] - b[0] * b[5]) / det,
                            (b[3] * b[7] - b[4] * b[6]) / det, (b[1] * b[6] - b[0] * b[7]) / det, (b[0] * b[4] - b[1] * b[3]) / det };
    double m[9], big = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) { m[3 * r + c] = a[3 * r] * inv[c] + a[3 * r + 1] * inv[3 + c] + a[3 * r + 2] * inv[6 + c]; big = std::fmax(big, std::fabs(m[3 * r + c])); }
    if (!(big > 0.0) || !std::isfinite(big)) return false;
    // (homogeneous: any POSITIVE scale -- w' = w_then / w_now is positive for plane points in front of both cameras, which is what
    //  k_plan asks of a landing point; keep the floats in range)
    for (int k = 0; k < 9; ++k) M.m[k] = (float)(m[k] / big);
    M.on = 1u;
    return true;
}
constexpr float kFreshFeedbackPx = 24.0f;   // from here on (3/8 of a tile per frame) the plan waits for the previous frame's feedback

#ifndef VF_GROUPS_MAX_RANKS
#define VF_GROUPS_MAX_RANKS 8    // handles sharded over this many ranks or more take the tile kernel without line groups
#endif
// the fast fragment path exists for fs_main as coded; the documented-only SPEC_T32 stage always takes the exact arithmetic
static bool fast_shading(const FrameInputs &in) { return in.precision == VF_PRECISION_FAST && in.shade_mode == VF_SHADE_REFERENCE; }

// The per-tile candidate lists of plan state S (k_tile_lists, vf_kernels.h), queued on `on`: behind the set-up pass whose records they
// are read from and behind the last frame that read this state's lists, never in front of a frame.  The buffers are made by the first
// builder of the state -- a one-shot render and a moving camera never pay for them.  SIZE: the entries are the (tile, block) pairs whose
// box meets the tile, which only the device knows; the buffer is sized from what the host knows -- two units (16 B) per grid block plus
// 512 per local tile, at most kTileListMaxUnits (64 MiB) -- and a tile that finds it full goes without (DESIGN.md 3 has the fill).
constexpr size_t kTileListMaxUnits = (size_t)4 << 20;
static bool lists_valid(const vf_terrain *t, const vf_terrain::PlanState &S)
{
    return S.list_stamp != 0 && S.list_stamp == S.geom_stamp && S.geom_stamp == t->geom_gen && S.height_stamp == t->height_gen;
}
static hipError_t queue_tile_lists(vf_terrain *t, vf_terrain::PlanState &S, const FrameParams &P, hipStream_t on)
{
    const uint32_t ntiles = t->local_tiles;
    if (t->tl_off || t->tl_failed || !ntiles || !S.slab || S.geom_stamp == 0) return hipSuccess;
    if (!S.tl_ent) {
        const size_t all_tiles = (size_t)t->ntx * t->nty;
        const size_t units = std::min<size_t>(kTileListMaxUnits, 2 * (size_t)t->nblocks + 512 * (size_t)ntiles);
        hipError_t e = hipMalloc((void **)&S.tl_ent, units * sizeof(uint4));
        if (e == hipSuccess) e = hipMalloc((void **)&S.tl_hdr, (all_tiles + 2) * sizeof(uint4));      // (+ 2: the control words behind the headers)
        if (e == hipSuccess && !S.listed) e = hipEventCreateWithFlags(&S.listed, hipEventDisableTiming);
        if (e != hipSuccess) {                              // no memory for them: the handle draws as it always has
            if (S.tl_ent) (void)hipFree(S.tl_ent);
            if (S.tl_hdr) (void)hipFree(S.tl_hdr);
            S.tl_ent = S.tl_hdr = nullptr;
            t->tl_failed = true;
            (void)hipGetLastError();
            return hipSuccess;
        }
        S.tl_ctl = reinterpret_cast<uint32_t *>(S.tl_hdr + all_tiles);
        S.tl_units = (uint32_t)units;
    }
    const size_t rc_n = (size_t)t->nb * t->ntx;
    hipError_t e = hipStreamWaitEvent(on, S.set_up, 0);
    if (e == hipSuccess) e = hipStreamWaitEvent(on, S.drawn, 0);        // (a frame that still reads the lists this builder writes over)
    if (e == hipSuccess) e = hipMemsetAsync(S.tl_ctl, 0, 8 * sizeof(uint32_t), on);
    if (e != hipSuccess) return e;
    S.tl_cap = std::min(S.tl_units, t->tl_cap_debug);
    hipLaunchKernelGGL(k_tile_lists, dim3(ntiles), dim3(256), 0, on, P, S.row_ranges, S.recs, S.cap_seg, S.cap_rad, S.rc, S.rc + rc_n,
                       S.tl_ent, S.tl_hdr, S.tl_ctl, S.tl_cap);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(S.listed, on);
    if (e == hipSuccess) S.list_stamp = S.geom_stamp;
    return e;
}
// ... for the caller that waits for its frames: the job noted by render_impl, behind whatever `s` holds by now
static void flush_tile_lists(vf_terrain *t, hipStream_t s)
{
    if (!t->tl_job.pending) return;
    t->tl_job.pending = false;
    vf_terrain::PlanState &S = t->ps[t->tl_job.set];
    // (the records must still be the ones the frame was drawn from, and the live geometry theirs)
    if (S.geom_stamp == 0 || S.geom_stamp != t->tl_job.geom || S.geom_stamp != t->geom_gen || S.height_stamp != t->height_gen || t->bounds_dirty) return;
    if (lists_valid(t, S)) return;
    if (queue_tile_lists(t, S, t->tl_job.P, s) != hipSuccess) (void)hipGetLastError();
}

// A frame in two halves (round 5).  plan_frame: everything up to the plan's last kernel -- block boxes, set-up pass, plan, sort -- on the
// side streams (a handle's first frame: on `s`); it touches plan state only.  draw_frame: the kernels on the caller's stream.  What the
// second half needs of the first travels in a FramePlan, so that the first half of the NEXT frame can be queued ahead of its call
// (vf_terrain::pre, render_impl).
static int plan_frame(vf_terrain *t, hipStream_t s, FramePlan &K, bool streaming = false, bool ahead = false)
{
    FrameParams &P = K.P;
    PlanCursor &C = t->cursor;
    const float *u = t->inputs.u;
    build_params(t, t->inputs, P);
    AxisTables A = axis(t);
    const uint32_t ntiles = t->local_tiles;
    const uint32_t set = C.cur_set;
    C.cur_set = (set + 1u) % vf_terrain::kPlanStates;
    C.frame_no++;
    // A handle's FIRST frame runs on the caller's stream alone, plan and set-up included: its chain is serial anyway (the static plan
    // estimate reads the set-up pass's records) and there is no earlier frame to hide anything under.  The side streams and the second
    // plan chain's events come into play with the second frame.
    // ... and so do the frames of a caller that waits for each of them (round 6): the plan streams are made for the caller that
    // streams -- a frame arriving while the previous one is in flight -- or borrowed when the context already has them.
    if (!t->side && C.frame_no > 1u) {
        bool have = false;
        { std::lock_guard<std::mutex> lk(t->ctx->lazy_mu); have = t->ctx->side && t->ctx->side2; }
        if (have || streaming || t->want_plan_streams) VF_HIP_TRY(ctx_side_streams(t->ctx, &t->side, &t->side2));   // (the context's: made once per process)
    }
    const bool solo = !t->side;
    VF_HIP_TRY(ensure_plan_state(t, set, solo ? s : t->side));
    vf_terrain::PlanState &S = t->ps[set], &O = t->ps[t->last_set];       // this frame's plan state, the previous frame's
    // A camera at rest (or moving slowly) plans under the previous frame's tile kernel with the feedback of the frame before it;
    // a camera that moves the picture by a good part of a tile per frame waits for the previous frame instead and uses ITS feedback:
    // the plan then costs its own time (k_plan + k_plan_sort after the tile kernel), stale feedback costs more (64-pose orbit
    // at 1920x1080, grid 2048: 0.80 -> 0.61 ms per pose together with the dilated weights in k_plan; tools/exp_orbit.py).
    float shift = 0.0f;
    if (C.have_drawn) {
        shift = camera_shift_px(t, C.u_drawn, u);
        if (shift > kFreshFeedbackPx) C.camera_moving = true;                  // (SAME GEOMETRY by construction: view and projection alone) hysteresis: frames that alternate between the two
        else if (shift < 0.5f * kFreshFeedbackPx) C.camera_moving = false;     // modes get the worst of both
    }
    // (one more frame after the motion stops: the frame before last still shows the old view, the last one the new)
    // ... and the second frame of a handle: its own plan state has no times yet, the first frame's has
    // ... and the frames of a handle whose own plan state has no times yet (the sets take turns): the previous frame's has
    // Round 5: a moving camera's plan no longer waits either when this set's times can be looked up THROUGH the motion (k_plan,
    // MotionMap): the homography of the ground plane between this frame's screen and the screen of the frame before last.  What is
    // left of the waiting mode: a handle's second frame, sharded handles (their feedback is per local tile), a jump cut (the view of
    // two frames ago shares little with this one: the previous frame's times, dilated, are the better guess), an edge-on plane.
    const bool young = C.frames_since_reset >= 1 && C.frames_since_reset < vf_terrain::kPlanStates;
    MotionMap M;
    std::memset(&M, 0, sizeof M);
    if ((C.camera_moving || C.was_moving) && !young && C.frames_since_reset >= vf_terrain::kPlanStates && S.have_u_used && t->nranks == 1u && !t->shard_tiles &&
        camera_shift_px(t, S.u_used, u) < 0.4f * (float)std::max(t->W, t->H))
        (void)motion_map(t, S.u_used, u, M);
    const bool after_drop = t->replan_fresh && C.frames_since_reset >= vf_terrain::kPlanStates;   // (a handle's first frames have their own rules)
    t->replan_fresh = false;
    if (after_drop) M.on = 0u;                              // (the motion map reads this set's times too)
    const bool fresh = young || after_drop || ((C.camera_moving || C.was_moving) && !M.on);
    const bool first = C.frames_since_reset == 0;           // no tile times at all yet: a static estimate stands in (k_plan_estimate)
    C.frames_since_reset++;
    const bool motion_starts = C.camera_moving && !C.was_moving;
    C.was_moving = C.camera_moving;
    const bool dilate = fresh || shift > 0.5f * kFreshFeedbackPx;     // slower motion: still overlapped, but the tile weights spread to the neighbours
    std::memcpy(C.u_drawn, u, sizeof C.u_drawn);
    C.have_drawn = true;
    hipStream_t side = solo ? s : t->side, side2 = solo ? s : t->side2;
    // (the plan's three timing events belong to its plan state, not to a slot of the frame ring: a plan queued ahead of its call has no
    //  place in the ring yet -- advisor, round 5 -- and the ring's events sit on the draw stream, where every record costs the frame)
    K.sampled = t->timing_every <= 1u || C.frame_no % t->timing_every == 0u;
    // (not at timing level 3: an event record between two kernels of the plan chain delays the chain, and a plan that is late holds its frame's
    //  tile kernel back -- three records per plan cost a C4 frame 2.5 %, on the plan streams as on the draw stream)
    const bool timed = t->timing && t->timing_every <= 1u && S.pev[0] != nullptr;
    hipEvent_t *ev = S.pev;
    S.pev_valid = timed;
    // ---- plan, on the side stream: needs this set back from the frame before last, then touches plan state only ----
    VF_HIP_TRY(hipStreamWaitEvent(side, S.drawn, 0));
    if (t->bounds_dirty) {
        // the height texture may have been produced by work queued on the caller's stream: order the cache rebuild after it
        VF_HIP_TRY(hipEventRecord(t->entry, s));
        VF_HIP_TRY(hipStreamWaitEvent(side, t->entry, 0));
        hipLaunchKernelGGL(k_height_blocks, dim3(t->nblocks), dim3(64), 0, side, t->n, t->nb, t->tw, A, t->d_height, t->d_hblk, t->d_bounds);
        VF_HIP_TRY(hipGetLastError());
        VF_HIP_TRY(hipEventRecord(t->cached, side));
        t->cached_on = side;
        t->bounds_dirty = false;
        for (auto &X : t->ps) { X.geom_stamp = X.height_stamp = 0; X.list_stamp = 0; }   // (whatever the generations say: nothing was built from this cache)
    }
    if (t->cached_on && t->cached_on != side) {             // the cache was last rebuilt on another stream: this chain (and, through S.boxed and S.planned, the set-up pass and the draw) comes after it
        VF_HIP_TRY(hipStreamWaitEvent(side, t->cached, 0));
        t->cached_on = side;
    }
    // This set's boxes, ranges, segment list, records, masks and vertex records are a pure function of the geometry inputs: when they
    // were built from the live generations they are left as they are (S.boxed and S.set_up keep their last record: completed long ago).
    // After a geometry change each of the two sets pays the full pass once.
    const bool reuse = S.geom_stamp != 0 && S.geom_stamp == t->geom_gen && S.height_stamp == t->height_gen;
    if (timed) VF_HIP_TRY(hipEventRecord(ev[0], side));
    const size_t rc_n = (size_t)t->nb * t->ntx;
    uint32_t *rc_lo = S.rc, *rc_hi = S.rc + rc_n;
    // the split quantum comes from the same tile times the plan will read: summed by an extra workgroup of k_block_boxes, or --
    // when those times belong to the frame still being drawn -- by a kernel of its own after the wait below
    uint32_t *quantum = S.feedback + (size_t)t->ntx * t->nty;
    const uint32_t nsegs_all = grid_segments(t);
    uint32_t *seg_count = S.seg_list + nsegs_all;
    const uint32_t *const quantum_from = fresh || first ? (const uint32_t *)nullptr : S.feedback;
    if (reuse) {
        // the work of k_block_boxes' extra workgroup alone: this frame's queue words and split quantum, in front of k_plan.  The segment
        // counter stays at the zero k_clear left it at, and nothing is launched against it.
        hipLaunchKernelGGL(k_plan_begin, dim3(1), dim3(512), 0, side, quantum_from, t->ntx * t->nty, quantum, S.work_count);
    } else {
        S.geom_stamp = S.height_stamp = 0;                                  // half-written from here until both kernels are on their way
        S.list_stamp = 0;                                                   // (the candidate lists were built from the records that go now)
        if (S.listed) VF_HIP_TRY(hipStreamWaitEvent(side, S.listed, 0));    // ... and their builder, if it is still on its way, reads those records
        hipLaunchKernelGGL(k_block_boxes, dim3(t->nb + 1), dim3(t->nb > 256 ? 512 : 256), 0, side, P, t->d_bounds, S.ranges, S.row_ranges, S.cap_seg, S.cap_rad, rc_lo, rc_hi,
                           quantum_from, t->ntx * t->nty, quantum, S.work_count, S.recs, S.seg_list, seg_count);
        // vertex stage + tile-independent culling, once per geometry (streams ~1.3 KB per block into this frame's plan state): needs the
        // block boxes only, so it runs on a second stream beside k_plan / k_plan_sort -- all of them under the previous frame's tile kernel
        VF_HIP_TRY(hipEventRecord(S.boxed, side));
        VF_HIP_TRY(hipStreamWaitEvent(side2, S.boxed, 0));                  // (orders it after S.drawn and the height cache too)
        // (one short-lived workgroup per possible segment -- those beyond the list's length leave at once: workgroups that come and go
        //  share the CUs with the previous frame's tile kernel more smoothly than a few long-lived ones)
        hipLaunchKernelGGL(k_block_setup, dim3(nsegs_all), dim3(kSetupThreads), 0, side2,
                           P, t->d_hblk, S.ranges, S.vtx, S.recs, S.gen, S.seg_list, seg_count, S.band);
        VF_HIP_TRY(hipEventRecord(S.set_up, side2));
        VF_HIP_TRY(hipGetLastError());                                      // both launched without error: the stamp
        S.geom_stamp = t->geom_gen; S.height_stamp = t->height_gen;
    }
    // the candidate lists of a state whose records stand: read by this frame when they are of this generation; built otherwise -- on the
    // set-up stream, behind S.set_up, beside the plan chain and not on it: this frame does not wait for them and draws without.
    // Only where a frame in flight hides the builder: a plan made ahead, or a caller that streams.  A caller that waits for this
    // frame would wait for the builder too (it fills the GPU for 0.1 ms at C4 and the plan chain queues up behind it: +0.09 ms on a
    // handle's third frame): render_impl notes the job instead, and it goes out behind the frame.
    K.lists = reuse && ntiles && !t->tl_off && lists_valid(t, S);
    if (reuse && ntiles && !K.lists && !solo && (ahead || streaming)) VF_HIP_TRY(queue_tile_lists(t, S, P, side2));
    if (timed) VF_HIP_TRY(hipEventRecord(ev[1], side));
    if (ntiles) {
        if (fresh) {
            VF_HIP_TRY(hipStreamWaitEvent(side, O.drawn, 0));         // (the block boxes above did not need to wait)
            hipLaunchKernelGGL(k_quantum, dim3(1), dim3(512), 0, side, O.feedback, t->ntx * t->nty, quantum);
        } else if (first) {
            VF_HIP_TRY(hipStreamWaitEvent(side, S.set_up, 0));       // the estimate reads the set-up pass's block records
            hipLaunchKernelGGL(k_plan_estimate, dim3(ntiles), dim3(256), 0, side, P, S.row_ranges, S.recs, S.cap_seg, S.cap_rad, rc_lo, rc_hi, S.feedback);
            hipLaunchKernelGGL(k_quantum, dim3(1), dim3(512), 0, side, S.feedback, t->ntx * t->nty, quantum);
        }
        const vf_terrain::PlanState &F = fresh ? O : S;               // whose tile times steer this frame
        hipLaunchKernelGGL(k_plan, dim3(ntiles), dim3(256), 0, side, P, S.row_ranges, S.flags_new, S.work, S.work_count,
                           F.feedback, quantum, S.work_count + 1, rc_lo, rc_hi, dilate ? 1u : 0u, F.background, M);
        hipLaunchKernelGGL(k_plan_sort, dim3(1), dim3(256), 0, side, S.work, S.work_sorted, S.work_count, S.feedback, t->ntx * t->nty,
                           S.flags_new, S.background, ntiles);
    }
    VF_HIP_TRY(hipGetLastError());                              // a failed plan launch is reported here: the probe block below clears hipEventQuery's "not ready"
    if (timed) VF_HIP_TRY(hipEventRecord(ev[2], side));
    VF_HIP_TRY(hipEventRecord(S.planned, side));
    K.mode = (first ? VF_PLAN_FIRST : 0u) | (fresh ? VF_PLAN_FRESH : 0u) | (M.on ? VF_PLAN_MOTION_MAP : 0u) | (dilate ? VF_PLAN_DILATE : 0u) |
             (reuse ? VF_PLAN_GEOMETRY_REUSED : 0u) | (K.lists ? VF_PLAN_TILE_LISTS : 0u);
    K.set = set; K.ntiles = ntiles; K.motion_starts = motion_starts; K.rc_lo = rc_lo; K.rc_hi = rc_hi; K.seg_count = seg_count;
    return VF_OK;
}

// The overlay pass of a frame (vf_overlay.h), on the draw stream behind the tile kernels.  The pair list is sized by the frame's pair
// count, which the host reads back between the scan and the scatter: a handle with overlays waits once per frame for that word.
// With an occluding layer the tile kernels have stored the frame's visibility in d_vis (draw_frame), and the composite reads it.
// With a hazed layer on a handle whose haze is enabled with a density above zero, k_ov_haze_setup fills the layers'
// side records and k_ov_composite_haze composites; every other frame launches what it did before hazed layers existed.
// (their launches stand behind the haze pass's, at the end of this file: the kernels that were there before keep their places)
static void ov_haze_setup_launch(vf_terrain *t, hipStream_t s, const FrameParams &P);
static void ov_haze_composite_launch(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, uint32_t nbx, uint32_t nbins, bool occlude);
static int overlay_pass(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V)
{
    vf_terrain::Overlays &O = t->ov;
    const uint32_t nbx = (t->oW + kOvBin - 1u) / kOvBin, nby = (t->oH + kOvBin - 1u) / kOvBin, nbins = nbx * nby;   // (P is the output size's: output_params)
    const dim3 per_prim((O.nprims + 255u) / 256u), threads(256);
    const bool occlude = O.occluding != 0u;
    const bool hazed = O.hazed != 0u && t->hz.enabled && t->hz.density > 0.0f;
    if (hazed && (!O.hzrec.p || O.hzrec.cap < O.nprims)) return fail(VF_ERR_HIP, "overlays: the hazed layers' side records are missing");
    hipLaunchKernelGGL(k_ov_setup, per_prim, threads, 0, s, P, axis(t), O.nprims, O.in.p, O.prim.p, O.box.p, O.d_cnt, nbx,
                       occlude ? O.dep.p : nullptr);
    if (hazed) ov_haze_setup_launch(t, s, P);
    const dim3 per_slot((O.pg_hi - O.pg_lo + 255u) / 256u);
    if (O.nfill) {                                          // fill edges and headers: binned with the rest
        hipLaunchKernelGGL(k_pg_setup, per_slot, threads, 0, s, P, axis(t), O.pg_lo, O.pg_hi, O.in.p, O.prim.p, O.box.p, O.d_cnt, nbx, O.pg_fbox.p);
        hipLaunchKernelGGL(k_pg_header, dim3((O.nfill + 255u) / 256u), threads, 0, s, P, O.nfill, O.pg_hdr.p, O.in.p, O.pg_fbox.p, O.pg_fbin.p,
                           O.prim.p, O.box.p, O.d_cnt, nbx, O.pg_total.p);
    }
    hipLaunchKernelGGL(k_ov_scan, dim3(1), dim3(1024), 0, s, nbins, O.d_cnt, O.d_start);
    VF_HIP_TRY(hipGetLastError());
    VF_HIP_TRY(hipMemcpyAsync(O.h_total, O.d_start + nbins, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (O.nfill) {
        VF_HIP_TRY(hipMemcpyAsync(O.h_total + 2, O.pg_total.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        VF_HIP_TRY(hipMemsetAsync(O.pg_total.p, 0, sizeof(unsigned long long), s));
    }
    VF_HIP_TRY(hipEventRecord(O.counted, s));
    VF_HIP_TRY(hipEventSynchronize(O.counted));
    const uint32_t total = *O.h_total;
    unsigned long long words = 0;
    if (O.nfill) std::memcpy(&words, O.h_total + 2, sizeof words);
    // (k_ov_scan has zeroed the counts: a frame that stops here leaves them as the next one needs them, and stays as drawn)
    if (total == 0u) return VF_OK;                          // (nothing on screen)
    if (total == 0xFFFFFFFFu) return fail(VF_ERR_NOMEM, "overlays: more than 2^32 - 2 (primitive, screen bin) pairs in one frame");
    if (words > 0xFFFFFFFFull) return fail(VF_ERR_NOMEM, "overlays: polygon fills reach more than 2^32 - 1 (feature, screen bin) pairs in one frame");
    hipError_t e = O.mask.reserve(words, words + words / 2u + 4096u);
    if (e != hipSuccess) return fail(VF_ERR_NOMEM, std::string("polygon mask allocation failed: ") + hipGetErrorString(e));
    if (words) {                                            // the backdrop: row crossings right of each bin, per fill feature
        VF_HIP_TRY(hipMemsetAsync(O.mask.p, 0, (size_t)words * sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_pg_backdrop, per_slot, threads, 0, s, t->oH, O.pg_lo, O.pg_hi, O.in.p, O.prim.p, O.pg_fbin.p, O.mask.p);
        hipLaunchKernelGGL(k_pg_prefix, dim3((O.nfill + 3u) / 4u), threads, 0, s, O.nfill, O.pg_fbin.p, O.mask.p);
    }
    e = O.list.reserve(total, (size_t)total + total / 2u + 4096u);
    if (e != hipSuccess) return fail(VF_ERR_NOMEM, std::string("overlay pair list allocation failed: ") + hipGetErrorString(e));
    hipLaunchKernelGGL(k_ov_scatter, per_prim, threads, 0, s, O.nprims, O.box.p, nbx, O.d_start, O.d_cnt, O.list.p);
    if (hazed) ov_haze_composite_launch(t, s, P, V, nbx, nbins, occlude);
    else if (occlude)
        hipLaunchKernelGGL(k_ov_composite_occlude, dim3(nbins), threads, 0, s, t->oW, t->oH, nbx, O.prim.p, O.d_cnt, O.d_start, O.list.p, t->ctx->d_decode,
                           t->ctx->d_thresh, O.mask.p, t->d_rgba, P, V, t->d_vis, O.dep.p);
    else
        hipLaunchKernelGGL(k_ov_composite, dim3(nbins), threads, 0, s, t->oW, t->oH, nbx, O.prim.p, O.d_cnt, O.d_start, O.list.p, t->ctx->d_decode,
                           t->ctx->d_thresh, O.mask.p, t->d_rgba);
    VF_HIP_TRY(hipGetLastError());
    return VF_OK;
}

// The resolve of a supersampled handle's samples into its frame (vf_resolve.h).  Defined with the other supersampling calls below: the template is
// instantiated there, behind the tile kernels and what they call, whose code -- PC-relative call offsets included -- keeps its place
static void resolve_launch(const vf_terrain *t, hipStream_t s, uint32_t *dst);

// The FrameParams of the overlay pass of a supersampled handle: the caller's camera on a frame of the output size (sizes and widths in
// pixels mean output pixels).  The overlay kernels read the camera, the grid and hw, hh, W, H of it; the tile and shard fields follow.
static FrameParams output_params(const vf_terrain *t, const FrameParams &P)
{
    FrameParams Q = P;
    Q.hw = 0.5f * (float)t->oW; Q.hh = 0.5f * (float)t->oH;
    Q.W = t->oW; Q.H = t->oH; Q.ntx = (t->oW + kTileW - 1) / kTileW; Q.nty = (t->oH + kTileH - 1) / kTileH;
    Q.local_rows = t->oH;
    return Q;
}

// diag: a visibility / diagnostics frame (render_visibility): stores its visibility, composites no overlays and runs no pass of
// kFramePassTable: the frame as the tile kernel shades it.  A frame of a handle with an occluding overlay layer or with such a pass
// stores its visibility too, for that pass.
static int draw_frame(vf_terrain *t, hipStream_t s, const FramePlan &K, bool diag)
{
    const FrameParams &P = K.P;
    const bool passes = !diag && std::any_of(std::begin(kFramePassTable), std::end(kFramePassTable), [t](const FramePass &R) { return R.on(t); });
    const bool write_vis = diag || (t->ov.occluding && t->ov.nprims) || passes;
    vf_terrain::PlanState &S = t->ps[K.set];
    const uint32_t ntiles = K.ntiles, set = K.set;
    uint32_t *const rc_lo = K.rc_lo, *const rc_hi = K.rc_hi, *const seg_count = K.seg_count;
    vf_terrain::FrameEvents &ev = t->ev[t->timed_frames % (uint32_t)vf_terrain::kTimingRing];
    const bool timing_now = t->timing && K.sampled;
    const SetupView V = { S.vtx, t->d_hblk, S.recs, S.gen };
    // what the terrain passes draw into: the samples of a supersampled handle, else the frame itself (as a diagnostics frame's scratch buffer is)
    const bool resolve = t->ss > 1u && !diag;
    uint32_t *const raster = resolve ? t->d_samples : t->d_rgba;
    // ---- draw, on the caller's stream: everything that touches the output buffers ----
    uint32_t *stats = t->timing && t->stats_on ? t->d_stats : nullptr;
    const uint32_t nstats = (uint32_t)stats_layout(t).words;     // zeroed by k_clear (no memset dispatch)
    VF_HIP_TRY(hipStreamWaitEvent(s, S.planned, 0));
    VF_HIP_TRY(hipStreamWaitEvent(s, S.set_up, 0));
    if (K.lists) VF_HIP_TRY(hipStreamWaitEvent(s, S.listed, 0));
    const TileLists TL = { K.lists ? S.tl_ent : nullptr, K.lists ? S.tl_hdr : nullptr };
    // The previous frame may have been drawn on another stream of the caller's: this frame waits for it (same output / statistics
    // buffers; and when it went to another output buffer, letting the two tile kernels overlap costs more than it gains --
    // tools/exp_overlap.py; d_vis is one buffer per handle anyway).
    if (t->last_stream && t->last_stream != s && t->rendered)
        VF_HIP_TRY(hipStreamWaitEvent(s, t->ps[t->last_set].drawn, 0));
    if (timing_now) VF_HIP_TRY(hipEventRecord(ev.begin, s));
    // line groups in the raster's line loop (vf_kernels.h, raster_fast): whole frames and shards of few ranks -- wide items, triangles
    // with many lines -- gain from them (C4: one GPU -2 %, top-down camera -7 %); a rank of many mostly draws narrow strips, whose
    // triangles have a handful of lines, and is better off with the leaner kernel.  That is the variant by default; the handle
    // measures (LineLoop), and starts again when the layout is new or the camera starts to move.
    const int guess = t->nranks < (uint32_t)VF_GROUPS_MAX_RANKS ? 1 : 0;
    // (the probe's reset is about geometry -- a new layout, a camera that starts to move, other heights (set_height_common) -- never about the light)
    const LoopPick pick = t->loop.choose(guess, t->cursor.frames_since_reset <= 1 || K.motion_starts, ntiles != 0u);
    const bool groups = pick.variant != 0;
    LineLoop::Probe *gp = pick.probe ? t->loop.arm(s) : nullptr;
    if (ntiles) {
        uint32_t *vis = write_vis ? t->d_vis : nullptr;
        hipLaunchKernelGGL(k_clear, dim3(ntiles), dim3(256), 0, s, P, S.background, raster, vis, stats, nstats, seg_count);
        // one persistent workgroup per CU (a 1024-thread workgroup with 70 KB of LDS fills one), the fast variant, works through
        // the items; then a handful of persistent workgroups of the complete variant take the items that met a clipped or
        // oversized primitive (normally none)
        const dim3 per_cu(std::min<uint32_t>((uint32_t)std::max(1, t->ctx->prop.multiProcessorCount) * (1024u / (uint32_t)kTileThreads), ntiles + kSplitBudget)),
                   few(std::min<uint32_t>(64u, ntiles + kSplitBudget)), threads(kTileThreads);
#define VF_TILE_ARGS P, V, S.row_ranges, S.cap_seg, S.cap_rad, t->d_lut, t->ctx->d_thresh, S.work_sorted, S.work_count, \
                     rc_lo, rc_hi, raster, vis, stats, S.feedback, S.redo, S.band, TL
        const bool fast = fast_shading(t->inputs);
        // (the complete variant redraws the rare items that met a clipped primitive: always the plain loop)
#define VF_TILE_LAUNCH(WV, FS)                                                                                         \
        do {                                                                                                           \
            if (groups) hipLaunchKernelGGL((k_tile<WV, false, FS, true>), per_cu, threads, 0, s, VF_TILE_ARGS);        \
            else hipLaunchKernelGGL((k_tile<WV, false, FS, false>), per_cu, threads, 0, s, VF_TILE_ARGS);              \
            hipLaunchKernelGGL((k_tile<WV, true, FS, false>), few, threads, 0, s, VF_TILE_ARGS);                       \
        } while (0)
        if (write_vis && fast) VF_TILE_LAUNCH(true, true);
        else if (write_vis) VF_TILE_LAUNCH(true, false);
        else if (fast) VF_TILE_LAUNCH(false, true);
        else VF_TILE_LAUNCH(false, false);
#undef VF_TILE_LAUNCH
#undef VF_TILE_ARGS
        if (gp) t->loop.close(gp, s);
    }
    else VF_HIP_TRY(hipMemsetAsync(seg_count, 0, sizeof(uint32_t), s));   // (a shard without tiles: what k_clear does on its way in)
    if (timing_now) { VF_HIP_TRY(hipEventRecord(ev.end, s)); t->timed_frames++; }
    if (passes && ntiles)                                  // behind the tile kernels, under the resolve and the overlays
        for (const FramePass &R : kFramePassTable) {
            if (int rc = R.on(t) ? R.run(t, s, P, V, S.work_count + 3, raster) : VF_OK) return rc;
        }
    if (resolve) {                                        // the samples -> the frame: every output pixel is rewritten, whatever the tiles drew
        resolve_launch(t, s, t->d_rgba);
        VF_HIP_TRY(hipGetLastError());
    }
    if (t->ov.nprims && !diag) {                           // (visibility / diagnostics frames: none)
        const int orc = resolve ? overlay_pass(t, s, output_params(t, P), V) : overlay_pass(t, s, P, V);
        if (orc != VF_OK) return orc;
    }
    VF_HIP_TRY(hipEventRecord(S.drawn, s));
    VF_HIP_TRY(hipGetLastError());
    std::memcpy(S.u_used, t->inputs.u, sizeof S.u_used);           // the camera this set's tile times (being measured now) belong to
    S.have_u_used = true;
    t->last_stream = s;
    t->last_set = set;
    t->rendered = true;
    return VF_OK;
}

// The first half of the NEXT frame, queued ahead of its call (vf_terrain::pre).
static void plan_ahead(vf_terrain *t, hipStream_t s)
{
    vf_terrain::PrePlan &R = t->pre;
    R.before = t->cursor;
    if (plan_frame(t, s, R.K, false, true) == VF_OK) { R.valid = true; R.gen = t->inputs_gen; R.geom = t->geom_gen; }
    else {                                                  // (a failed launch: the next call plans for itself and reports it)
        // (the whole cursor goes back, though only cur_set, frame_no and frames_since_reset can have moved: a plan is made ahead for a
        //  camera at rest only -- neither moving nor was_moving, a frame drawn, u_drawn equal to the live uniforms -- and plan_frame
        //  leaves the other four fields of such a cursor as they were)
        t->cursor = R.before;
        (void)hipGetLastError();
    }
}

// A read-back has queued its copy on `s`: the plan a waiting caller's next frame will want goes out now, behind the copy (the caller
// waits for the copy's event, not for the stream), if the frame was drawn from geometry inputs that still stand (SAME GEOMETRY: a plan
// made ahead survives a change of the shading inputs, render_impl).
static void flush_preplan(vf_terrain *t, hipStream_t s)
{
    if (!t->preplan_pending) return;
    t->preplan_pending = false;
    if (t->pre.valid || t->side || t->last_drawn_geom != t->geom_gen || t->bounds_dirty || s != t->last_stream) return;
    plan_ahead(t, s);
}

// ... and the wait that goes with it: for the copy's event when a plan was queued behind it, for the stream otherwise
static hipError_t finish_readback(vf_terrain *t, hipStream_t s)
{
    if (!t->preplan_pending && !t->tl_job.pending) return hipStreamSynchronize(s);
    hipError_t e = t->copied ? hipSuccess : hipEventCreateWithFlags(&t->copied, hipEventDisableTiming);
    if (e != hipSuccess) { t->preplan_pending = false; t->tl_job.pending = false; return hipStreamSynchronize(s); }
    e = hipEventRecord(t->copied, s);
    if (e != hipSuccess) return e;
    flush_tile_lists(t, s);
    flush_preplan(t, s);
    return hipEventSynchronize(t->copied);
}

static int render_impl(vf_terrain *t, hipStream_t s, bool write_vis)
{
    FramePlan K;
    bool planned = false;
    // Was the GPU done with the previous frame when this call came in?  Then the caller waits between frames (render_png, render_rgba,
    // anything that reads a frame back) and the next frame's plan is worth queuing ahead; a caller that streams frames brings the next
    // plan itself, at the same moment, and a plan queued ahead would only be one more after the last frame.
    const bool idle_at_entry = t->rendered && hipEventQuery(t->ps[t->last_set].drawn) == hipSuccess;
    (void)hipGetLastError();                                // ("not ready" is not an error)
    const bool streaming = t->rendered && !idle_at_entry;
    t->preplan_pending = false;                             // (no read-back came in between: this call plans for itself)
    if (t->pre.valid) {
        t->pre.valid = false;
        // SAME GEOMETRY, not "same picture": the plan holds for the geometry generation and the feedback it read (whoever changes the
        // feedback or the layout drops it: vf_terrain_debug_set_plan_feedback, the shard setters).  When only shading inputs moved --
        // sun, exposure, height range, shade mode, precision -- the plan stays and K.P is made again from the live inputs: its geometry
        // fields come out bit for bit as the plan's kernels saw them, its shading fields are the new ones.  What the plan chose (set,
        // mode, ranges, sampling) is not in K.P.
        if (t->pre.geom == t->geom_gen && !write_vis) {
            K = t->pre.K; planned = true;
            if (t->pre.gen != t->inputs_gen) build_params(t, t->inputs, K.P);
            if (!t->side) {                                 // a waiting caller's plan, queued behind its last read-back: done by now?
                const bool ready = hipEventQuery(t->ps[K.set].planned) == hipSuccess;
                (void)hipGetLastError();
                t->tight_calls = ready ? 0u : t->tight_calls + 1u;
                if (t->tight_calls >= 3u) t->want_plan_streams = true;
            }
        }
        else { t->pre.valid = true; VF_HIP_TRY(drop_preplan(t, s)); }     // made for other geometry
    }
    if (!planned) { const int rc = plan_frame(t, s, K, streaming); if (rc != VF_OK) return rc; }
    const bool again = t->last_drawn_geom == t->geom_gen;       // SAME GEOMETRY: the frame before this one was drawn from the same geometry inputs (its light may differ)
    const int rc = draw_frame(t, s, K, write_vis);
    if (rc != VF_OK) return rc;
    t->last_plan_mode = K.mode | (planned ? VF_PLAN_QUEUED_AHEAD : 0u);
    t->last_drawn_geom = t->geom_gen;
    // a caller that waits for its frames: the lists of the state drawn before this one go out now, behind this frame's kernels (on the
    // set-up stream when there is one), if no read-back took them; those of this frame's state wait for the next read-back's copy
    // (finish_readback) or the next frame
    flush_tile_lists(t, t->side ? t->side2 : s);
    if (!write_vis && (K.mode & VF_PLAN_GEOMETRY_REUSED) && !K.lists && !t->tl_off && !t->tl_failed && K.ntiles && !lists_valid(t, t->ps[K.set])) {
        t->tl_job.pending = true; t->tl_job.set = K.set; t->tl_job.geom = t->ps[K.set].geom_stamp; t->tl_job.P = K.P;
    }
    // the camera is at rest (two frames from one set of geometry inputs), the handle is past its first frames, nothing diagnostic is going on:
    // the next frame's plan goes out now
    // (round 6: also for a caller that streams frames of a resting camera -- its next plan goes out one call early, which changes nothing while
    //  the frames keep coming and has the plan ready for the first frame after it has waited once)
    if (again && (idle_at_entry || t->side) && !write_vis && !t->bounds_dirty && !t->cursor.camera_moving && !t->cursor.was_moving && t->cursor.frames_since_reset > vf_terrain::kPlanStates && !(t->timing && t->stats_on)) {
        if (t->side) plan_ahead(t, s);                      // on the plan streams, under this frame's tile kernel
        else t->preplan_pending = true;                     // no plan streams (a waiting caller): behind the next read-back's copy, flush_preplan
    }
    return VF_OK;
}

// a frame for the caller: the inputs it is drawn from are what the diagnostics render again (render_visibility)
static int render_recorded(vf_terrain *t, hipStream_t s)
{
    t->drawn_inputs = t->inputs;
    t->have_frame = true;
    return render_impl(t, s, false);
}

int vf_terrain_render(vf_terrain *t, void *stream)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->have_uniforms) return fail(VF_ERR_INVALID, "uniforms not set");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    return render_recorded(t, stream ? (hipStream_t)stream : t->ctx->stream);
}

int vf_terrain_render_batch(vf_terrain *t, const float *uniforms, uint32_t n, void *const *dev_rgba, void *stream)
{
    if (!t || (!uniforms && n)) return fail(VF_ERR_INVALID, "NULL argument");
    if (const char *why = pass_refusal(t, true)) return fail(VF_ERR_INVALID, why);
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : t->ctx->stream;
    for (uint32_t k = 0; k < n; ++k) {
        if (dev_rgba && !dev_rgba[k]) return fail(VF_ERR_INVALID, "dev_rgba holds a NULL output buffer");
        take_uniforms(t, uniforms + 44u * k);
        if (dev_rgba) t->d_rgba = (uint32_t *)dev_rgba[k];
        const int rc = render_recorded(t, s);
        if (rc != VF_OK) return rc;
    }
    return VF_OK;
}

int vf_terrain_render_batch_host(vf_terrain *t, const float *uniforms, uint32_t n, uint8_t *const *host_rgba)
{
    if (!t || !uniforms || !host_rgba) return fail(VF_ERR_INVALID, "NULL argument");
    if (t->shard_tiles || t->local_rows != t->H) return fail(VF_ERR_INVALID, "batch read-back needs the whole frame on one handle (pose-parallel ranks are replicas)");
    if (const char *why = pass_refusal(t, true)) return fail(VF_ERR_INVALID, why);
    for (uint32_t k = 0; k < n; ++k) if (!host_rgba[k]) return fail(VF_ERR_INVALID, "host_rgba holds a NULL destination");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    constexpr uint32_t R = vf_terrain::kBatchRing;
    const size_t frame_bytes = (size_t)t->W * t->H * 4, slot_bytes = (size_t)t->ntx * t->nty * kTileW * kTileH * 4;
    VF_HIP_TRY(ctx_copy_stream(t->ctx, &t->copy_stream));
    for (uint32_t r = 0; r < R && r < n; ++r) {
        if (!t->d_batch[r]) VF_HIP_TRY(hipMalloc(&t->d_batch[r], slot_bytes));
        if (!t->batch_drawn[r]) VF_HIP_TRY(hipEventCreateWithFlags(&t->batch_drawn[r], hipEventDisableTiming));
        if (!t->batch_copied[r]) VF_HIP_TRY(hipEventCreateWithFlags(&t->batch_copied[r], hipEventDisableTiming));
    }
    hipStream_t s = t->ctx->stream;
    uint32_t *const out_before = t->d_rgba;
    int rc = VF_OK;
    hipError_t err = hipSuccess;
    for (uint32_t k = 0; k < n && rc == VF_OK && err == hipSuccess; ++k) {
        const uint32_t r = k % R;
        if (k >= R) err = hipStreamWaitEvent(s, t->batch_copied[r], 0);       // pose k - R has left the slot
        if (err != hipSuccess) break;
        rc = vf_terrain_render_batch(t, uniforms + 44u * k, 1, (void *const *)&t->d_batch[r], s);
        if (rc != VF_OK) break;
        err = hipEventRecord(t->batch_drawn[r], s);
        if (err == hipSuccess) err = hipStreamWaitEvent(t->copy_stream, t->batch_drawn[r], 0);
        // (a pinned destination -- vf_host_alloc -- makes this one asynchronous DMA under the next pose's kernels; a pageable one is
        //  staged by the runtime and holds the host until it is done: correct, slower)
        if (err == hipSuccess) err = hipMemcpyAsync(host_rgba[k], t->d_batch[r], frame_bytes, hipMemcpyDeviceToHost, t->copy_stream);
        if (err == hipSuccess) err = hipEventRecord(t->batch_copied[r], t->copy_stream);
    }
    const hipError_t e2 = hipStreamSynchronize(t->copy_stream);
    const hipError_t e3 = hipStreamSynchronize(s);
    t->d_rgba = out_before;
    t->rendered = false;                                    // the handle's own output buffer does not hold the last pose: read-backs must render first
    if (rc != VF_OK) return rc;
    if (err != hipSuccess) return fail(VF_ERR_HIP, std::string("batch read-back: ") + hipGetErrorString(err));
    if (e2 != hipSuccess || e3 != hipSuccess) return fail(VF_ERR_HIP, std::string("batch read-back: ") + hipGetErrorString(e2 != hipSuccess ? e2 : e3));
    return VF_OK;
}

// The handle's visibility buffer, one id per pixel of its whole tiles: made by the first caller that needs a stored visibility (a
// visibility or diagnostics frame, an occluding overlay layer, shadows)
static int ensure_vis(vf_terrain *t)
{
    const size_t npx = (size_t)t->ntx * t->nty * kTileW * kTileH;
    if (!t->d_vis) VF_HIP_TRY(hipMalloc(&t->d_vis, npx * sizeof(uint32_t)));
    return VF_OK;
}

// Re-render the frame vf_terrain_render drew last with the visibility store enabled, into scratch buffers: uniforms set since,
// the output buffer (also a caller's, vf_terrain_set_output_device), the stream later calls synchronise with, the timing ring
// and the camera-motion state are as before afterwards.  What the extra frame does leave behind: it uses one of the two plan
// states and adds its tile times to that state's scheduling feedback -- the same view as the frame before it, so the feedback
// stays valid -- and the next frame plans with the other state.
static int render_visibility(vf_terrain *t)
{
    const size_t npx = (size_t)t->ntx * t->nty * kTileW * kTileH;
    if (int rc = ensure_vis(t)) return rc;
    if (!t->d_rgba_scratch) VF_HIP_TRY(hipMalloc(&t->d_rgba_scratch, npx * sizeof(uint32_t)));
    int rc = vf_terrain_sync(t);
    if (rc != VF_OK) return rc;
    VF_HIP_TRY(sync_sides(t));
    const FrameInputs inputs_now = t->inputs;
    PlanCursor cursor_now = t->cursor;
    uint32_t *const out_now = t->d_rgba;
    const hipStream_t stream_now = t->last_stream;
    const bool timing = t->timing, rendered = t->rendered;
    const uint32_t plan_mode_now = t->last_plan_mode;
    // uniforms set since the frame was drawn may describe other geometry: the diagnostic frame then gets a geometry generation of its own,
    // and so does the live block when it comes back -- the plan state the frame filled is not taken for the live inputs' (nor the other way)
    const bool other_geometry = t->have_frame && !same_geometry(t->drawn_inputs.u, t->inputs.u);
    if (t->have_frame) t->inputs = t->drawn_inputs;
    if (other_geometry) t->geom_gen++;
    t->d_rgba = t->d_rgba_scratch; t->timing = false;
    rc = render_impl(t, t->ctx->stream, true);
    hipError_t e = hipStreamSynchronize(t->ctx->stream);
    t->inputs = inputs_now;
    if (other_geometry) t->geom_gen++;
    cursor_now.cur_set = t->cursor.cur_set; cursor_now.frame_no = t->cursor.frame_no;      // (the plan state and the frame number it used stay used, see above)
    t->cursor = cursor_now;
    t->d_rgba = out_now; t->last_stream = stream_now; t->timing = timing;
    t->rendered = rendered;                                 // the diagnostic frame went to scratch buffers: the caller's output is as it was
    t->last_plan_mode = plan_mode_now;
    if (rc != VF_OK) return rc;
    if (e != hipSuccess) return fail(VF_ERR_HIP, std::string("visibility render: ") + hipGetErrorString(e));
    return VF_OK;
}

int vf_terrain_sync(vf_terrain *t)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    VF_HIP_TRY(wait_frame(t));
    return VF_OK;
}

// ---- overlays (vf_overlay.h) ---------------------------------------------------------------------

static float ov_clamp_px(float v) { return std::fmin(std::fmax(v, 1.0f), 64.0f); }

static uint32_t pack_rgba8(const uint8_t c[4]) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24); }

static int ov_usable(const vf_terrain *t)
{
    if (t->shard_tiles || t->nranks != 1) return fail(VF_ERR_INVALID, "overlays need a whole-frame handle: sharded compositing is not supported");
    return VF_OK;
}

// the primitive budget of a handle (all layers): `more` records on top of `have` (checked as records are built, and by ov_append)
static int ov_budget(uint64_t have, uint64_t more)
{
    if (have + more > kOvMaxPrims)
        return fail(VF_ERR_INVALID, "overlays: more than 2^24 primitives on one handle (a point is one, a polyline of m vertices up to 2m, "
                                    "a polygon fill 1 + 2 per ring edge)");
    return VF_OK;
}

// One layer, appended as a whole: its `nadd` records (feature order), which `produce` writes to the device array it is handed (the
// layer's first record) -- an upload of records built on the host, or a kernel that makes them where they are; for a polygon layer with
// fills the header record index of each fill feature (`hdr`) and the number of fill records at the start of the layer; the handle's
// feature count after the layer; `occlude`: the layer's records are made with kOvOcclude set (vf_terrain_set_layer_occlusion's state
// is brought about here).  The first layer makes the overlay state.  Nothing is committed before every allocation and the producer
// have succeeded: a failure leaves the layers as they were.
using OvProducer = std::function<int(OvIn *dst)>;
// (the set-up records and the visibility of a supersampled frame are the samples'; the composite's depth test reads them at the pixel centre)
static const char *const kSsNoOcclusion = "the handle is supersampled: occluding overlay layers are not supported (their depth test reads the frame's visibility per output pixel)";
static int ov_append(vf_terrain *t, size_t nadd, const OvProducer &produce, const std::vector<uint32_t> &hdr, uint32_t nfillrec, bool polygon,
                     uint32_t features, uint32_t *layer_id, bool occlude = false)
{
    vf_terrain::Overlays &O = t->ov;
    if (int rc = ov_budget(O.nprims, nadd)) return rc;
    if (occlude && t->ss > 1u) return fail(VF_ERR_INVALID, kSsNoOcclusion);
    VF_HIP_TRY(wait_frame(t));                                // (a frame in flight reads the arrays)
    if (occlude) { if (int rc = ensure_vis(t)) return rc; }
    if (!O.d_cnt) {
        const uint32_t nbins = ((t->oW + kOvBin - 1u) / kOvBin) * ((t->oH + kOvBin - 1u) / kOvBin);
        hipError_t e = hipMalloc(&O.d_cnt, (size_t)nbins * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemset(O.d_cnt, 0, (size_t)nbins * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&O.d_start, ((size_t)nbins + 1u) * sizeof(uint32_t));
        if (e == hipSuccess) e = hipHostMalloc((void **)&O.h_total, 4 * sizeof(uint32_t), hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&O.counted, hipEventDisableTiming);
        if (e != hipSuccess) { ov_release(t); return fail(VF_ERR_NOMEM, std::string("overlay allocation failed: ") + hipGetErrorString(e)); }
    }
    // Growth: each array of a group to the group's new capacity.  When a group only partly grows, the arrays that did are larger than
    // they need to be; no counter has moved, so that is harmless.  dep (per-frame values, made again by the next k_ov_setup) is made
    // when a layer is first set to occlude -- by this growth instead if the handle had no room for records then -- and grows with the
    // primitives from then on.
    const uint32_t need = O.nprims + (uint32_t)nadd, nfill = O.nfill + (uint32_t)hdr.size();
    const size_t cap = std::min<size_t>(kOvMaxPrims, std::max<size_t>({ need, 2u * O.in.cap, 1024u }));
    hipError_t e = O.in.reserve(need, cap, O.nprims);
    if (e == hipSuccess) e = O.prim.reserve(need, cap);
    if (e == hipSuccess) e = O.box.reserve(need, cap);
    if (e == hipSuccess && (O.dep.p || O.occluding || occlude)) e = O.dep.reserve(need, cap, 0, true);
    if (e == hipSuccess && (O.hzrec.p || O.hazed)) e = O.hzrec.reserve(need, cap);      // (per-frame values: k_ov_haze_setup writes every record)
    if (e != hipSuccess) return fail(VF_ERR_NOMEM, std::string("overlay allocation failed: ") + hipGetErrorString(e));
    if (!hdr.empty()) {
        const size_t fill_cap = std::max<size_t>({ nfill, 2u * O.pg_hdr.cap, 256u });
        e = O.pg_total.reserve(1, 1, 0, true);
        if (e == hipSuccess) e = O.pg_hdr.reserve(nfill, fill_cap, O.nfill);
        if (e == hipSuccess) e = O.pg_fbox.reserve(nfill, fill_cap, 0, true);
        if (e == hipSuccess) e = O.pg_fbin.reserve(nfill, fill_cap);
        if (e != hipSuccess) return fail(VF_ERR_NOMEM, std::string("polygon overlay allocation failed: ") + hipGetErrorString(e));
        VF_HIP_TRY(hipMemcpy(O.pg_hdr.p + O.nfill, hdr.data(), hdr.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (nadd)
        if (int rc = produce(O.in.p + O.nprims)) return rc;
    if (!hdr.empty()) {
        if (!O.nfill) O.pg_lo = O.nprims;
        O.pg_hi = O.nprims + nfillrec;
        O.nfill = nfill;
    }
    if (layer_id) *layer_id = (uint32_t)O.layer.size();
    O.layer.push_back({ O.nprims, need, polygon, occlude });
    if (occlude) O.occluding++;
    O.nprims = need;
    O.features = features;
    return VF_OK;
}

// ... of records built on the host
static int ov_append(vf_terrain *t, const std::vector<OvIn> &add, const std::vector<uint32_t> &hdr, uint32_t nfillrec, bool polygon,
                     uint32_t features, uint32_t *layer_id)
{
    return ov_append(t, add.size(), [&](OvIn *dst) -> int {
        VF_HIP_TRY(hipMemcpy(dst, add.data(), add.size() * sizeof(OvIn), hipMemcpyHostToDevice));
        return VF_OK;
    }, hdr, nfillrec, polygon, features, layer_id);
}

int vf_terrain_add_points(vf_terrain *t, const float *xyz, uint32_t n, const float *size_px, const uint8_t *rgba, float default_size,
                          const uint8_t default_rgba[4], int shape, int drape, uint32_t *layer_id)
{
    if (!t || (!xyz && n) || (!rgba && !default_rgba)) return fail(VF_ERR_INVALID, "NULL argument");
    if (shape != VF_SHAPE_CIRCLE && shape != VF_SHAPE_SQUARE) return fail(VF_ERR_INVALID, "shape must be VF_SHAPE_CIRCLE or VF_SHAPE_SQUARE");
    if (int rc = ov_usable(t)) return rc;
    if (!size_px && !std::isfinite(default_size)) return fail(VF_ERR_INVALID, "size_px must be finite");
    std::vector<OvIn> add;
    add.reserve(n);
    uint32_t feature = t->ov.features;
    for (uint32_t k = 0; k < n; ++k) {
        const float *p = xyz + 3u * k;
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;     // (dropped, ROADMAP V4.1)
        const float sz = size_px ? size_px[k] : default_size;
        if (!std::isfinite(sz)) return fail(VF_ERR_INVALID, "size_px must be finite");
        OvIn q{};
        for (int c = 0; c < 3; ++c) { q.p0[c] = p[c]; q.p1[c] = p[c]; }
        q.size = ov_clamp_px(sz) * 0.5f;
        q.flags = (shape == VF_SHAPE_SQUARE ? kOvSquare : kOvCircle) | (drape ? kOvDrape : 0u);
        q.rgba = pack_rgba8(rgba ? rgba + 4u * k : default_rgba);
        q.feature = feature++;
        add.push_back(q);
    }
    return ov_append(t, add, {}, 0, false, feature, layer_id);
}

// the primitives of one polyline (vertices v0 .. v1 - 1 of xyz; a closed ring ends at its first vertex again): butt segments, discs at
// interior vertices (round joins) and, for round caps, at both ends; square caps extend the path's first / last segment
static void ov_path(const float *xyz, uint32_t v0, uint32_t v1, bool closed, float hw, uint32_t rgba, int cap, uint32_t base, uint32_t feature,
                    std::vector<OvIn> &add)
{
    const uint32_t n = v1 - v0, m = n + (closed ? 1u : 0u);
    auto at = [&](uint32_t v) { return xyz + 3u * (v0 + (v < n ? v : 0u)); };
    for (uint32_t v = 0; v < m; ++v) {
        const bool end = v == 0 || v + 1u == m;
        if (!end || cap == VF_CAP_ROUND) {                    // disc: round join / round cap
            OvIn q{};
            for (int c = 0; c < 3; ++c) { q.p0[c] = at(v)[c]; q.p1[c] = q.p0[c]; }
            q.size = hw; q.flags = kOvCircle | base; q.rgba = rgba; q.feature = feature;
            add.push_back(q);
        }
        if (v + 1u < m) {                                     // butt segment v -> v + 1 (square caps extend the path's first / last one)
            OvIn q{};
            for (int c = 0; c < 3; ++c) { q.p0[c] = at(v)[c]; q.p1[c] = at(v + 1u)[c]; }
            q.size = hw; q.rgba = rgba; q.feature = feature;
            q.flags = kOvSegment | base | (cap == VF_CAP_SQUARE && v == 0 ? kOvExt0 : 0u) | (cap == VF_CAP_SQUARE && v + 2u == m ? kOvExt1 : 0u);
            add.push_back(q);
        }
    }
}

int vf_terrain_add_lines(vf_terrain *t, const float *xyz, const uint32_t *path_offsets, uint32_t npaths, float width_px,
                         const uint8_t rgba[4], int cap, int drape, uint32_t *layer_id)
{
    if (!t || !path_offsets || !rgba) return fail(VF_ERR_INVALID, "NULL argument");
    if (cap != VF_CAP_BUTT && cap != VF_CAP_SQUARE && cap != VF_CAP_ROUND) return fail(VF_ERR_INVALID, "cap must be VF_CAP_BUTT, VF_CAP_SQUARE or VF_CAP_ROUND");
    if (!std::isfinite(width_px)) return fail(VF_ERR_INVALID, "width_px must be finite");
    if (int rc = ov_usable(t)) return rc;
    if (npaths && !xyz) return fail(VF_ERR_INVALID, "NULL argument");
    std::vector<OvIn> add;
    uint32_t feature = t->ov.features;
    const float hw = ov_clamp_px(width_px) * 0.5f;
    const uint32_t base = (drape ? kOvDrape : 0u);
    for (uint32_t p = 0; p < npaths; ++p) {
        const uint32_t v0 = path_offsets[p], v1 = path_offsets[p + 1];
        if (v1 < v0 || v1 - v0 < 2u) return fail(VF_ERR_INVALID, "every path needs at least 2 vertices (path_offsets ascending)");
        for (uint32_t v = v0; v < v1; ++v)
            for (int c = 0; c < 3; ++c)
                if (!std::isfinite(xyz[3u * v + c])) return fail(VF_ERR_INVALID, "a line vertex is not finite");
        if (int rc = ov_budget(t->ov.nprims + add.size(), 2ull * (v1 - v0))) return rc;
        ov_path(xyz, v0, v1, false, hw, pack_rgba8(rgba), cap, base, feature++, add);
    }
    return ov_append(t, add, {}, 0, false, feature, layer_id);
}

int vf_terrain_add_polygons(vf_terrain *t, const float *xyz, const uint32_t *ring_offsets, uint32_t nrings, const uint32_t *feature_offsets,
                            uint32_t nfeatures, const uint8_t *fill_rgba, const uint8_t default_fill[4], const uint8_t line_rgba[4],
                            float line_width_px, int drape, uint32_t *layer_id)
{
    if (!t || !ring_offsets || !feature_offsets) return fail(VF_ERR_INVALID, "NULL argument");
    if (!fill_rgba && !default_fill && !line_rgba) return fail(VF_ERR_INVALID, "a polygon layer needs a fill colour, an outline colour or both");
    if (line_rgba && !std::isfinite(line_width_px)) return fail(VF_ERR_INVALID, "line_width_px must be finite");
    if (int rc = ov_usable(t)) return rc;
    if (nrings && !xyz) return fail(VF_ERR_INVALID, "NULL argument");
    const bool fill = fill_rgba || default_fill;
    for (uint32_t f = 0; f < nfeatures; ++f) {
        const uint32_t r0 = feature_offsets[f], r1 = feature_offsets[f + 1];
        if (r1 <= r0 || r1 > nrings) return fail(VF_ERR_INVALID, "every polygon needs at least 1 ring (feature_offsets ascending, <= nrings)");
        for (uint32_t r = r0; r < r1; ++r) {
            const uint32_t v0 = ring_offsets[r], v1 = ring_offsets[r + 1];
            if (v1 < v0 || v1 - v0 < 3u) return fail(VF_ERR_INVALID, "every ring needs at least 3 vertices (ring_offsets ascending)");
            for (uint32_t v = v0; v < v1; ++v)
                for (int c = 0; c < 3; ++c)
                    if (!std::isfinite(xyz[3u * v + c])) return fail(VF_ERR_INVALID, "a polygon vertex is not finite");
        }
    }
    const vf_terrain::Overlays &O = t->ov;
    std::vector<OvIn> add;
    std::vector<uint32_t> hdr;
    uint32_t feature = O.features;
    const uint32_t base = drape ? kOvDrape : 0u;
    if (fill)                                                 // fills: a header, then the two slots of every ring edge, in ring order
        for (uint32_t f = 0; f < nfeatures; ++f) {
            const uint32_t k = O.nfill + (uint32_t)hdr.size();
            float kbits;
            std::memcpy(&kbits, &k, sizeof kbits);
            uint64_t n = 1;
            for (uint32_t r = feature_offsets[f]; r < feature_offsets[f + 1]; ++r) n += 2ull * (ring_offsets[r + 1] - ring_offsets[r]);
            if (int rc = ov_budget(O.nprims + add.size(), n)) return rc;
            hdr.push_back(O.nprims + (uint32_t)add.size());
            OvIn h{};
            h.size = kbits; h.flags = kOvPoly | kPgHeader; h.rgba = pack_rgba8(fill_rgba ? fill_rgba + 4u * f : default_fill); h.feature = feature;
            add.push_back(h);
            for (uint32_t r = feature_offsets[f]; r < feature_offsets[f + 1]; ++r) {
                const uint32_t v0 = ring_offsets[r], nv = ring_offsets[r + 1] - v0, first = O.nprims + (uint32_t)add.size();
                for (uint32_t e = 0; e < nv; ++e)
                    for (uint32_t slot = 0; slot < 2u; ++slot) {
                        OvIn q{};
                        for (int c = 0; c < 3; ++c) { q.p0[c] = xyz[3u * (v0 + e) + c]; q.p1[c] = xyz[3u * (v0 + (e + 1u) % nv) + c]; }
                        q.size = kbits; q.flags = kOvPoly | base | (slot ? kPgClose : 0u); q.feature = feature;
                        q.pad[0] = first; q.pad[1] = nv;
                        add.push_back(q);
                    }
            }
            feature++;
        }
    const uint32_t nfillrec = (uint32_t)add.size();
    if (line_rgba) {                                          // outlines: add_lines of each ring closed back to its first vertex, round caps
        const float hw = ov_clamp_px(line_width_px) * 0.5f;
        for (uint32_t f = 0; f < nfeatures; ++f)
            for (uint32_t r = feature_offsets[f]; r < feature_offsets[f + 1]; ++r) {
                const uint32_t v0 = ring_offsets[r], v1 = ring_offsets[r + 1];
                if (int rc = ov_budget(O.nprims + add.size(), 2ull * (v1 - v0) + 1u)) return rc;
                ov_path(xyz, v0, v1, true, hw, pack_rgba8(line_rgba), VF_CAP_ROUND, base, feature++, add);
            }
    }
    return ov_append(t, add, hdr, nfillrec, true, feature, layer_id);
}

int vf_terrain_set_layer_occlusion(vf_terrain *t, uint32_t layer_id, int occlude, float depth_bias)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (int rc = ov_usable(t)) return rc;
    if (!std::isfinite(depth_bias) || depth_bias < 0.0f) return fail(VF_ERR_INVALID, "depth_bias must be a finite number >= 0");
    vf_terrain::Overlays &O = t->ov;
    if (layer_id >= O.layer.size()) return fail(VF_ERR_INVALID, "no overlay layer with that id");
    vf_terrain::Overlays::Layer &L = O.layer[layer_id];
    if (L.polygon) return fail(VF_ERR_INVALID, "a polygon layer cannot occlude: polygon fills have no depth");
    if (occlude && t->ss > 1u) return fail(VF_ERR_INVALID, kSsNoOcclusion);
    VF_HIP_TRY(wait_frame(t));                                // (a frame in flight reads the records)
    if (occlude) {
        if (int rc = ensure_vis(t)) return rc;
        VF_HIP_TRY(O.dep.reserve(O.in.cap, O.in.cap, 0, true));
    }
    const float kb = 1.0f + depth_bias;                       // the layer's depth factor, rounded once (binary32)
    uint32_t kb_bits;
    std::memcpy(&kb_bits, &kb, sizeof kb_bits);
    if (L.hi > L.lo) {
        hipLaunchKernelGGL(k_ov_occlude, dim3((L.hi - L.lo + 255u) / 256u), dim3(256), 0, t->ctx->stream, L.lo, L.hi, O.in.p,
                           occlude ? 1u : 0u, kb_bits);
        VF_HIP_TRY(hipGetLastError());
        VF_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
    }
    if (L.occlude != (occlude != 0)) O.occluding += occlude ? 1u : (uint32_t)-1;
    L.occlude = occlude != 0;
    return VF_OK;
}

// ---- contour lines (vf_contour.h) ----------------------------------------------------

// the displaced-height cache and the per-block bounds hold the handle's current heights (no frame in flight afterwards)
static int ct_heights_current(vf_terrain *t)
{
    VF_HIP_TRY(wait_frame(t));
    VF_HIP_TRY(sync_sides(t));
    if (t->bounds_dirty) {
        hipLaunchKernelGGL(k_height_blocks, dim3(t->nblocks), dim3(64), 0, t->ctx->stream, t->n, t->nb, t->tw, axis(t), t->d_height, t->d_hblk, t->d_bounds);
        VF_HIP_TRY(hipGetLastError());
        VF_HIP_TRY(hipEventRecord(t->cached, t->ctx->stream));
        t->cached_on = t->ctx->stream;
        t->bounds_dirty = false;
    }
    return VF_OK;
}

int vf_terrain_height_bounds(vf_terrain *t, float *lo, float *hi)
{
    if (!t || !lo || !hi) return fail(VF_ERR_INVALID, "NULL argument");
    if (int rc = ct_heights_current(t)) return rc;
    if (t->ct.bounds.reserve(1, 1) != hipSuccess) return fail(VF_ERR_NOMEM, "height bounds allocation failed");
    hipLaunchKernelGGL(k_ct_bounds, dim3(1), dim3(1024), 0, t->ctx->stream, t->n, t->nb, t->d_bounds, t->d_hblk, t->ct.bounds.p);
    VF_HIP_TRY(hipGetLastError());
    float2 b;
    VF_HIP_TRY(hipMemcpyAsync(&b, t->ct.bounds.p, sizeof b, hipMemcpyDeviceToHost, t->ctx->stream));
    VF_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
    *lo = b.x; *hi = b.y;
    return VF_OK;
}

int vf_terrain_layer_primitive_count(vf_terrain *t, uint32_t layer_id, uint32_t *count)
{
    if (!t || !count) return fail(VF_ERR_INVALID, "NULL argument");
    if (layer_id >= t->ov.layer.size()) return fail(VF_ERR_INVALID, "no overlay layer with that id");
    *count = t->ov.layer[layer_id].hi - t->ov.layer[layer_id].lo;
    return VF_OK;
}

int vf_terrain_add_contours(vf_terrain *t, const float *levels, uint32_t nlevels, float width_px, const uint8_t rgba[4], float lift, int join,
                            int occlude, float depth_bias, uint32_t *layer_id, uint32_t *nsegments)
{
    if (!t || !levels || !rgba) return fail(VF_ERR_INVALID, "NULL argument");
    if (join != VF_JOIN_ROUND && join != VF_JOIN_NONE) return fail(VF_ERR_INVALID, "join must be VF_JOIN_ROUND or VF_JOIN_NONE");
    if (!std::isfinite(width_px)) return fail(VF_ERR_INVALID, "width_px must be finite");
    if (!std::isfinite(lift)) return fail(VF_ERR_INVALID, "lift must be finite");
    if (occlude && (!std::isfinite(depth_bias) || depth_bias < 0.0f)) return fail(VF_ERR_INVALID, "depth_bias must be a finite number >= 0");
    if (nlevels < 1u || nlevels > kCtMaxLevels) return fail(VF_ERR_INVALID, "a contour layer needs 1 .. 65536 levels");
    for (uint32_t k = 0; k < nlevels; ++k)
        if (!std::isfinite(levels[k]) || (k && !(levels[k] > levels[k - 1])))
            return fail(VF_ERR_INVALID, "contour levels must be finite and strictly ascending");
    if (int rc = ov_usable(t)) return rc;
    if (!t->have_uniforms) return fail(VF_ERR_INVALID, "uniforms not set");     // (the grid spacing)
    if (int rc = ct_heights_current(t)) return rc;
    vf_terrain::Contours &C = t->ct;
    hipStream_t s = t->ctx->stream;
    hipError_t e = C.levels.reserve(nlevels, nlevels);
    if (e == hipSuccess) e = C.count.reserve(t->nblocks, t->nblocks);
    if (e == hipSuccess) e = C.total.reserve(1, 1);
    if (e != hipSuccess) return fail(VF_ERR_NOMEM, std::string("contour allocation failed: ") + hipGetErrorString(e));
    VF_HIP_TRY(hipMemcpyAsync(C.levels.p, levels, nlevels * sizeof(float), hipMemcpyHostToDevice, s));
    const CtGrid G = { t->n - 1u, t->nb, grid_step(t), spacing_of(t->inputs.u), t->d_hblk, t->d_bounds, C.levels.p, nlevels };
    hipLaunchKernelGGL(k_ct_count, dim3(t->nblocks), dim3(64), 0, s, G, C.count.p);
    VF_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ct_scan, dim3(1), dim3(1024), 0, s, t->nblocks, C.count.p, C.total.p);
    VF_HIP_TRY(hipGetLastError());
    unsigned long long nseg = 0;
    VF_HIP_TRY(hipMemcpyAsync(&nseg, C.total.p, sizeof nseg, hipMemcpyDeviceToHost, s));
    VF_HIP_TRY(hipStreamSynchronize(s));                      // (the level list is only borrowed; the count sizes the layer)
    const bool round = join == VF_JOIN_ROUND;
    const unsigned long long nrec = nseg * (round ? 2ull : 1ull);
    if (t->ov.nprims + nrec > kOvMaxPrims)
        return fail(VF_ERR_INVALID, "contours: " + std::to_string(nseg) + " segments (" + std::to_string(nrec) + " primitives) on top of the handle's " +
                                    std::to_string(t->ov.nprims) + " exceed the 2^24 primitive budget: fewer levels, VF_JOIN_NONE or a coarser grid");
    const float kb = 1.0f + depth_bias;                       // as vf_terrain_set_layer_occlusion forms it
    CtStyle S = {};
    S.hw = ov_clamp_px(width_px) * 0.5f; S.lift = lift; S.rgba = pack_rgba8(rgba); S.feature = t->ov.features;
    S.base = kOvDrape | (occlude ? kOvOcclude : 0u); S.round = round ? 1u : 0u;
    if (occlude) std::memcpy(&S.kb_bits, &kb, sizeof kb);
    const int rc = ov_append(t, (size_t)nrec, [&](OvIn *dst) -> int {
        hipLaunchKernelGGL(k_ct_emit, dim3(t->nblocks), dim3(64), 0, s, G, S, C.count.p, dst);
        VF_HIP_TRY(hipGetLastError());
        VF_HIP_TRY(hipStreamSynchronize(s));
        return VF_OK;
    }, {}, 0, false, t->ov.features + 1u, layer_id, occlude != 0);
    if (rc == VF_OK && nsegments) *nsegments = (uint32_t)nseg;
    return rc;
}

int vf_terrain_clear_overlays(vf_terrain *t)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    VF_HIP_TRY(wait_frame(t));
    ov_release(t);
    return VF_OK;
}

constexpr size_t kStageChunk = 8u << 20;
constexpr size_t kStageSlots = 4;
static unsigned copy_threads()
{
    if (const char *e = std::getenv("VF_COPY_THREADS")) { const int v = std::atoi(e); if (v >= 1) return (unsigned)std::min(v, 16); }
    const unsigned hw = std::thread::hardware_concurrency();
    return std::max(1u, std::min(4u, hw > 1 ? hw - 1 : 1u));
}
// Device -> pageable host memory through a ring of pinned chunks: the DMA engine fills chunk k + 1 .. k + 3 while host threads
// move chunk k out (a frame-sized destination is usually fresh memory: the copy out is page-fault bound, which is why it is
// spread over a few threads).  The calling thread only orchestrates: it enqueues a chunk once every thread is done with the
// chunk that used the slot before.  The ring is owned by the handle: nothing is allocated or registered per call (the
// reference maps a fresh buffer per call, src/terrain/mod.rs:446-451).
static bool is_pinned_host(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // (ordinary pageable memory: "invalid value")
    return a.type == hipMemoryTypeHost;
}
// Device -> page-locked host memory, queued on s.  Where the device can address the destination the bytes travel by a kernel's
// stores (k_copy_to_host) -- the same PCIe time as the copy engine's transfer (C4 frame: 1.35 against 1.30 ms), without the 8-10 ms
// the engine's FIRST transfer of a process costs, which a one-shot caller (construct, render once) would pay in its only read-back.
// The batch read-back keeps the copy engine: its copies run beside the next poses' kernels.
static hipError_t copy_to_pinned(void *host, const void *dev, size_t n, hipStream_t s)
{
    void *view = nullptr;
    if (n >= 4096 && hipHostGetDevicePointer(&view, host, 0) == hipSuccess && view && (((uintptr_t)view | (uintptr_t)dev) & 15u) == 0) {
        const size_t n16 = n / 16;
        const unsigned grid = (unsigned)std::min<size_t>(1024, (n16 + 255) / 256);
        hipLaunchKernelGGL(k_copy_to_host, dim3(grid), dim3(256), 0, s, (const uint4 *)dev, (uint4 *)view, n16, n);
        return hipGetLastError();
    }
    (void)hipGetLastError();
    return hipMemcpyAsync(host, dev, n, hipMemcpyDeviceToHost, s);
}
static int copy_to_host_staged(vf_terrain *t, uint8_t *dst, const uint8_t *src, size_t n, hipStream_t s)
{
    // a destination in pinned host memory (vf_host_alloc, or the caller's own hipHostMalloc / hipHostRegister): one transfer, nothing to stage
    if (is_pinned_host(dst)) { VF_HIP_TRY(copy_to_pinned(dst, src, n, s)); VF_HIP_TRY(finish_readback(t, s)); return VF_OK; }
    if (n < kStageChunk) { VF_HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, s)); VF_HIP_TRY(finish_readback(t, s)); return VF_OK; }
    if (!t->h_stage) VF_HIP_TRY(pinned_alloc((void **)&t->h_stage, kStageSlots * kStageChunk));
    for (auto &e : t->stage_ev) if (!e) VF_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const size_t nchunks = (n + kStageChunk - 1) / kStageChunk;
    const unsigned nthreads = copy_threads();
    auto chunk_len = [&](size_t k) { return k + 1 == nchunks ? n - k * kStageChunk : kStageChunk; };
    std::atomic<size_t> enqueued{0};                       // chunks whose copy + event are on the stream
    std::unique_ptr<std::atomic<uint32_t>[]> done(new std::atomic<uint32_t>[nchunks]);
    for (size_t k = 0; k < nchunks; ++k) done[k].store(0, std::memory_order_relaxed);
    std::atomic<int> failed{0};
    const int device = t->ctx->device;
    auto worker = [&](unsigned w) {
        (void)hipSetDevice(device);
        for (size_t k = 0; k < nchunks; ++k) {
            while (enqueued.load(std::memory_order_acquire) <= k) {
                if (failed.load(std::memory_order_relaxed)) return;
                std::this_thread::yield();
            }
            if (hipEventSynchronize(t->stage_ev[k % kStageSlots]) != hipSuccess) failed.store(1);
            else {
                const size_t len = chunk_len(k);
                const size_t lo = (len * w / nthreads) & ~(size_t)4095, hi = w + 1 == nthreads ? len : (len * (w + 1) / nthreads) & ~(size_t)4095;
                if (hi > lo) std::memcpy(dst + k * kStageChunk + lo, t->h_stage + (k % kStageSlots) * kStageChunk + lo, hi - lo);
            }
            done[k].fetch_add(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> pool;
    pool.reserve(nthreads);
    for (unsigned w = 0; w < nthreads; ++w) pool.emplace_back(worker, w);
    hipError_t err = hipSuccess;
    for (size_t i = 0; i < nchunks && err == hipSuccess && !failed.load(); ++i) {
        if (i >= kStageSlots)
            while (done[i - kStageSlots].load(std::memory_order_acquire) < nthreads) std::this_thread::yield();
        err = copy_to_pinned(t->h_stage + (i % kStageSlots) * kStageChunk, src + i * kStageChunk, chunk_len(i), s);
        if (err == hipSuccess) err = hipEventRecord(t->stage_ev[i % kStageSlots], s);
        if (err == hipSuccess) enqueued.store(i + 1, std::memory_order_release);
    }
    if (err == hipSuccess) { flush_tile_lists(t, s); flush_preplan(t, s); }   // (behind the last chunk's copy: the threads above wait for the chunks' events)
    if (err != hipSuccess) failed.store(1);
    for (auto &th : pool) th.join();
    if (err != hipSuccess) return fail(VF_ERR_HIP, hipGetErrorString(err));
    if (failed.load()) return fail(VF_ERR_HIP, "device -> host copy failed");
    return VF_OK;
}

int vf_terrain_read_rgba(vf_terrain *t, uint8_t *dst, uint32_t y0, uint32_t rows)
{
    if (!t || !dst) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->rendered) return fail(VF_ERR_INVALID, "nothing rendered yet");
    if (t->shard_tiles) return fail(VF_ERR_INVALID, "tile-sharded handle: read with vf_terrain_read_tiles");
    if ((uint64_t)y0 + rows > (t->ss > 1u ? t->oH : t->local_rows)) return fail(VF_ERR_INVALID, "row range outside the local rows");   // (supersampled: a whole-frame handle)
    int rc = vf_terrain_sync(t);
    if (rc != VF_OK) return rc;
    return copy_to_host_staged(t, dst, (const uint8_t *)(t->d_rgba + (size_t)y0 * t->oW), (size_t)rows * t->oW * 4,
                               t->last_stream ? t->last_stream : t->ctx->stream);
}

int vf_host_alloc(size_t bytes, void **host)
{
    if (!host || bytes == 0) return fail(VF_ERR_INVALID, "NULL argument or zero size");
    *host = nullptr;
    hipError_t e = pinned_alloc(host, bytes);
    if (e != hipSuccess) { *host = nullptr; return fail(e == hipErrorOutOfMemory ? VF_ERR_NOMEM : VF_ERR_HIP, std::string("page-locked allocation: ") + hipGetErrorString(e)); }
    return VF_OK;
}
void vf_host_free(void *host) { pinned_free(host); }

int vf_terrain_read_png_scanlines(vf_terrain *t, const uint8_t **host_scanlines, size_t *nbytes)
{
    if (!t || !host_scanlines || !nbytes) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->rendered) return fail(VF_ERR_INVALID, "nothing rendered yet");
    if (t->shard_tiles || t->local_rows != t->H) return fail(VF_ERR_INVALID, "PNG read-back needs the whole frame on one handle");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    const size_t n = ((size_t)t->oW * 4 + 1) * t->oH;
    if (!t->d_png) VF_HIP_TRY(hipMalloc(&t->d_png, n));
    hipStream_t s = t->last_stream ? t->last_stream : t->ctx->stream;
    hipLaunchKernelGGL(k_png_filter, dim3(t->oH), dim3(256), 0, s, (const uint32_t *)t->d_rgba, t->oW, t->d_png);
    VF_HIP_TRY(hipGetLastError());
    // the scanlines land in a page-locked buffer of the handle (pinned_alloc: 2.6 ms to make for a C4 frame, then one DMA per frame):
    // persistent, where the reference allocates per call (:446-451)
    if (!t->h_png) VF_HIP_TRY(pinned_alloc((void **)&t->h_png, n));
    uint8_t *host = t->h_png;
    VF_HIP_TRY(copy_to_pinned(host, t->d_png, n, s));
    VF_HIP_TRY(finish_readback(t, s));                      // (a waiting caller's next plan runs while the host deflates)
    *host_scanlines = host;
    *nbytes = n;
    return VF_OK;
}

int vf_terrain_read_visibility(vf_terrain *t, uint32_t *dst)
{
    if (!t || !dst) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->have_uniforms) return fail(VF_ERR_INVALID, "uniforms not set");
    if (t->shard_tiles) return fail(VF_ERR_INVALID, "visibility read-back needs a row-oriented handle (vf_terrain_set_shard)");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    // the visibility tile normally lives and dies in LDS: the last frame is rendered again with the debug store enabled
    int rc = render_visibility(t);
    if (rc != VF_OK) return rc;
    VF_HIP_TRY(hipMemcpy(dst, t->d_vis, (size_t)t->local_rows * t->W * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return VF_OK;
}

// Persistent workgroups for `regions` regions of a pass over the stored visibility (RegionWalk): a multiple of 8 of them (one share
// per XCD), at most per_cu per CU; the environment variable `env`, when set, gives per_cu.  FEW per CU on purpose: the record gathers
// of more waves than these evict each other's lines from the 32 KB L1 (C4 fill camera, k_resolve4: 3 per CU 0.130 ms, 4: 0.144, 8: 0.148)
static dim3 region_grid(const vf_terrain *t, uint32_t regions, const char *env, uint32_t per_cu)
{
    if (const char *v = std::getenv(env)) per_cu = (uint32_t)std::max(1, std::atoi(v));
    const uint32_t cus = (uint32_t)std::max(8, t->ctx->prop.multiProcessorCount) / 8u * 8u;
    return dim3(std::min<uint32_t>((regions + 7u) / 8u * 8u, cus * per_cu));
}

int vf_terrain_debug_fragment_stage(vf_terrain *t, uint32_t repeats, vf_fragment_timing *out)
{
    if (!t || !out) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->have_uniforms) return fail(VF_ERR_INVALID, "uniforms not set");
    if (t->shard_tiles || t->nranks != 1) return fail(VF_ERR_INVALID, "fragment-stage diagnostics need a whole-frame handle");
    if (repeats == 0) repeats = 1;
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    int rc = render_visibility(t);                          // d_vis + the frame as the tile kernel shades it (d_rgba_scratch)
    if (rc != VF_OK) return rc;
    const size_t npx = (size_t)t->W * t->H;
    uint32_t *d_out = nullptr;
    VF_HIP_TRY(hipMalloc(&d_out, npx * sizeof(uint32_t)));
    if (!t->d_diag) { hipError_t e = hipMalloc(&t->d_diag, 4 * sizeof(uint32_t)); if (e != hipSuccess) { (void)hipFree(d_out); return fail(VF_ERR_NOMEM, "diagnostics allocation failed"); } }
    uint32_t redo = 0;                                      // did the frame hold clipped / oversized primitives?  (normally not)
    hipError_t err = hipMemcpy(&redo, t->ps[t->last_set].work_count + 3, sizeof redo, hipMemcpyDeviceToHost);
    FrameParams P;
    const FrameInputs &in = t->have_frame ? t->drawn_inputs : t->inputs;     // the frame render_visibility has just drawn again
    build_params(t, in, P);
    const bool fast = fast_shading(in);
    hipStream_t s = t->ctx->stream;
    // 16-byte HBM accesses, four pixels per lane, when the rows allow them and the frame holds no clipped primitive (VF_RESOLVE_PER_PIXEL=1: the per-pixel form)
    const bool quads = !redo && t->W % 4u == 0 && !std::getenv("VF_RESOLVE_PER_PIXEL");
    const dim3 grid = region_grid(t, ((t->W + 31u) / 32u) * ((t->H + 7u) / 8u), "VF_RESOLVE_PER_CU", 4u), threads(256);   // 32 x 8 pixel regions
    const vf_terrain::PlanState &S = t->ps[t->last_set];     // the set-up of the frame just rendered
    const SetupView V = { S.vtx, t->d_hblk, S.recs, S.gen };
    constexpr uint32_t RQ = 8u, RY = 32u;                  // k_resolve4's region: 8 quads x 32 rows
    const dim3 grid4 = region_grid(t, ((t->W / 4u + RQ - 1u) / RQ) * ((t->H + RY - 1u) / RY), "VF_RESOLVE_PER_CU", 3u);
    auto launch = [&](uint32_t *covered) {
        if (quads && fast) hipLaunchKernelGGL((k_resolve4<true>), grid4, threads, 0, s, P, V, t->d_lut, t->ctx->d_thresh, (const uint4 *)t->d_vis, (uint4 *)d_out, covered);
        else if (quads) hipLaunchKernelGGL((k_resolve4<false>), grid4, threads, 0, s, P, V, t->d_lut, t->ctx->d_thresh, (const uint4 *)t->d_vis, (uint4 *)d_out, covered);
        else if (redo && fast) hipLaunchKernelGGL((k_resolve<true, true>), grid, threads, 0, s, P, V, t->d_lut, t->ctx->d_thresh, t->d_vis, d_out, covered);
        else if (redo) hipLaunchKernelGGL((k_resolve<true, false>), grid, threads, 0, s, P, V, t->d_lut, t->ctx->d_thresh, t->d_vis, d_out, covered);
        else if (fast) hipLaunchKernelGGL((k_resolve<false, true>), grid, threads, 0, s, P, V, t->d_lut, t->ctx->d_thresh, t->d_vis, d_out, covered);
        else hipLaunchKernelGGL((k_resolve<false, false>), grid, threads, 0, s, P, V, t->d_lut, t->ctx->d_thresh, t->d_vis, d_out, covered);
    };
    if (err == hipSuccess) err = hipMemsetAsync(t->d_diag, 0, 4 * sizeof(uint32_t), s);
    float ms = 0.0f;
    if (err == hipSuccess) err = time_launches(s, repeats, ms, [&](bool warm) { launch(warm ? t->d_diag : nullptr); return hipGetLastError(); });   // the warm-up launch counts the covered pixels
    uint32_t covered = 0;
    if (err == hipSuccess) err = hipMemcpy(&covered, t->d_diag, sizeof covered, hipMemcpyDeviceToHost);
    // the resolved frame against the one the tile kernel produced (row-major whole frame in both buffers)
    uint32_t equal = 0;
    if (err == hipSuccess) {
        std::vector<uint32_t> a(npx), b(npx);
        err = hipMemcpy(a.data(), d_out, npx * 4, hipMemcpyDeviceToHost);
        if (err == hipSuccess) err = hipMemcpy(b.data(), t->d_rgba_scratch, npx * 4, hipMemcpyDeviceToHost);
        if (err == hipSuccess) equal = std::memcmp(a.data(), b.data(), npx * 4) == 0 ? 1u : 0u;
    }
    (void)hipFree(d_out);
    if (err != hipSuccess) return fail(VF_ERR_HIP, std::string("fragment-stage diagnostics: ") + hipGetErrorString(err));
    out->resolve_ms = ms; out->covered_pixels = covered; out->repeats = repeats; out->equal_to_frame = equal;
    return VF_OK;
}

// ---- geometry buffers (vf_gbuffer.h) ---------------------------------------------------

// The frame the three calls describe: drawn again with the visibility store on (render_visibility: d_vis and the set-up arrays of
// t->last_set are complete when it returns), its parameters, and whether it held a clipped / oversized primitive.
struct GbFrame { FrameParams P; SetupView V; bool clipped; };

static int gb_frame(vf_terrain *t, GbFrame &F)
{
    if (!t->have_uniforms) return fail(VF_ERR_INVALID, "uniforms not set");
    if (t->shard_tiles || t->nranks != 1) return fail(VF_ERR_INVALID, "geometry buffers need a whole-frame handle: sharded handles are not supported");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    const int rc = render_visibility(t);
    if (rc != VF_OK) return rc;
    uint32_t redo = 0;
    VF_HIP_TRY(hipMemcpy(&redo, t->ps[t->last_set].work_count + 3, sizeof redo, hipMemcpyDeviceToHost));
    build_params(t, t->have_frame ? t->drawn_inputs : t->inputs, F.P);
    const vf_terrain::PlanState &S = t->ps[t->last_set];
    F.V = { S.vtx, t->d_hblk, S.recs, S.gen };
    F.clipped = redo != 0;
    return VF_OK;
}

// the launch shape of for_each_visible (vf_visible.h): 32 x 8 pixel regions, four workgroups per CU, as k_resolve
static dim3 gb_grid(const vf_terrain *t) { return region_grid(t, ((t->W + 31u) / 32u) * ((t->H + 7u) / 8u), "VF_GBUFFER_PER_CU", 4u); }

static void gb_launch(const vf_terrain *t, const GbFrame &F, const GbPlanes &O, hipStream_t s)
{
    if (F.clipped) hipLaunchKernelGGL((k_gbuffer<true>), gb_grid(t), dim3(256), 0, s, F.P, F.V, (const uint32_t *)t->d_vis, O);
    else hipLaunchKernelGGL((k_gbuffer<false>), gb_grid(t), dim3(256), 0, s, F.P, F.V, (const uint32_t *)t->d_vis, O);
}

// Work queued on a stream of the caller's reads d_vis and the set-up arrays of t->last_set: that set's `drawn` event is recorded
// again behind it, so whatever waits for the set before it is reused (plan_frame) or for the frame before (draw_frame on another
// stream) waits for this too, and the handle's own streams are ordered behind it.
static hipError_t gb_order_after(vf_terrain *t, hipStream_t s)
{
    hipEvent_t ev = t->ps[t->last_set].drawn;
    hipError_t e = hipEventRecord(ev, s);
    if (e == hipSuccess && t->last_stream && t->last_stream != s) e = hipStreamWaitEvent(t->last_stream, ev, 0);
    if (e == hipSuccess && t->ctx->stream != s) e = hipStreamWaitEvent(t->ctx->stream, ev, 0);
    return e;
}

int vf_terrain_gbuffer_device(vf_terrain *t, float *dev_depth, float *dev_position, float *dev_normal, uint32_t *dev_primitive, void *stream)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (!dev_depth && !dev_position && !dev_normal && !dev_primitive) return fail(VF_ERR_INVALID, "no plane requested");
    GbFrame F;
    const int rc = gb_frame(t, F);
    if (rc != VF_OK) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : t->ctx->stream;
    gb_launch(t, F, GbPlanes{ dev_depth, dev_position, dev_normal, dev_primitive }, s);
    VF_HIP_TRY(hipGetLastError());
    VF_HIP_TRY(gb_order_after(t, s));
    return VF_OK;
}

// The planes of `mask` (bit k: depth, position, normal, primitive) packed one behind the other in the handle's d_gb, grown to hold them
struct GbLayout {
    size_t bytes[4] = {};                // of plane k (0: not asked for)
    GbPlanes dev = {};
    void *plane(int k) const { void *const p[4] = { dev.depth, dev.position, dev.normal, dev.primitive }; return p[k]; }
};

static int gb_planes(vf_terrain *t, uint32_t mask, GbLayout &L)
{
    const size_t npx = (size_t)t->W * t->H, words[4] = { 1, 3, 3, 1 };
    size_t off[4], total = 0;
    for (int k = 0; k < 4; ++k) { off[k] = total; L.bytes[k] = (mask & (1u << k)) ? npx * words[k] * 4 : 0; total += L.bytes[k]; }
    if (t->d_gb.reserve(total, total) != hipSuccess) { (void)hipGetLastError(); return fail(VF_ERR_NOMEM, "geometry-buffer allocation failed"); }
    auto dev = [&](int k) -> void * { return L.bytes[k] ? t->d_gb.p + off[k] : nullptr; };
    L.dev = GbPlanes{ (float *)dev(0), (float *)dev(1), (float *)dev(2), (uint32_t *)dev(3) };
    return VF_OK;
}

int vf_terrain_read_gbuffer(vf_terrain *t, float *depth, float *position, float *normal, uint32_t *primitive)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (!depth && !position && !normal && !primitive) return fail(VF_ERR_INVALID, "no plane requested");
    GbFrame F;
    int rc = gb_frame(t, F);
    if (rc != VF_OK) return rc;
    void *const host[4] = { depth, position, normal, primitive };
    GbLayout L;
    rc = gb_planes(t, (depth ? 1u : 0u) | (position ? 2u : 0u) | (normal ? 4u : 0u) | (primitive ? 8u : 0u), L);
    if (rc != VF_OK) return rc;
    hipStream_t s = t->ctx->stream;
    gb_launch(t, F, L.dev, s);
    VF_HIP_TRY(hipGetLastError());
    for (int k = 0; k < 4; ++k)
        if (host[k]) VF_HIP_TRY(hipMemcpyAsync(host[k], L.plane(k), L.bytes[k], hipMemcpyDeviceToHost, s));
    VF_HIP_TRY(hipStreamSynchronize(s));
    return VF_OK;
}

int vf_terrain_pick(vf_terrain *t, const int32_t *pixels_xy, uint32_t n, float *out8)
{
    if (!t || (n && (!pixels_xy || !out8))) return fail(VF_ERR_INVALID, "NULL argument");
    for (uint32_t k = 0; k < n; ++k)
        if (pixels_xy[2 * k] < 0 || pixels_xy[2 * k + 1] < 0 || (uint32_t)pixels_xy[2 * k] >= t->oW || (uint32_t)pixels_xy[2 * k + 1] >= t->oH)
            return fail(VF_ERR_INVALID, "pixel " + std::to_string(k) + " (" + std::to_string(pixels_xy[2 * k]) + ", " + std::to_string(pixels_xy[2 * k + 1]) +
                                        ") lies outside the " + std::to_string(t->oW) + " x " + std::to_string(t->oH) + " frame");
    // a supersampled handle answers for the pixel's representative sample (ss x + ss / 2, ss y + ss / 2): the kernel sees sample coordinates
    std::vector<int32_t> mapped;
    if (t->ss > 1u && n) {
        mapped.resize(2u * (size_t)n);
        for (size_t k = 0; k < 2u * (size_t)n; ++k) mapped[k] = (int32_t)(t->ss * (uint32_t)pixels_xy[k] + t->ss / 2u);
        pixels_xy = mapped.data();
    }
    GbFrame F;
    int rc = gb_frame(t, F);
    if (rc != VF_OK || n == 0) return rc;
    const size_t in_bytes = ((size_t)n * 8 + 31) / 32 * 32, out_bytes = (size_t)n * sizeof(GbPixel);
    if (t->d_pick.reserve(in_bytes + out_bytes, in_bytes + out_bytes) != hipSuccess) { (void)hipGetLastError(); return fail(VF_ERR_NOMEM, "geometry-buffer allocation failed"); }
    hipStream_t s = t->ctx->stream;
    const int2 *d_in = (const int2 *)t->d_pick.p;
    GbPixel *d_out = (GbPixel *)(t->d_pick.p + in_bytes);
    VF_HIP_TRY(hipMemcpyAsync(t->d_pick.p, pixels_xy, (size_t)n * 8, hipMemcpyHostToDevice, s));
    const dim3 grid((n + 255u) / 256u);
    if (F.clipped) hipLaunchKernelGGL((k_gbuffer_pick<true>), grid, dim3(256), 0, s, F.P, F.V, (const uint32_t *)t->d_vis, d_in, n, d_out);
    else hipLaunchKernelGGL((k_gbuffer_pick<false>), grid, dim3(256), 0, s, F.P, F.V, (const uint32_t *)t->d_vis, d_in, n, d_out);
    VF_HIP_TRY(hipGetLastError());
    VF_HIP_TRY(hipMemcpyAsync(out8, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    VF_HIP_TRY(hipStreamSynchronize(s));
    return VF_OK;
}

int vf_terrain_debug_gbuffer_stage(vf_terrain *t, uint32_t planes, uint32_t repeats, float *ms)
{
    if (!t || !ms) return fail(VF_ERR_INVALID, "NULL argument");
    if (!(planes & 15u) || (planes & ~15u)) return fail(VF_ERR_INVALID, "planes: a non-empty combination of VF_GBUFFER_DEPTH / _POSITION / _NORMAL / _PRIMITIVE");
    if (repeats == 0) repeats = 1;
    GbFrame F;
    int rc = gb_frame(t, F);
    if (rc != VF_OK) return rc;
    GbLayout L;
    rc = gb_planes(t, planes, L);
    if (rc != VF_OK) return rc;
    hipStream_t s = t->ctx->stream;
    float mean = 0.0f;
    const hipError_t err = time_launches(s, repeats, mean, [&](bool) { gb_launch(t, F, L.dev, s); return hipGetLastError(); });
    if (err != hipSuccess) return fail(VF_ERR_HIP, std::string("geometry-buffer diagnostics: ") + hipGetErrorString(err));
    *ms = mean;
    return VF_OK;
}

// ---- supersampling (vf_resolve.h) --------------------------------------------------------

// the resolve launch (declared in front of draw_frame; see there for why it stands here): persistent, a few workgroups per CU
static void resolve_launch(const vf_terrain *t, hipStream_t s, uint32_t *dst)
{
    const uint32_t px = t->ss == 2u ? (uint32_t)SsShape<2>::PX : (t->ss == 3u ? (uint32_t)SsShape<3>::PX : (uint32_t)SsShape<4>::PX);
    const uint32_t lanes = ((t->oW + px - 1u) / px) * t->oH;
    const dim3 grid(std::min<uint32_t>((lanes + 255u) / 256u, (uint32_t)std::max(1, t->ctx->prop.multiProcessorCount) * 8u)), threads(256);
    const float *dec = t->ctx->d_decode, *thr = t->ctx->d_thresh;
    if (t->ss == 2u) hipLaunchKernelGGL((k_ss_resolve<2>), grid, threads, 0, s, (const uint32_t *)t->d_samples, t->oW, t->oH, dec, thr, dst);
    else if (t->ss == 3u) hipLaunchKernelGGL((k_ss_resolve<3>), grid, threads, 0, s, (const uint32_t *)t->d_samples, t->oW, t->oH, dec, thr, dst);
    else hipLaunchKernelGGL((k_ss_resolve<4>), grid, threads, 0, s, (const uint32_t *)t->d_samples, t->oW, t->oH, dec, thr, dst);
}

int vf_terrain_supersampling(const vf_terrain *t, uint32_t *factor, uint32_t *sample_width, uint32_t *sample_height)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (factor) *factor = t->ss;
    if (sample_width) *sample_width = t->W;
    if (sample_height) *sample_height = t->H;
    return VF_OK;
}

// the samples of the frame rendered last: what the resolve read (a frame in flight is waited for / ordered in front)
static int samples_ready(const vf_terrain *t)
{
    if (t->ss <= 1u) return fail(VF_ERR_INVALID, "the handle is not supersampled: it keeps no samples apart from its frame (vf_terrain_create_supersampled)");
    if (!t->rendered) return fail(VF_ERR_INVALID, "nothing rendered yet");
    return VF_OK;
}

int vf_terrain_read_samples(vf_terrain *t, uint8_t *dst)
{
    if (!t || !dst) return fail(VF_ERR_INVALID, "NULL argument");
    if (int rc = samples_ready(t)) return rc;
    int rc = vf_terrain_sync(t);
    if (rc != VF_OK) return rc;
    return copy_to_host_staged(t, dst, (const uint8_t *)t->d_samples, (size_t)t->W * t->H * 4, t->last_stream ? t->last_stream : t->ctx->stream);
}

int vf_terrain_samples_device(vf_terrain *t, void *dev_dst, void *stream)
{
    if (!t || !dev_dst) return fail(VF_ERR_INVALID, "NULL argument");
    if (int rc = samples_ready(t)) return rc;
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : t->ctx->stream;
    if (t->last_stream && t->last_stream != s) VF_HIP_TRY(hipStreamWaitEvent(s, t->ps[t->last_set].drawn, 0));
    VF_HIP_TRY(hipMemcpyAsync(dev_dst, t->d_samples, (size_t)t->W * t->H * 4, hipMemcpyDeviceToDevice, s));
    VF_HIP_TRY(gb_order_after(t, s));                       // (the next frame overwrites the samples: it waits for this copy)
    return VF_OK;
}

int vf_terrain_debug_resolve_stage(vf_terrain *t, uint32_t repeats, float *ms)
{
    if (!t || !ms) return fail(VF_ERR_INVALID, "NULL argument");
    if (int rc = samples_ready(t)) return rc;
    if (repeats == 0) repeats = 1;
    int rc = vf_terrain_sync(t);
    if (rc != VF_OK) return rc;
    uint32_t *d_out = nullptr;                              // (not the frame: it may hold overlays)
    if (hipMalloc(&d_out, (size_t)t->oW * t->oH * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); return fail(VF_ERR_NOMEM, "resolve diagnostics allocation failed"); }
    hipStream_t s = t->ctx->stream;
    float mean = 0.0f;
    const hipError_t err = time_launches(s, repeats, mean, [&](bool) { resolve_launch(t, s, d_out); return hipGetLastError(); });
    (void)hipFree(d_out);
    if (err != hipSuccess) return fail(VF_ERR_HIP, std::string("resolve diagnostics: ") + hipGetErrorString(err));
    *ms = mean;
    return VF_OK;
}

// ---- cast shadows (vf_shadow.h) ---------------------------------------------------------

// The sheared grid lines that run along the horizontal direction (hx, hz): S.n ... S.nchunks, and the
// magnitude of the direction's major component; false when it has no usable horizontal part.  The ratio comes from the vector as
// given, not from a normalised one: it is free of scale, so the lines depend on the azimuth alone.
static bool line_geometry(const vf_terrain *t, float hx, float hz, ShadowPlan &S, float &amaj)
{
    const float ax = std::fabs(hx), az = std::fabs(hz);
    const bool zmajor = az > ax;                              // a tie goes to x
    amaj = zmajor ? az : ax;
    const float amin = zmajor ? ax : az;
    const float smaj = zmajor ? hz : hx, smin = zmajor ? hx : hz;
    if (!(amaj > 0.0f) || !std::isfinite(amaj) || !(amin <= amaj)) return false;
    S.n = t->n; S.nb = t->nb;
    S.zmajor = zmajor ? 1u : 0u;
    S.from_high = smaj > 0.0f ? 1u : 0u;
    S.s = smin < 0.0f ? -1 : 1;
    S.a = amin / amaj;
    const int32_t R = (int32_t)std::rint((float)(t->n - 1u) * S.a);
    S.c_lo = S.s > 0 ? 0 : -R;
    S.nlines = t->n + (uint32_t)R;
    S.nchunks = (t->n + kShChunk - 1u) / kShChunk;
    return true;
}

// The frame of reference of the field for the uniforms `u`; false: every vertex is lit.
static bool sun_plan(const vf_terrain *t, const float sun[3], float spacing, float exag, float strength, float softness, float bias, ShadowPlan &S)
{
    const float sy = sun[1];
    float amaj;
    if (!line_geometry(t, sun[0], sun[2], S, amaj) || !std::isfinite(sy)) return false;
    const float d = sy > 0.0f ? ((grid_step(t) * spacing) * sy) / amaj : 0.0f;
    if (!std::isfinite(d)) return false;
    S.d = d; S.exag = exag; S.strength = strength; S.softness = softness; S.bias = bias;
    return true;
}

// ... of the handle's own sun and shadow parameters
static bool shadow_plan(const vf_terrain *t, const float *u, ShadowPlan &S)
{
    const vf_terrain::Shadows &H = t->sh;
    return sun_plan(t, u + 32, spacing_of(u), u[38], H.strength, H.softness, H.bias, S);
}

// `lit` holds the field of the uniforms `u`, the handle's heights and shadow parameters once the work queued on `s` is done.  The
// displaced-height cache must be current and ordered before `s` (a frame's plan, ct_heights_current).  force: compute it anyway.
static int shadow_field(vf_terrain *t, const float *u, hipStream_t s, bool force = false)
{
    vf_terrain::Shadows &H = t->sh;
    std::vector<uint32_t> key = key_of({ u[32], u[33], u[34], spacing_of(u), u[38], H.strength, H.softness, H.bias });
    bool current;
    if (int rc = H.lit.prepare(t, key, force, "shadow field allocation failed", &current)) return rc;
    if (current) return VF_OK;
    const size_t nv = (size_t)t->n * t->n;
    ShadowPlan S;
    if (!shadow_plan(t, u, S)) hipLaunchKernelGGL((k_shadow_fill<0>), dim3((uint32_t)((nv + 255u) / 256u)), dim3(256), 0, s, nv, H.lit.d.p);
    else {
        // (grown once, to what any sun needs: at most 2n - 1 lines)
        if (H.d_cmax.reserve((size_t)S.nchunks * S.nlines, (size_t)S.nchunks * 2u * t->n) != hipSuccess) { (void)hipGetLastError(); return fail(VF_ERR_NOMEM, "shadow scan allocation failed"); }
        const dim3 grid(S.nchunks, (S.nlines + kShLines - 1u) / kShLines), threads(256);
        if (S.zmajor) hipLaunchKernelGGL((k_shadow_chunk_max<true>), grid, threads, 0, s, S, (const float *)t->d_hblk, H.d_cmax.p);
        else hipLaunchKernelGGL((k_shadow_chunk_max<false>), grid, threads, 0, s, S, (const float *)t->d_hblk, H.d_cmax.p);
        hipLaunchKernelGGL((k_shadow_carry<0>), dim3((S.nlines + 255u) / 256u), threads, 0, s, S.nlines, S.nchunks, H.d_cmax.p);
        if (S.zmajor) hipLaunchKernelGGL((k_shadow_lit<true>), grid, threads, 0, s, S, (const float *)t->d_hblk, (const float *)H.d_cmax.p, H.lit.d.p);
        else hipLaunchKernelGGL((k_shadow_lit<false>), grid, threads, 0, s, S, (const float *)t->d_hblk, (const float *)H.d_cmax.p, H.lit.d.p);
    }
    VF_HIP_TRY(hipGetLastError());
    H.lit.computed(t, key);
    return VF_OK;
}

static int ambient_field(vf_terrain *t, const float *u, hipStream_t s, bool force = false);

// The fields a pass reads hold the values of the uniforms `u` once the work queued on `s` is done: the shadow field
// if asked, the sky-view field if asked; at no cost when they are current.  force: compute them anyway.
static int relight_fields(vf_terrain *t, const float *u, hipStream_t s, bool shadows, bool ambient, bool force = false)
{
    if (shadows) { if (int rc = shadow_field(t, u, s, force)) return rc; }
    if (ambient) { if (int rc = ambient_field(t, u, s, force)) return rc; }
    return VF_OK;
}

// Where the levels of a drape's mip pyramid lie: level k is w[k] x h[k] texels, halved rounding up; levels 1 ... in
// one buffer at texel offsets off[k], each even (16-byte aligned rows for the build kernel's vector accesses); texels: its length
struct MipLayout {
    uint32_t levels;
    uint32_t w[kMipLevelsMax], h[kMipLevelsMax];
    size_t off[kMipLevelsMax], texels;
};

static MipLayout mip_layout(uint32_t iw, uint32_t ih)
{
    MipLayout L = {};
    L.w[0] = iw; L.h[0] = ih; L.levels = 1;
    while ((L.w[L.levels - 1u] > 1u || L.h[L.levels - 1u] > 1u) && L.levels < (uint32_t)kMipLevelsMax) {
        const uint32_t k = L.levels++;
        L.w[k] = std::max(1u, (L.w[k - 1u] + 1u) >> 1); L.h[k] = std::max(1u, (L.h[k - 1u] + 1u) >> 1);
        L.off[k] = L.texels;
        L.texels += ((size_t)L.w[k] * L.h[k] + 1u) & ~(size_t)1u;
    }
    return L;
}

// The build alone: the launches that make the pyramid of layout L in d_pyr (which holds L.texels texels) from the image held, on
// `s`.  Three levels per launch (vf_drape_mips.h): the first reads the image, the later ones binary16 texels.  Touches no state.
static void mips_launch(const vf_terrain *t, hipStream_t s, const MipLayout &L)
{
    const vf_terrain::DrapeMipState &M = t->dm;
    for (uint32_t k = 0; k + 1u < L.levels; k += 3u) {
        const uint32_t nout = std::min(3u, L.levels - 1u - k);
        uint2 *d[3];
        for (uint32_t q = 0; q < 3u; ++q) d[q] = q < nout ? M.d_pyr.p + L.off[k + 1u + q] : nullptr;
        const dim3 grid((L.w[k] + 63u) / 64u, (L.h[k] + 31u) / 32u), threads(256);
        if (k == 0u) hipLaunchKernelGGL((k_drape_mips<true>), grid, threads, 0, s, (const void *)t->dr.d_img.p, (const float *)t->ctx->d_decode, L.w[k], L.h[k], nout, d[0], d[1], d[2]);
        else hipLaunchKernelGGL((k_drape_mips<false>), grid, threads, 0, s, (const void *)(M.d_pyr.p + L.off[k]), (const float *)nullptr, L.w[k], L.h[k], nout, d[0], d[1], d[2]);
    }
}

// The pyramid of the image held is complete in d_pyr once the work queued on `s` is done (which is ordered behind the image's
// upload): built when stale -- after a new image or after enabling -- and at no cost otherwise.  The buffer is allocated when first
// needed and kept from image to image while the layout's texel count stays (an image update of the same size frees and allocates
// nothing); the caller of whatever made it stale has waited for the frames that read the old one.
static int mips_current(vf_terrain *t, hipStream_t s)
{
    vf_terrain::DrapeMipState &M = t->dm;
    if (!M.enabled || !t->dr.iw) return VF_OK;
    const MipLayout L = mip_layout(t->dr.iw, t->dr.ih);
    if (L.levels < 2u) { M.d_pyr.release(); M.stale = false; return VF_OK; }   // (a 1 x 1 image is its own pyramid)
    if (M.d_pyr.cap != L.texels) {
        M.d_pyr.release();
        M.stale = true;
        if (M.d_pyr.reserve(L.texels, L.texels) != hipSuccess) { (void)hipGetLastError(); return fail(VF_ERR_NOMEM, "drape mip pyramid allocation failed"); }
    }
    if (!M.stale) return VF_OK;
    mips_launch(t, s, L);
    VF_HIP_TRY(hipGetLastError());
    M.stale = false; M.builds++;
    return VF_OK;
}

// Both instantiations of a pass of the relight kernel (vf_relight.h), in k_resolve's launch shape (gb_grid).  shadows / ambient:
// the pass reads that field (kShadow reads the shadow field, kAmbient the sky-view field, whatever they say).
static void relight_launch(const vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba, Relight pass,
                           bool shadows, bool ambient)
{
    RelightParams R = {};
    R.lit = shadows || pass == kShadow ? t->sh.lit.d.p : nullptr;
    R.sky = ambient || pass == kAmbient ? t->am.sky.d.p : nullptr;
    R.amb_strength = t->am.strength;
    const dim3 grid = gb_grid(t), threads(256);
#define VF_RELIGHT(CLIPPED, PASS) hipLaunchKernelGGL((k_relight<CLIPPED, PASS>), grid, threads, 0, s, P, V, (const float *)t->d_lut, (const float *)t->ctx->d_thresh, \
                                                     (const uint32_t *)t->d_vis, R, redo, rgba)
    if (pass == kShadow) { VF_RELIGHT(false, kShadow); VF_RELIGHT(true, kShadow); }
    else if (pass == kAmbient) { VF_RELIGHT(false, kAmbient); VF_RELIGHT(true, kAmbient); }
    else {
        const vf_terrain::Drape &H = t->dr;
        R.decode = t->ctx->d_decode; R.img = H.d_img.p;
        DrapeParams &D = R.D;
        D.x0 = H.extent[0]; D.z0 = H.extent[1];
        D.sx = (float)H.iw / (H.extent[2] - H.extent[0]); D.sz = (float)H.ih / (H.extent[3] - H.extent[1]);
        D.iw = H.iw; D.ih = H.ih; D.opacity = H.opacity; D.linear = H.filter == VF_DRAPE_LINEAR ? 1u : 0u;
        if (pass == kDrape) { VF_RELIGHT(false, kDrape); VF_RELIGHT(true, kDrape); }
        else {                                                 // kDrapeMip: the pyramid beside it (current: mips_current)
            RelightAnisoParams RA = {};
            static_cast<RelightParams &>(RA) = R;
            const MipLayout L = mip_layout(H.iw, H.ih);
            RA.M.levels = L.levels; RA.M.bias = t->dm.bias;
            for (uint32_t k = 0; k < L.levels; ++k) { RA.M.w[k] = (uint16_t)L.w[k]; RA.M.h[k] = (uint16_t)L.h[k]; RA.M.lvl[k] = k ? t->dm.d_pyr.p + L.off[k] : nullptr; }
            if (pass == kDrapeMip) {
                const RelightMipParams &RM = RA;
                hipLaunchKernelGGL((k_relight<false, kDrapeMip>), grid, threads, 0, s, P, V, (const float *)t->d_lut, (const float *)t->ctx->d_thresh,
                                   (const uint32_t *)t->d_vis, RM, redo, rgba);
                hipLaunchKernelGGL((k_relight<true, kDrapeMip>), grid, threads, 0, s, P, V, (const float *)t->d_lut, (const float *)t->ctx->d_thresh,
                                   (const uint32_t *)t->d_vis, RM, redo, rgba);
            } else {                                           // kDrapeAniso: the largest anisotropy A and 1 / A^2 behind that
                RA.max_aniso = t->dm.aniso; RA.inv_a2 = 1.0f / (float)(t->dm.aniso * t->dm.aniso);
                hipLaunchKernelGGL((k_relight<false, kDrapeAniso>), grid, threads, 0, s, P, V, (const float *)t->d_lut, (const float *)t->ctx->d_thresh,
                                   (const uint32_t *)t->d_vis, RA, redo, rgba);
                hipLaunchKernelGGL((k_relight<true, kDrapeAniso>), grid, threads, 0, s, P, V, (const float *)t->d_lut, (const float *)t->ctx->d_thresh,
                                   (const uint32_t *)t->d_vis, RA, redo, rgba);
            }
        }
    }
#undef VF_RELIGHT
}

// A relight pass of a frame, on the draw stream behind its tile kernels (which stored the visibility) and the pass before: the
// fields it reads if they are stale, then the shade pass over the covered pixels.  The drape comes behind the shadow / ambient pass,
// which has brought the fields up to date; they are checked again here, at no cost when they are current.
static int relight_pass(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba, Relight pass,
                        bool shadows, bool ambient)
{
    if (int rc = relight_fields(t, t->inputs.u, s, shadows, ambient)) return rc;
    if (relight_drapes(pass) && t->dr.copied) VF_HIP_TRY(hipStreamWaitEvent(s, t->dr.copied, 0));
    if (relight_mips(pass)) { if (int rc = mips_current(t, s)) return rc; }
    relight_launch(t, s, P, V, redo, rgba, pass, shadows, ambient);
    VF_HIP_TRY(hipGetLastError());
    return VF_OK;
}

int vf_terrain_set_shadows(vf_terrain *t, int enable, float strength, float softness, float bias)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (!(std::isfinite(strength) && strength >= 0.0f && strength <= 1.0f)) return fail(VF_ERR_INVALID, "strength must be a finite number in [0, 1]");
    if (!(std::isfinite(softness) && softness > 0.0f)) return fail(VF_ERR_INVALID, "softness must be a finite number > 0");
    if (!(std::isfinite(bias) && bias >= 0.0f)) return fail(VF_ERR_INVALID, "bias must be a finite number >= 0");
    if (enable && (t->shard_tiles || t->nranks != 1)) return fail(VF_ERR_INVALID, "shadows need a whole-frame handle: sharded handles are not supported");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    if (enable) { if (int rc = ensure_vis(t)) return rc; }
    vf_terrain::Shadows &H = t->sh;
    if (H.enabled != (enable != 0) || H.strength != strength || H.softness != softness || H.bias != bias) t->inputs_gen++;
    H.enabled = enable != 0; H.strength = strength; H.softness = softness; H.bias = bias;
    return VF_OK;
}

static int viewshed_field(vf_terrain *t, const float *u, hipStream_t s, bool force = false);
static int cumulative_field(vf_terrain *t, const float *u, hipStream_t s, bool force = false);
static int exposure_field(vf_terrain *t, const float *u, hipStream_t s, bool force = false);
static int flood_field(vf_terrain *t, const float *u, hipStream_t s, bool force = false);
static int spill_field(vf_terrain *t, const float *u, hipStream_t s, bool force = false);

// The per-vertex fields a caller can have.  A new one is a feature struct that holds a VertexField, its *_field function and a row here.
enum Field { kFieldLit, kFieldSky, kFieldSeen, kFieldCount, kFieldExposure, kFieldFlood, kFieldSpill, kFields };
struct FieldRow {
    int (*compute)(vf_terrain *, const float *, hipStream_t, bool);   // its *_field function
    VertexField &(*cache)(vf_terrain *);                               // its buffer, key and scan counter
    const char *(*refusal)(const vf_terrain *);                        // why the handle cannot have it now (nullptr: it can); no rule: nullptr
};
static const FieldRow kFieldTable[kFields] = {
    { shadow_field, [](vf_terrain *t) -> VertexField & { return t->sh.lit; }, nullptr },
    { ambient_field, [](vf_terrain *t) -> VertexField & { return t->am.sky; }, nullptr },
    { viewshed_field, [](vf_terrain *t) -> VertexField & { return t->vs.seen; },
      [](const vf_terrain *t) -> const char * { return t->vs.have_observer ? nullptr : "no observer set (vf_terrain_set_viewshed)"; } },
    { cumulative_field, [](vf_terrain *t) -> VertexField & { return t->cv.sum.value; },
      [](const vf_terrain *t) -> const char * { return t->cv.xz.empty() ? "no observers set (vf_terrain_set_cumulative_viewshed)" : nullptr; } },
    { exposure_field, [](vf_terrain *t) -> VertexField & { return t->se.sum.value; },
      [](const vf_terrain *t) -> const char * { return t->se.suns.empty() ? "no suns set (vf_terrain_set_sun_exposure)" : nullptr; } },
    { flood_field, [](vf_terrain *t) -> VertexField & { return t->fd.fill.field; },
      [](const vf_terrain *t) -> const char * { return t->fd.fill.have ? nullptr : "no flood set (vf_terrain_set_flood)"; } },
    { spill_field, [](vf_terrain *t) -> VertexField & { return t->sp.fill.field; },
      [](const vf_terrain *t) -> const char * { return t->sp.fill.have ? nullptr : "no spill set (vf_terrain_set_spill)"; } },
};

// Field f for the live uniforms, heights and parameters, complete in its buffer; then to `host`, or to `dev` behind the work on
// `stream` (NULL: the handle's)
static int field_out(vf_terrain *t, Field f, float *host, float *dev, void *stream)
{
    if (!t || !(host || dev)) return fail(VF_ERR_INVALID, "NULL argument");
    const FieldRow &R = kFieldTable[f];
    if (const char *why = R.refusal ? R.refusal(t) : nullptr) return fail(VF_ERR_INVALID, why);
    if (!t->have_uniforms) return fail(VF_ERR_INVALID, "uniforms not set");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    if (int rc = ct_heights_current(t)) return rc;
    if (int rc = R.compute(t, t->inputs.u, t->ctx->stream, false)) return rc;
    VF_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
    const float *field = R.cache(t).d.p;
    const size_t bytes = (size_t)t->n * t->n * sizeof(float);
    if (host) { VF_HIP_TRY(hipMemcpy(host, field, bytes, hipMemcpyDeviceToHost)); return VF_OK; }
    hipStream_t s = stream ? (hipStream_t)stream : t->ctx->stream;
    VF_HIP_TRY(hipMemcpyAsync(dev, field, bytes, hipMemcpyDeviceToDevice, s));
    VF_HIP_TRY(gb_order_after(t, s));                         // (a later field of this handle is computed behind the copy)
    return VF_OK;
}

static int field_scans(vf_terrain *t, Field f, uint32_t *count)
{
    if (!t || !count) return fail(VF_ERR_INVALID, "NULL argument");
    *count = kFieldTable[f].cache(t).scans;
    return VF_OK;
}

int vf_terrain_read_shadow_field(vf_terrain *t, float *lit) { return field_out(t, kFieldLit, lit, nullptr, nullptr); }
int vf_terrain_shadow_field_device(vf_terrain *t, float *dev_lit, void *stream) { return field_out(t, kFieldLit, nullptr, dev_lit, stream); }
int vf_terrain_debug_shadow_scans(vf_terrain *t, uint32_t *count) { return field_scans(t, kFieldLit, count); }

// Diagnostic launches are not the handle's: the scan counters of every field are handed back as hold() found them, whichever way
// the call returns.
struct ScansHeld {
    vf_terrain *t = nullptr;
    uint32_t scans[kFields] = {};
    void hold(vf_terrain *handle)
    {
        t = handle;
        for (int f = 0; f < kFields; ++f) scans[f] = kFieldTable[f].cache(t).scans;
    }
    ~ScansHeld() { for (int f = 0; t && f < kFields; ++f) kFieldTable[f].cache(t).scans = scans[f]; }
};

// The vf_terrain_debug_*_stage call of a summed field (kFieldCount, kFieldExposure): its computation, forced and timed.  label: whose
// diagnostics these are.
static int summed_stage(vf_terrain *t, Field f, const char *label, uint32_t repeats, float *ms)
{
    if (!t || !ms) return fail(VF_ERR_INVALID, "NULL argument");
    const FieldRow &R = kFieldTable[f];
    if (const char *why = R.refusal(t)) return fail(VF_ERR_INVALID, why);
    if (!t->have_uniforms) return fail(VF_ERR_INVALID, "uniforms not set");
    if (repeats == 0) repeats = 1;
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    if (int rc = ct_heights_current(t)) return rc;
    hipStream_t s = t->ctx->stream;
    ScansHeld held;
    held.hold(t);
    int rc = VF_OK;
    float a = 0.0f;
    const hipError_t err = time_launches(s, repeats, a, [&](bool) { rc = R.compute(t, t->inputs.u, s, true); return rc == VF_OK ? hipSuccess : hipErrorUnknown; });
    if (rc != VF_OK) return rc;
    if (err != hipSuccess) return fail(VF_ERR_HIP, std::string(label) + " diagnostics: " + hipGetErrorString(err));
    *ms = a;
    return VF_OK;
}

// What the stage calls below start from: the frame rendered last, drawn again into scratch buffers with its visibility (gb_frame),
// the uniforms it was drawn with and its `redo` word.
struct RelightStage {
    GbFrame F;
    const float *u = nullptr;
    const uint32_t *redo = nullptr;
    hipStream_t s = nullptr;
    vf_terrain *t = nullptr;
    ScansHeld held;
    int open(vf_terrain *handle)
    {
        if (int rc = gb_frame(handle, F)) return rc;
        t = handle;
        u = (t->have_frame ? t->drawn_inputs : t->inputs).u;
        redo = t->ps[t->last_set].work_count + 3;
        s = t->ctx->stream;
        held.hold(t);
        return VF_OK;
    }
    // the shade pass into the scratch frame (the fields it reads are current), and timed
    void shade(Relight pass) const { relight_launch(t, s, F.P, F.V, redo, t->d_rgba_scratch, pass, t->sh.enabled, t->am.enabled); }
    hipError_t time_shade(uint32_t repeats, float &ms, Relight pass) const
    {
        return time_launches(s, repeats, ms, [&](bool) { shade(pass); return hipGetLastError(); });
    }
    // ms[0]: field() timed, a field computed anyway, which states its own error when it fails; ms[1]: shade() timed, the pass that
    // reads what the field's last launch left.  label: whose diagnostics these are.
    int time_pair(uint32_t repeats, float ms[2], const char *label, const std::function<int()> &field, const std::function<void()> &shade) const
    {
        int rc = VF_OK;
        float a = 0.0f, b = 0.0f;
        hipError_t err = time_launches(s, repeats, a, [&](bool) { rc = field(); return rc == VF_OK ? hipSuccess : hipErrorUnknown; });
        if (err == hipSuccess) err = time_launches(s, repeats, b, [&](bool) { shade(); return hipGetLastError(); });
        if (rc != VF_OK) return rc;
        if (err != hipSuccess) return fail(VF_ERR_HIP, std::string(label) + " diagnostics: " + hipGetErrorString(err));
        ms[0] = a; ms[1] = b;
        return VF_OK;
    }
};

int vf_terrain_debug_shadow_stage(vf_terrain *t, uint32_t repeats, float ms[2])
{
    if (!t || !ms) return fail(VF_ERR_INVALID, "NULL argument");
    if (repeats == 0) repeats = 1;
    RelightStage G;
    if (int rc = G.open(t)) return rc;
    return G.time_pair(repeats, ms, "shadow", [&] { return shadow_field(t, G.u, G.s, true); }, [&] { G.shade(kShadow); });
}

// ---- ambient occlusion (vf_ambient.h) ---------------------------------------------------

// The default set of D directions: azimuth 360 t / D degrees in binary64, rounded; whole octants are the exact axes and (+-1, +-1)
// (vulkan_forge_amd/_ambient.py: directions states the same rule).
static void ambient_default_dirs(uint32_t D, std::vector<float> &dirs)
{
    static const float oct[8][2] = { { 1, 0 }, { 1, 1 }, { 0, 1 }, { -1, 1 }, { -1, 0 }, { -1, -1 }, { 0, -1 }, { 1, -1 } };
    dirs.resize(2u * D);
    for (uint32_t k = 0; k < D; ++k) {
        if ((8u * k) % D == 0u) { dirs[2u * k] = oct[8u * k / D][0]; dirs[2u * k + 1u] = oct[8u * k / D][1]; continue; }
        const double az = 2.0 * 3.14159265358979323846 * (double)k / (double)D;
        dirs[2u * k] = (float)std::cos(az); dirs[2u * k + 1u] = (float)std::sin(az);
    }
}

// The frame of reference of direction (ux, uz) of the field for the uniforms `u`: the lines are
// line_geometry's (set_ambient has refused a direction without a horizontal part).
static void ambient_plan(const vf_terrain *t, const float *u, float ux, float uz, AmbientPlan &A)
{
    ShadowPlan &S = A.S;
    float amaj;
    (void)line_geometry(t, ux, uz, S, amaj);
    S.d = 0.0f; S.exag = u[38]; S.strength = 0.0f; S.softness = 1.0f; S.bias = 0.0f;
    const float g = std::sqrt(std::fma(S.a, S.a, 1.0f));
    A.ell = (grid_step(t) * spacing_of(u)) * g;
    const float rf = std::floor(t->am.reach / g);
    A.R = std::min<uint32_t>(rf >= 1.0f ? (uint32_t)rf : 1u, kAmMaxReach);
}

// `sky` holds the field of the uniforms `u`, the handle's heights, directions and reach once the work queued on `s` is done (the
// height cache must be current and ordered before `s`, as for shadow_field).  force: compute it anyway.
static int ambient_field(vf_terrain *t, const float *u, hipStream_t s, bool force)
{
    vf_terrain::Ambient &H = t->am;
    if (H.default_dirs && H.dirs.size() != 2u * H.ndirs) ambient_default_dirs(H.ndirs, H.dirs);
    std::vector<uint32_t> key = key_of({ spacing_of(u), u[38], H.reach });
    key.push_back((uint32_t)H.dirs.size());
    for (float d : H.dirs) key.push_back(key_bits(d));
    bool current;
    if (int rc = H.sky.prepare(t, key, force, "sky-view field allocation failed", &current)) return rc;
    if (current) return VF_OK;
    for (uint32_t k = 0; k < H.ndirs; ++k) {
        AmbientPlan A;
        ambient_plan(t, u, H.dirs[2u * k], H.dirs[2u * k + 1u], A);
        A.first = k == 0u ? 1u : 0u; A.last = k + 1u == H.ndirs ? 1u : 0u; A.count = (float)H.ndirs;
        const dim3 grid(A.S.nchunks, (A.S.nlines + kShLines - 1u) / kShLines), threads(256);
        if (A.S.zmajor) hipLaunchKernelGGL((k_ambient_dir<true>), grid, threads, 0, s, A, (const float *)t->d_hblk, H.sky.d.p);
        else hipLaunchKernelGGL((k_ambient_dir<false>), grid, threads, 0, s, A, (const float *)t->d_hblk, H.sky.d.p);
    }
    VF_HIP_TRY(hipGetLastError());
    H.sky.computed(t, key);
    return VF_OK;
}

int vf_terrain_set_ambient(vf_terrain *t, int enable, float strength, float reach, uint32_t ndirs, const float *dirs_xz)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (!(std::isfinite(strength) && strength >= 0.0f && strength <= 1.0f)) return fail(VF_ERR_INVALID, "strength must be a finite number in [0, 1]");
    if (!(std::isfinite(reach) && reach >= 1.0f && reach <= (float)VF_AMBIENT_REACH_MAX)) return fail(VF_ERR_INVALID, "reach must be a finite number in [1, 1024]");
    if (ndirs < 1u || ndirs > VF_AMBIENT_DIRECTIONS_MAX) return fail(VF_ERR_INVALID, "ndirs must lie in [1, 64]");
    for (uint32_t k = 0; dirs_xz && k < ndirs; ++k) {
        const float ux = dirs_xz[2u * k], uz = dirs_xz[2u * k + 1u];
        if (!std::isfinite(ux) || !std::isfinite(uz) || (ux == 0.0f && uz == 0.0f)) return fail(VF_ERR_INVALID, "a direction must be finite and have a horizontal part");
    }
    if (enable && (t->shard_tiles || t->nranks != 1)) return fail(VF_ERR_INVALID, "ambient occlusion needs a whole-frame handle: sharded handles are not supported");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    if (enable) { if (int rc = ensure_vis(t)) return rc; }
    vf_terrain::Ambient &H = t->am;
    std::vector<float> dirs;
    if (dirs_xz) dirs.assign(dirs_xz, dirs_xz + 2u * ndirs);
    else ambient_default_dirs(ndirs, dirs);
    if (H.enabled != (enable != 0) || H.strength != strength || H.reach != reach || H.dirs != dirs) t->inputs_gen++;
    H.enabled = enable != 0; H.strength = strength; H.reach = reach; H.ndirs = ndirs; H.default_dirs = dirs_xz == nullptr; H.dirs = std::move(dirs);
    return VF_OK;
}

int vf_terrain_read_sky_view_field(vf_terrain *t, float *sky) { return field_out(t, kFieldSky, sky, nullptr, nullptr); }
int vf_terrain_sky_view_field_device(vf_terrain *t, float *dev_sky, void *stream) { return field_out(t, kFieldSky, nullptr, dev_sky, stream); }
int vf_terrain_debug_ambient_scans(vf_terrain *t, uint32_t *count) { return field_scans(t, kFieldSky, count); }

int vf_terrain_debug_ambient_stage(vf_terrain *t, uint32_t repeats, float ms[2])
{
    if (!t || !ms) return fail(VF_ERR_INVALID, "NULL argument");
    if (repeats == 0) repeats = 1;
    RelightStage G;
    if (int rc = G.open(t)) return rc;
    if (int rc = relight_fields(t, G.u, G.s, t->sh.enabled, false)) return rc;   // (the shade pass below reads it)
    return G.time_pair(repeats, ms, "ambient", [&] { return ambient_field(t, G.u, G.s, true); }, [&] { G.shade(kAmbient); });
}

// ---- the draped image (vf_drape.h) ------------------------------------------------------

// the argument rules of both setters (vulkan_forge_amd/_drape.py states the same); ext: the extent to keep
static int drape_check(const vf_terrain *t, const void *image, uint32_t iw, uint32_t ih, const float *extent, float opacity, int filter, float ext[4])
{
    if (!t || !image) return fail(VF_ERR_INVALID, "NULL argument");
    if (iw < 1u || ih < 1u || iw > VF_DRAPE_SIZE_MAX || ih > VF_DRAPE_SIZE_MAX) return fail(VF_ERR_INVALID, "image width and height must lie in [1, 16384]");
    const float whole[4] = { -1.5f, -1.5f, 1.5f, 1.5f };
    std::memcpy(ext, extent ? extent : whole, sizeof whole);
    for (int k = 0; k < 4; ++k) if (!std::isfinite(ext[k])) return fail(VF_ERR_INVALID, "extent must be finite");
    if (!(ext[2] > ext[0]) || !(ext[3] > ext[1])) return fail(VF_ERR_INVALID, "extent (x0, z0, x1, z1) needs x1 > x0 and z1 > z0");
    if (!(std::isfinite(opacity) && opacity >= 0.0f && opacity <= 1.0f)) return fail(VF_ERR_INVALID, "opacity must be a finite number in [0, 1]");
    if (filter != VF_DRAPE_NEAREST && filter != VF_DRAPE_LINEAR) return fail(VF_ERR_INVALID, "filter must be VF_DRAPE_NEAREST or VF_DRAPE_LINEAR");
    if (t->shard_tiles || t->nranks != 1) return fail(VF_ERR_INVALID, "a draped image needs a whole-frame handle: sharded handles are not supported");
    return VF_OK;
}

// what a drape needs beside its image (nothing is changed when this fails); the caller has waited for the frame in flight
static int drape_buffers(vf_terrain *t, size_t texels)
{
    if (int rc = ensure_vis(t)) return rc;
    vf_terrain::Drape &H = t->dr;
    if (H.d_img.reserve(texels, texels) != hipSuccess) { (void)hipGetLastError(); return fail(VF_ERR_NOMEM, "drape image allocation failed"); }
    return VF_OK;
}

static void drape_commit(vf_terrain *t, uint32_t iw, uint32_t ih, const float ext[4], float opacity, int filter)
{
    vf_terrain::Drape &H = t->dr;
    H.iw = iw; H.ih = ih; H.opacity = opacity; H.filter = filter;
    std::memcpy(H.extent, ext, sizeof H.extent);
    t->dm.stale = true;                                      // (a new image: its pyramid is built by the first frame that wants it, into the buffer held if the size is the old one)
    t->inputs_gen++;
}

int vf_terrain_set_drape(vf_terrain *t, const uint8_t *rgba, uint32_t iw, uint32_t ih, uint32_t channels, const float extent[4], float opacity, int filter)
{
    float ext[4];
    if (int rc = drape_check(t, rgba, iw, ih, extent, opacity, filter, ext)) return rc;
    if (channels != 3u && channels != 4u) return fail(VF_ERR_INVALID, "channels must be 3 or 4");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));                                // (the frame in flight reads the image this call replaces)
    if (t->dr.copied) VF_HIP_TRY(hipEventSynchronize(t->dr.copied));   // (and so does an earlier device copy, on a stream of the caller's)
    const size_t texels = (size_t)iw * ih;
    DevBuf<uint8_t> rgb;                                      // an RGB upload's bytes: expanded on the device, then freed
    if (channels == 3u && rgb.reserve(texels * 3u, texels * 3u) != hipSuccess) { (void)hipGetLastError(); return fail(VF_ERR_NOMEM, "drape upload allocation failed"); }
    if (int rc = drape_buffers(t, texels)) { rgb.release(); return rc; }
    hipStream_t s = t->ctx->stream;
    hipError_t err;
    if (channels == 3u) {
        err = hipMemcpyAsync(rgb.p, rgba, texels * 3u, hipMemcpyHostToDevice, s);
        if (err == hipSuccess) {
            hipLaunchKernelGGL((k_drape_expand<0>), dim3((uint32_t)((texels + 255u) / 256u)), dim3(256), 0, s, texels, (const uint8_t *)rgb.p, t->dr.d_img.p);
            err = hipGetLastError();
        }
    }
    else err = hipMemcpyAsync(t->dr.d_img.p, rgba, texels * 4u, hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);     // (a snapshot: the caller's array is free when this returns)
    rgb.release();
    if (err != hipSuccess) { drape_release(t); return fail(VF_ERR_HIP, std::string("drape upload: ") + hipGetErrorString(err)); }
    if (t->dr.copied) { (void)hipEventDestroy(t->dr.copied); t->dr.copied = nullptr; }
    drape_commit(t, iw, ih, ext, opacity, filter);
    return VF_OK;
}

int vf_terrain_set_drape_device(vf_terrain *t, const void *dev_rgba, uint32_t iw, uint32_t ih, const float extent[4], float opacity, int filter, void *stream)
{
    float ext[4];
    if (int rc = drape_check(t, dev_rgba, iw, ih, extent, opacity, filter, ext)) return rc;
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    if (t->dr.copied) VF_HIP_TRY(hipEventSynchronize(t->dr.copied));
    const size_t texels = (size_t)iw * ih;
    if (int rc = drape_buffers(t, texels)) return rc;
    if (!t->dr.copied) VF_HIP_TRY(hipEventCreateWithFlags(&t->dr.copied, hipEventDisableTiming));
    hipStream_t s = stream ? (hipStream_t)stream : t->ctx->stream;
    hipError_t err = hipMemcpyAsync(t->dr.d_img.p, dev_rgba, texels * 4u, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess) err = hipEventRecord(t->dr.copied, s);
    if (err != hipSuccess) { drape_release(t); return fail(VF_ERR_HIP, std::string("drape copy: ") + hipGetErrorString(err)); }
    drape_commit(t, iw, ih, ext, opacity, filter);
    return VF_OK;
}

int vf_terrain_clear_drape(vf_terrain *t)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->dr.iw && !t->dr.d_img.p) return VF_OK;
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    if (t->dr.copied) VF_HIP_TRY(hipEventSynchronize(t->dr.copied));
    drape_release(t);
    t->inputs_gen++;
    return VF_OK;
}

int vf_terrain_drape_info(const vf_terrain *t, uint32_t *iw, uint32_t *ih, float extent[4], float *opacity, int *filter)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    const vf_terrain::Drape &H = t->dr;
    if (iw) *iw = H.iw;
    if (!H.iw) return VF_OK;
    if (ih) *ih = H.ih;
    if (extent) std::memcpy(extent, H.extent, sizeof H.extent);
    if (opacity) *opacity = H.opacity;
    if (filter) *filter = H.filter;
    return VF_OK;
}

int vf_terrain_debug_drape_stage(vf_terrain *t, uint32_t repeats, float *ms)
{
    if (!t || !ms) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->dr.iw) return fail(VF_ERR_INVALID, "the handle holds no draped image");
    if (repeats == 0) repeats = 1;
    RelightStage G;
    if (int rc = G.open(t)) return rc;
    if (int rc = relight_fields(t, G.u, G.s, t->sh.enabled, t->am.enabled)) return rc;   // (the shade pass below reads them)
    if (t->dr.copied) VF_HIP_TRY(hipStreamWaitEvent(G.s, t->dr.copied, 0));
    if (int rc = mips_current(t, G.s)) return rc;            // (whichever drape pass the handle would run)
    float mean = 0.0f;
    const hipError_t err = G.time_shade(repeats, mean, drape_pass_of(t));
    if (err != hipSuccess) return fail(VF_ERR_HIP, std::string("drape diagnostics: ") + hipGetErrorString(err));
    *ms = mean;
    return VF_OK;
}

// ---- its mip pyramid (vf_drape_mips.h) ---------------------------------------------------

int vf_terrain_set_drape_mips(vf_terrain *t, int enabled, float bias)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (!(std::isfinite(bias) && bias >= -VF_DRAPE_MIP_BIAS_MAX && bias <= VF_DRAPE_MIP_BIAS_MAX)) return fail(VF_ERR_INVALID, "bias must be a finite number in [-16, 16]");
    vf_terrain::DrapeMipState &M = t->dm;
    if (M.enabled == (enabled != 0) && M.bias == bias) return VF_OK;
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));                                // (the frame in flight reads the pyramid this call may free)
    if (!enabled) { M.d_pyr.release(); M.stale = true; }
    M.enabled = enabled != 0; M.bias = bias;
    t->inputs_gen++;
    return VF_OK;
}

int vf_terrain_drape_mip_info(const vf_terrain *t, int *enabled, uint32_t *levels, float *bias, uint64_t *bytes, uint32_t *builds)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    const vf_terrain::DrapeMipState &M = t->dm;
    const bool held = M.enabled && t->dr.iw != 0u;
    const MipLayout L = held ? mip_layout(t->dr.iw, t->dr.ih) : MipLayout();
    if (enabled) *enabled = M.enabled ? 1 : 0;
    if (levels) *levels = held ? L.levels : 0u;
    if (bias) *bias = M.bias;
    if (bytes) *bytes = (uint64_t)L.texels * sizeof(uint2);
    if (builds) *builds = M.builds;
    return VF_OK;
}

// ---- and anisotropic taps through it (vf_drape_aniso.h) -----------------------------------
// The setting reads nothing the frame in flight holds and leaves the pyramid as it is: the next frame is drawn again, that is all.

int vf_terrain_set_drape_anisotropy(vf_terrain *t, uint32_t max_anisotropy)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    const uint32_t a = max_anisotropy;
    if (!(a == 1u || a == 2u || a == 4u || a == 8u || a == VF_DRAPE_ANISOTROPY_MAX)) return fail(VF_ERR_INVALID, "max_anisotropy must be 1, 2, 4, 8 or 16");
    if (t->dm.aniso == a) return VF_OK;
    t->dm.aniso = a;
    t->inputs_gen++;
    return VF_OK;
}

int vf_terrain_drape_anisotropy(const vf_terrain *t, uint32_t *max_anisotropy)
{
    if (!t || !max_anisotropy) return fail(VF_ERR_INVALID, "NULL argument");
    *max_anisotropy = t->dm.aniso;
    return VF_OK;
}

int vf_terrain_read_drape_level(vf_terrain *t, uint32_t level, uint16_t *out, uint32_t *w, uint32_t *h)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->dm.enabled || !t->dr.iw) return fail(VF_ERR_INVALID, "no mip pyramid: it needs a draped image and mipmaps enabled");
    const MipLayout L = mip_layout(t->dr.iw, t->dr.ih);
    if (level < 1u || level >= L.levels) return fail(VF_ERR_INVALID, "level must lie in [1, levels)");
    if (w) *w = L.w[level];
    if (h) *h = L.h[level];
    if (!out) return VF_OK;
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    // The frame in flight may have been drawn on a stream of the caller's, and the build with it: the copy below, on the context's
    // stream, is ordered against neither by itself.  So the frame is waited for first, always: the copy then reads a complete
    // pyramid, and a build queued here does not overtake a frame that still reads the image.
    VF_HIP_TRY(wait_frame(t));
    hipStream_t s = t->ctx->stream;
    if (t->dr.copied) VF_HIP_TRY(hipStreamWaitEvent(s, t->dr.copied, 0));
    if (int rc = mips_current(t, s)) return rc;
    VF_HIP_TRY(hipMemcpyAsync(out, t->dm.d_pyr.p + L.off[level], (size_t)L.w[level] * L.h[level] * sizeof(uint2), hipMemcpyDeviceToHost, s));
    VF_HIP_TRY(hipStreamSynchronize(s));
    return VF_OK;
}

int vf_terrain_debug_drape_mip_build(vf_terrain *t, uint32_t repeats, float *ms)
{
    if (!t || !ms) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->dm.enabled || !t->dr.iw) return fail(VF_ERR_INVALID, "no mip pyramid: it needs a draped image and mipmaps enabled");
    if (repeats == 0) repeats = 1;
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    hipStream_t s = t->ctx->stream;
    if (t->dr.copied) VF_HIP_TRY(hipStreamWaitEvent(s, t->dr.copied, 0));
    if (int rc = mips_current(t, s)) return rc;              // (the handle's own build, if it was due; the timed ones below touch no state)
    const MipLayout L = mip_layout(t->dr.iw, t->dr.ih);
    float mean = 0.0f;
    const hipError_t err = L.levels < 2u ? hipSuccess : time_launches(s, repeats, mean, [&](bool) { mips_launch(t, s, L); return hipGetLastError(); });
    if (err != hipSuccess) return fail(VF_ERR_HIP, std::string("drape mip diagnostics: ") + hipGetErrorString(err));
    *ms = mean;
    return VF_OK;
}

// ---- viewshed analysis (vf_viewshed.h) --------------------------------------------------

// The observer's vertex on one axis from its world coordinate: the drape's grid coordinate (4b step 1), rounded
static uint32_t viewshed_index(const vf_terrain *t, float x, float spacing)
{
    float mx = x / spacing;
    mx = std::fmin(std::fmax(mx, -1.5f), 1.5f);
    const float gx = (mx + 1.5f) / grid_step(t);
    return std::min((uint32_t)std::rint(gx), t->n - 1u);
}

// The frame of reference of the field for the uniforms `u`
static void viewshed_plan(const vf_terrain *t, const float *u, ViewshedPlan &S)
{
    const vf_terrain::Viewshed &H = t->vs;
    const float spacing = spacing_of(u);
    S.n = t->n; S.nb = t->nb;
    S.io = viewshed_index(t, H.ox, spacing); S.jo = viewshed_index(t, H.oz, spacing);
    S.L = t->n - 1u;
    S.nlines = 2u * S.L + 1u; S.nchunks = (S.L + kShChunk - 1u) / kShChunk;
    S.steps[0] = t->n - 1u - S.io; S.steps[1] = S.io; S.steps[2] = t->n - 1u - S.jo; S.steps[3] = S.jo;
    S.exag = u[38]; S.eye_height = H.eye_height; S.target_height = H.target_height; S.softness = H.softness; S.bias = H.bias;
}

// `seen` holds the field of the uniforms `u`, the handle's heights, observer and scan parameters once the work queued on `s` is done
// (the height cache must be current and ordered before `s`, as for shadow_field).  force: compute it anyway.
static int viewshed_field(vf_terrain *t, const float *u, hipStream_t s, bool force)
{
    vf_terrain::Viewshed &H = t->vs;
    if (!H.have_observer) return fail(VF_ERR_INVALID, "no observer set (vf_terrain_set_viewshed)");
    ViewshedPlan S;
    viewshed_plan(t, u, S);
    std::vector<uint32_t> key = key_of({ S.exag, S.eye_height, S.target_height, S.softness, S.bias });
    key.push_back(S.io); key.push_back(S.jo);
    bool current;
    if (int rc = H.seen.prepare(t, key, force, "viewshed field allocation failed", &current)) return rc;
    if (current) return VF_OK;
    const size_t ncmax = (size_t)4u * S.nchunks * S.nlines;
    if (H.d_cmax.reserve(ncmax, ncmax) != hipSuccess) { (void)hipGetLastError(); return fail(VF_ERR_NOMEM, "viewshed scan allocation failed"); }
    // (the x-major quadrants in one launch, the z-major ones in another: a quadrant's chunks beyond its steps leave at once)
    const uint32_t cx = (std::max(S.steps[0], S.steps[1]) + kShChunk - 1u) / kShChunk, cz = (std::max(S.steps[2], S.steps[3]) + kShChunk - 1u) / kShChunk;
    const uint32_t groups = (S.nlines + kShLines - 1u) / kShLines;
    const dim3 gx(cx, groups, 2), gz(cz, groups, 2), threads(256);
    hipLaunchKernelGGL((k_viewshed_chunk_max<false>), gx, threads, 0, s, S, (const float *)t->d_hblk, H.d_cmax.p);
    hipLaunchKernelGGL((k_viewshed_chunk_max<true>), gz, threads, 0, s, S, (const float *)t->d_hblk, H.d_cmax.p);
    hipLaunchKernelGGL((k_viewshed_carry<0>), dim3((S.nlines + 255u) / 256u, 4), threads, 0, s, S, H.d_cmax.p);
    hipLaunchKernelGGL((k_viewshed_seen<false>), gx, threads, 0, s, S, (const float *)t->d_hblk, (const float *)H.d_cmax.p, H.seen.d.p);
    hipLaunchKernelGGL((k_viewshed_seen<true>), gz, threads, 0, s, S, (const float *)t->d_hblk, (const float *)H.d_cmax.p, H.seen.d.p);
    VF_HIP_TRY(hipGetLastError());
    H.seen.computed(t, key);
    return VF_OK;
}

} // extern "C"   (a template has C++ linkage)
// Both instantiations of a tint kernel (k_viewshed_tint, k_flood_tint, k_spill_tint) with its parameters T, in k_resolve's launch shape (gb_grid)
template <typename Tint> using TintKernel = void(FrameParams, SetupView, const float *, const uint32_t *, Tint, const uint32_t *, uint32_t *);
template <typename Tint> static void tint_launch(const vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba,
                                                 const Tint &T, TintKernel<Tint> *whole, TintKernel<Tint> *clipped)
{
    const dim3 grid = gb_grid(t), threads(256);
    hipLaunchKernelGGL(whole, grid, threads, 0, s, P, V, (const float *)t->ctx->d_thresh, (const uint32_t *)t->d_vis, T, redo, rgba);
    hipLaunchKernelGGL(clipped, grid, threads, 0, s, P, V, (const float *)t->ctx->d_thresh, (const uint32_t *)t->d_vis, T, redo, rgba);
}
extern "C" {

static void viewshed_launch(const vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba)
{
    const vf_terrain::Viewshed &H = t->vs;
    ViewshedTint T = {};
    T.seen = H.seen.d.p; T.decode = t->ctx->d_decode;
    T.visible_rgba = H.visible_rgba; T.hidden_rgba = H.hidden_rgba;
    const float step = grid_step(t);   // (P.step, as the vertex stage forms the grid coordinates)
    T.xo = -1.5f + (float)viewshed_index(t, H.ox, P.spacing) * step; T.zo = -1.5f + (float)viewshed_index(t, H.oz, P.spacing) * step;
    const float R = H.radius / P.spacing;
    T.RR = R * R; T.radius_on = H.radius > 0.0f ? 1u : 0u;
    tint_launch(t, s, P, V, redo, rgba, T, k_viewshed_tint<false>, k_viewshed_tint<true>);
}

// The tint of a frame, on the draw stream behind its tile kernels (which stored the visibility) and the relight passes: the field
// if it is stale, then the tint pass over the covered pixels
static int viewshed_pass(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba)
{
    if (int rc = viewshed_field(t, t->inputs.u, s)) return rc;
    viewshed_launch(t, s, P, V, redo, rgba);
    VF_HIP_TRY(hipGetLastError());
    return VF_OK;
}

// the scan parameters of both viewshed setters
static int viewshed_params_check(float eye_height, float target_height, float radius, float softness, float bias)
{
    if (!(std::isfinite(eye_height) && eye_height >= 0.0f)) return fail(VF_ERR_INVALID, "eye_height must be a finite number >= 0");
    if (!(std::isfinite(target_height) && target_height >= 0.0f)) return fail(VF_ERR_INVALID, "target_height must be a finite number >= 0");
    if (!(std::isfinite(radius) && radius >= 0.0f)) return fail(VF_ERR_INVALID, "radius must be a finite number > 0, or 0 for none");
    if (!(std::isfinite(softness) && softness > 0.0f)) return fail(VF_ERR_INVALID, "softness must be a finite number > 0");
    if (!(std::isfinite(bias) && bias >= 0.0f)) return fail(VF_ERR_INVALID, "bias must be a finite number >= 0");
    return VF_OK;
}

int vf_terrain_set_viewshed(vf_terrain *t, int enable, const float observer_xz[2], float eye_height, float target_height, float radius,
                            const uint8_t visible_rgba[4], const uint8_t hidden_rgba[4], float softness, float bias)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    vf_terrain::Viewshed &H = t->vs;
    if (!observer_xz) {                                        // forget the observer: off, and everything made for it is freed
        if (enable) return fail(VF_ERR_INVALID, "a viewshed needs an observer");
        VF_HIP_TRY(hipSetDevice(t->ctx->device));
        VF_HIP_TRY(wait_frame(t));
        if (H.enabled) t->inputs_gen++;
        viewshed_release(t);
        return VF_OK;
    }
    if (!visible_rgba || !hidden_rgba) return fail(VF_ERR_INVALID, "NULL argument");
    if (!(std::isfinite(observer_xz[0]) && std::isfinite(observer_xz[1]))) return fail(VF_ERR_INVALID, "the observer must be finite");
    if (int rc = viewshed_params_check(eye_height, target_height, radius, softness, bias)) return rc;
    if (enable && (t->shard_tiles || t->nranks != 1)) return fail(VF_ERR_INVALID, "a viewshed needs a whole-frame handle: sharded handles are not supported");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    if (enable) {
        if (int rc = ensure_vis(t)) return rc;
        H.tinted = true;
    }
    const uint32_t vis = pack_rgba8(visible_rgba), hid = pack_rgba8(hidden_rgba);
    if (H.enabled != (enable != 0) || !H.have_observer || H.ox != observer_xz[0] || H.oz != observer_xz[1] || H.eye_height != eye_height
        || H.target_height != target_height || H.radius != radius || H.softness != softness || H.bias != bias || H.visible_rgba != vis || H.hidden_rgba != hid)
        t->inputs_gen++;
    H.enabled = enable != 0; H.have_observer = true;
    H.ox = observer_xz[0]; H.oz = observer_xz[1];
    H.eye_height = eye_height; H.target_height = target_height; H.radius = radius; H.softness = softness; H.bias = bias;
    H.visible_rgba = vis; H.hidden_rgba = hid;
    return VF_OK;
}

int vf_terrain_read_viewshed_field(vf_terrain *t, float *seen) { return field_out(t, kFieldSeen, seen, nullptr, nullptr); }
int vf_terrain_viewshed_field_device(vf_terrain *t, float *dev_seen, void *stream) { return field_out(t, kFieldSeen, nullptr, dev_seen, stream); }

int vf_terrain_viewshed_info(vf_terrain *t, vf_viewshed_info *out)
{
    if (!t || !out) return fail(VF_ERR_INVALID, "NULL argument");
    const vf_terrain::Viewshed &H = t->vs;
    *out = vf_viewshed_info();
    out->enabled = H.enabled ? 1 : 0; out->has_observer = H.have_observer ? 1 : 0;
    out->eye_height = H.eye_height; out->target_height = H.target_height; out->radius = H.radius; out->softness = H.softness; out->bias = H.bias;
    for (int k = 0; k < 4; ++k) { out->visible_rgba[k] = (uint8_t)(H.visible_rgba >> (8 * k)); out->hidden_rgba[k] = (uint8_t)(H.hidden_rgba >> (8 * k)); }
    if (!H.have_observer) return VF_OK;
    if (!t->have_uniforms) return fail(VF_ERR_INVALID, "uniforms not set");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    if (int rc = ct_heights_current(t)) return rc;
    ViewshedPlan S;
    viewshed_plan(t, t->inputs.u, S);
    const uint32_t bx = std::min(S.io >> 3, t->nb - 1u), by = std::min(S.jo >> 3, t->nb - 1u);   // (cached_height's place)
    float h = 0.0f;
    VF_HIP_TRY(hipMemcpyAsync(&h, t->d_hblk + (size_t)(by * t->nb + bx) * kBlockStride + (S.jo - 8u * by) * 9u + (S.io - 8u * bx), sizeof h,
                              hipMemcpyDeviceToHost, t->ctx->stream));
    VF_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
    const float spacing = spacing_of(t->inputs.u), step = grid_step(t);
    out->vertex[0] = S.io; out->vertex[1] = S.jo;
    out->observer_xyz[0] = (-1.5f + (float)S.io * step) * spacing;
    out->observer_xyz[1] = h * S.exag;
    out->observer_xyz[2] = (-1.5f + (float)S.jo * step) * spacing;
    out->eye_y = out->observer_xyz[1] + H.eye_height;
    return VF_OK;
}

int vf_terrain_debug_viewshed_scans(vf_terrain *t, uint32_t *count) { return field_scans(t, kFieldSeen, count); }

int vf_terrain_debug_viewshed_stage(vf_terrain *t, uint32_t repeats, float ms[2])
{
    if (!t || !ms) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->vs.have_observer || !t->vs.tinted) return fail(VF_ERR_INVALID, "no viewshed: it needs an observer, and to have been enabled once");
    if (repeats == 0) repeats = 1;
    RelightStage G;
    if (int rc = G.open(t)) return rc;
    return G.time_pair(repeats, ms, "viewshed", [&] { return viewshed_field(t, G.u, G.s, true); },
                       [&] { viewshed_launch(t, G.s, G.F.P, G.F.V, G.redo, t->d_rgba_scratch); });
}

// ---- summed fields: what cumulative viewsheds and sun exposure share ---------------

int SummedField::reserve(const vf_terrain *t, const char *nomem)
{
    const size_t nv = (size_t)t->n * t->n;
    if (d_sum.reserve(nv, nv) != hipSuccess || d_frac.reserve(nv, nv) != hipSuccess) { (void)hipGetLastError(); return fail(VF_ERR_NOMEM, nomem); }
    return VF_OK;
}

hipError_t SummedField::zero(const vf_terrain *t, hipStream_t s) { return hipMemsetAsync(d_sum.p, 0, (size_t)t->n * t->n * sizeof(uint32_t), s); }

int SummedField::finish(const vf_terrain *t, hipStream_t s, float total, std::vector<uint32_t> &key, uint32_t B)
{
    const size_t nv = (size_t)t->n * t->n;
    hipLaunchKernelGGL((k_sum_finish<0>), dim3((uint32_t)((nv + 255u) / 256u)), dim3(256), 0, s, (const uint32_t *)d_sum.p, (uint32_t)nv, total, value.d.p, d_frac.p);
    VF_HIP_TRY(hipGetLastError());
    value.computed(t, key);
    batch = B;
    return VF_OK;
}

int SummedField::tint(const vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba) const
{
    ViewshedTint T = {};                                       // (no radius: every covered pixel is treated)
    T.seen = d_frac.p; T.decode = t->ctx->d_decode;
    T.visible_rgba = high_rgba; T.hidden_rgba = low_rgba;
    tint_launch(t, s, P, V, redo, rgba, T, k_viewshed_tint<false>, k_viewshed_tint<true>);
    VF_HIP_TRY(hipGetLastError());
    return VF_OK;
}

// ---- cumulative viewsheds (vf_cumulative_viewshed.h) ------------------------------------

// The carries of a batch may take this many floats (32 MiB).  Not more: every observer of a batch reads the one height cache, and
// at grid 4096 carries of 134 MB and more push it out of the last-level cache between the stages (4 observers per
// launch there take 28 ms for 64 observers, 32 take 38 ms); at smaller grids the batch is still 64 observers and more.
constexpr size_t kCvCarryFloats = (size_t)8u << 20;
constexpr uint32_t kCvMaxBatch = 4096;                        // (the carry stage's grid holds four blocks rows per observer: 4 B <= 65535)

// Rc = radius / (spacing step) of the uniforms `u`; only with a radius
static float cumulative_rc(const vf_terrain *t, const float *u)
{
    const float spacing = spacing_of(u), step = grid_step(t);
    return t->cv.radius / (spacing * step);
}

// the steps of a line that can lie within Rc: min(L, ceil(Rc)), at least 1
static uint32_t cumulative_reach(const vf_terrain *t, float Rc)
{
    const uint32_t L = t->n - 1u;
    if (!(Rc < (float)L)) return L;
    return std::max(1u, (uint32_t)std::ceil(Rc));
}

// observers per launch: as many as the budget for the carries holds
static uint32_t cumulative_batch(const vf_terrain *t, uint32_t N, uint32_t nchunks)
{
    const size_t per = (size_t)4u * nchunks * (2u * (t->n - 1u) + 1u);
    const size_t B = t->cv.sum.forced_batch ? t->cv.sum.forced_batch : std::max<size_t>(kCvCarryFloats / per, 1u);
    return (uint32_t)std::min<size_t>(std::min<size_t>(B, kCvMaxBatch), N);
}

// `sum` holds the field of the uniforms `u`, the handle's heights, observers and scan parameters once the work queued on `s` is done
// (the height cache must be current and ordered before `s`).  force: compute it anyway.
static int cumulative_field(vf_terrain *t, const float *u, hipStream_t s, bool force)
{
    vf_terrain::CumulativeViewshed &H = t->cv;
    const uint32_t N = (uint32_t)(H.xz.size() / 2u);
    if (!N) return fail(VF_ERR_INVALID, "no observers set (vf_terrain_set_cumulative_viewshed)");
    const char *nomem = "cumulative viewshed field allocation failed";
    if (int rc = H.sum.reserve(t, nomem)) return rc;
    const float spacing = spacing_of(u);
    const bool ranged = H.radius > 0.0f;
    const float Rc = ranged ? cumulative_rc(t, u) : 0.0f;
    const uint32_t L = t->n - 1u, reach = ranged ? cumulative_reach(t, Rc) : L;
    std::vector<uint32_t> ij((size_t)2u * N);
    for (uint32_t o = 0; o < N; ++o) {
        ij[2u * o] = viewshed_index(t, H.xz[2u * o], spacing);
        ij[2u * o + 1u] = viewshed_index(t, H.xz[2u * o + 1u], spacing);
    }
    std::vector<uint32_t> key = key_of({ u[38], H.eye_height, H.target_height, H.softness, H.bias, ranged ? Rc : -1.0f });
    key.push_back((uint32_t)ij.size());
    key.insert(key.end(), ij.begin(), ij.end());
    bool current;
    if (int rc = H.sum.value.prepare(t, key, force, nomem, &current)) return rc;
    if (current) return VF_OK;
    const uint32_t nlines = 2u * L + 1u, nchunks = (reach + kShChunk - 1u) / kShChunk;
    const uint32_t B = cumulative_batch(t, N, nchunks);
    const size_t ncmax = (size_t)B * 4u * nchunks * nlines;
    if (H.d_cmax.reserve(ncmax, ncmax) != hipSuccess || H.d_plans.reserve(N, N) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VF_ERR_NOMEM, "cumulative viewshed scan allocation failed");
    }
    H.plans.resize(N);
    for (uint32_t o = 0; o < N; ++o) {                         // viewshed_plan's frame of reference, cut at the range
        ViewshedPlan &S = H.plans[o];
        S.n = t->n; S.nb = t->nb;
        S.io = ij[2u * o]; S.jo = ij[2u * o + 1u];
        S.L = L; S.nlines = nlines; S.nchunks = nchunks;
        S.steps[0] = std::min(L - S.io, reach); S.steps[1] = std::min(S.io, reach);
        S.steps[2] = std::min(L - S.jo, reach); S.steps[3] = std::min(S.jo, reach);
        S.exag = u[38]; S.eye_height = H.eye_height; S.target_height = H.target_height; S.softness = H.softness; S.bias = H.bias;
    }
    VF_HIP_TRY(hipMemcpyAsync(H.d_plans.p, H.plans.data(), (size_t)N * sizeof(ViewshedPlan), hipMemcpyHostToDevice, s));   // (pageable source: returns when the copy is staged)
    VF_HIP_TRY(H.sum.zero(t, s));
    const float RR = Rc * Rc;
    const uint32_t groups = (nlines + kShLines - 1u) / kShLines;
    const dim3 threads(256);
    for (uint32_t b0 = 0; b0 < N; b0 += B) {                   // five launches per batch; the batches share the carries, in stream order
        const uint32_t nb = std::min(B, N - b0);
        uint32_t sx = 0, sz = 0;
        for (uint32_t o = b0; o < b0 + nb; ++o) {
            sx = std::max(sx, std::max(H.plans[o].steps[0], H.plans[o].steps[1]));
            sz = std::max(sz, std::max(H.plans[o].steps[2], H.plans[o].steps[3]));
        }
        // (a quadrant's chunks beyond its steps leave at once)
        const dim3 gx((sx + kShChunk - 1u) / kShChunk, groups, 2u * nb), gz((sz + kShChunk - 1u) / kShChunk, groups, 2u * nb);
        const ViewshedPlan *plans = H.d_plans.p + b0;
        if (gx.x) hipLaunchKernelGGL((k_cumulative_chunk_max<false>), gx, threads, 0, s, plans, (const float *)t->d_hblk, H.d_cmax.p);
        if (gz.x) hipLaunchKernelGGL((k_cumulative_chunk_max<true>), gz, threads, 0, s, plans, (const float *)t->d_hblk, H.d_cmax.p);
        hipLaunchKernelGGL((k_cumulative_carry<0>), dim3((nlines + 255u) / 256u, 4u * nb), threads, 0, s, plans, H.d_cmax.p);
        // (with no x-major chunk the observer's own vertex would go without its 1: n >= 2 gives every observer a step on both axes)
        if (gx.x) hipLaunchKernelGGL((k_cumulative_seen<false>), gx, threads, 0, s, plans, (const float *)t->d_hblk, (const float *)H.d_cmax.p, RR, ranged ? 1u : 0u, H.sum.d_sum.p);
        if (gz.x) hipLaunchKernelGGL((k_cumulative_seen<true>), gz, threads, 0, s, plans, (const float *)t->d_hblk, (const float *)H.d_cmax.p, RR, ranged ? 1u : 0u, H.sum.d_sum.p);
    }
    return H.sum.finish(t, s, (float)N, key, B);
}

// The cumulative viewshed's tint of a frame: the field if it is stale, then k_viewshed_tint on f = count / N
static int cumulative_pass(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba)
{
    if (int rc = cumulative_field(t, t->inputs.u, s)) return rc;
    return t->cv.sum.tint(t, s, P, V, redo, rgba);
}

int vf_terrain_set_cumulative_viewshed(vf_terrain *t, int enable, const float *observers_xz, uint32_t count, float eye_height, float target_height,
                                       float radius, const uint8_t high_rgba[4], const uint8_t low_rgba[4], float softness, float bias)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    vf_terrain::CumulativeViewshed &H = t->cv;
    if (!observers_xz) {                                       // forget the observers: off, and everything made for them is freed
        if (enable) return fail(VF_ERR_INVALID, "a cumulative viewshed needs observers");
        VF_HIP_TRY(hipSetDevice(t->ctx->device));
        VF_HIP_TRY(wait_frame(t));
        if (H.enabled) t->inputs_gen++;
        cumulative_release(t);
        return VF_OK;
    }
    if (!high_rgba || !low_rgba) return fail(VF_ERR_INVALID, "NULL argument");
    if (count < 1u || count > VF_CUMULATIVE_VIEWSHED_MAX_OBSERVERS) return fail(VF_ERR_INVALID, "a cumulative viewshed takes 1 to 65535 observers");
    for (size_t k = 0; k < (size_t)2u * count; ++k)
        if (!std::isfinite(observers_xz[k])) return fail(VF_ERR_INVALID, "the observers must be finite");
    if (int rc = viewshed_params_check(eye_height, target_height, radius, softness, bias)) return rc;
    if (enable && (t->shard_tiles || t->nranks != 1)) return fail(VF_ERR_INVALID, "a cumulative viewshed needs a whole-frame handle: sharded handles are not supported");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    if (enable) { if (int rc = ensure_vis(t)) return rc; }
    const uint32_t hi = pack_rgba8(high_rgba), lo = pack_rgba8(low_rgba);
    std::vector<float> xz(observers_xz, observers_xz + (size_t)2u * count);
    if (H.enabled != (enable != 0) || H.xz != xz || H.eye_height != eye_height || H.target_height != target_height || H.radius != radius
        || H.softness != softness || H.bias != bias || H.sum.high_rgba != hi || H.sum.low_rgba != lo)
        t->inputs_gen++;
    H.enabled = enable != 0;
    H.xz.swap(xz);
    H.eye_height = eye_height; H.target_height = target_height; H.radius = radius; H.softness = softness; H.bias = bias;
    H.sum.high_rgba = hi; H.sum.low_rgba = lo;
    return VF_OK;
}

int vf_terrain_read_cumulative_viewshed_field(vf_terrain *t, float *count) { return field_out(t, kFieldCount, count, nullptr, nullptr); }
int vf_terrain_cumulative_viewshed_field_device(vf_terrain *t, float *dev_count, void *stream) { return field_out(t, kFieldCount, nullptr, dev_count, stream); }

int vf_terrain_cumulative_viewshed_info(vf_terrain *t, vf_cumulative_viewshed_info *out)
{
    if (!t || !out) return fail(VF_ERR_INVALID, "NULL argument");
    const vf_terrain::CumulativeViewshed &H = t->cv;
    *out = vf_cumulative_viewshed_info();
    out->enabled = H.enabled ? 1 : 0; out->count = (uint32_t)(H.xz.size() / 2u); out->batch = H.sum.batch;
    out->eye_height = H.eye_height; out->target_height = H.target_height; out->radius = H.radius; out->softness = H.softness; out->bias = H.bias;
    H.sum.colours(out->high_rgba, out->low_rgba);
    return VF_OK;
}

int vf_terrain_read_cumulative_viewshed_vertices(vf_terrain *t, uint32_t *vertices)
{
    if (!t || !vertices) return fail(VF_ERR_INVALID, "NULL argument");
    const vf_terrain::CumulativeViewshed &H = t->cv;
    if (H.xz.empty()) return fail(VF_ERR_INVALID, "no observers set (vf_terrain_set_cumulative_viewshed)");
    if (!t->have_uniforms) return fail(VF_ERR_INVALID, "uniforms not set");
    const float spacing = spacing_of(t->inputs.u);
    for (size_t k = 0; k < H.xz.size(); ++k) vertices[k] = viewshed_index(t, H.xz[k], spacing);
    return VF_OK;
}

int vf_terrain_debug_cumulative_viewshed_batch(vf_terrain *t, uint32_t batch)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    t->cv.sum.force_batch(batch);
    return VF_OK;
}

int vf_terrain_debug_cumulative_viewshed_scans(vf_terrain *t, uint32_t *count) { return field_scans(t, kFieldCount, count); }

int vf_terrain_debug_cumulative_viewshed_stage(vf_terrain *t, uint32_t repeats, float *ms) { return summed_stage(t, kFieldCount, "cumulative viewshed", repeats, ms); }

// ---- sun exposure (vf_sun_exposure.h) ---------------------------------------------------

// The carries of a batch may take this many floats (32 MiB), for the reason DESIGN.md 4m measured: every sun of a batch reads the one
// height cache, and carries that stream through the last-level cache push it out.
constexpr size_t kSeCarryFloats = (size_t)8u << 20;
constexpr uint32_t kSeMaxBatch = 4096;                        // (the sun's index rides in grid.z and grid.y: at most 65535)

// suns per launch: as many as the budget for the carries holds, a slot being nchunks x (2n - 1) floats
static uint32_t exposure_batch(const vf_terrain *t, uint32_t scans, size_t stride)
{
    const size_t B = t->se.sum.forced_batch ? t->se.sum.forced_batch : std::max<size_t>(kSeCarryFloats / stride, 1u);
    return (uint32_t)std::max<size_t>(std::min<size_t>(std::min<size_t>(B, kSeMaxBatch), scans), 1u);
}

// `sum` holds the field of the uniforms `u`, the handle's heights, suns, weights and scan parameters once the work queued on `s` is
// done (the height cache must be current and ordered before `s`).  force: compute it anyway.
static int exposure_field(vf_terrain *t, const float *u, hipStream_t s, bool force)
{
    vf_terrain::SunExposure &H = t->se;
    const uint32_t N = (uint32_t)H.weights.size();
    if (!N) return fail(VF_ERR_INVALID, "no suns set (vf_terrain_set_sun_exposure)");
    const size_t nv = (size_t)t->n * t->n;
    const char *nomem = "sun exposure field allocation failed";
    if (int rc = H.sum.reserve(t, nomem)) return rc;
    const float spacing = spacing_of(u), exag = u[38];
    std::vector<uint32_t> key = key_of({ spacing, exag, H.softness, H.bias, H.incidence ? 1.0f : 0.0f });
    key.push_back(N);
    for (float f : H.suns) key.push_back(key_bits(f));
    for (float f : H.weights) key.push_back(key_bits(f));
    bool current;
    if (int rc = H.sum.value.prepare(t, key, force, nomem, &current)) return rc;
    if (current) return VF_OK;
    // the suns that add something, in the order of their launches: x-major scans, z-major scans, degenerate suns (every vertex lit)
    std::vector<ExposureSun> part[3];
    for (uint32_t o = 0; o < N; ++o) {
        const float *sun = &H.suns[3u * o];
        if (!(sun[1] > 0.0f) || H.weights[o] == 0.0f) continue;           // not counted, or q = 0 everywhere
        ExposureSun E = {};
        const bool scan = sun_plan(t, sun, spacing, exag, 1.0f, H.softness, H.bias, E.S);
        E.S.n = t->n; E.S.nb = t->nb;
        E.sx = sun[0]; E.sy = sun[1]; E.sz = sun[2];
        E.sl = std::sqrt((sun[0] * sun[0] + sun[1] * sun[1]) + sun[2] * sun[2]);
        E.w = H.weights[o];
        part[scan ? (E.S.zmajor ? 1 : 0) : 2].push_back(E);
    }
    const uint32_t nx = (uint32_t)part[0].size(), scans = nx + (uint32_t)part[1].size(), nflat = (uint32_t)part[2].size();
    H.recs.clear();
    for (const std::vector<ExposureSun> &p : part) H.recs.insert(H.recs.end(), p.begin(), p.end());
    const uint32_t nchunks = (t->n + kShChunk - 1u) / kShChunk;
    const size_t stride = (size_t)nchunks * (2u * t->n - 1u);
    const uint32_t B = exposure_batch(t, scans, stride);
    if ((scans && H.d_cmax.reserve((size_t)B * stride, (size_t)B * stride) != hipSuccess)
        || (!H.recs.empty() && H.d_suns.reserve(H.recs.size(), H.recs.size()) != hipSuccess)
        || (H.incidence && H.d_slope.reserve(nv, nv) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(VF_ERR_NOMEM, "sun exposure scan allocation failed");
    }
    if (!H.recs.empty())
        VF_HIP_TRY(hipMemcpyAsync(H.d_suns.p, H.recs.data(), H.recs.size() * sizeof(ExposureSun), hipMemcpyHostToDevice, s));   // (pageable source: returns when the copy is staged)
    VF_HIP_TRY(H.sum.zero(t, s));
    const dim3 threads(256);
    const float *hblk = t->d_hblk;
    uint32_t *sum = H.sum.d_sum.p;
    const float2 *slope = H.incidence ? H.d_slope.p : nullptr;
    if (H.incidence && !H.recs.empty())
        hipLaunchKernelGGL((k_exposure_slopes<0>), dim3((t->n + 31u) / 32u, (t->n + 7u) / 8u), threads, 0, s, hblk, t->n, t->nb, exag, grid_step(t) * spacing, H.d_slope.p);
    for (uint32_t b0 = 0; b0 < scans; b0 += B) {               // three launches per major axis and batch; the batches share the carries, in stream order
        const uint32_t b1 = std::min(b0 + B, scans), mid = std::min(std::max(b0, nx), b1);
        const uint32_t lo[2] = { b0, mid }, hi[2] = { mid, b1 };
        uint32_t lines[2] = { 0u, 0u };
        for (int z = 0; z < 2; ++z)
            for (uint32_t o = lo[z]; o < hi[z]; ++o) lines[z] = std::max(lines[z], H.recs[o].S.nlines);
        const ExposureSun *suns = H.d_suns.p + b0;
        for (int z = 0; z < 2; ++z) {
            if (lo[z] == hi[z]) continue;
            const dim3 grid(nchunks, (lines[z] + kShLines - 1u) / kShLines, hi[z] - lo[z]);
            float *cmax = H.d_cmax.p + (size_t)(lo[z] - b0) * stride;
            if (z) hipLaunchKernelGGL((k_exposure_chunk_max<true>), grid, threads, 0, s, H.d_suns.p + lo[z], hblk, cmax, stride);
            else hipLaunchKernelGGL((k_exposure_chunk_max<false>), grid, threads, 0, s, H.d_suns.p + lo[z], hblk, cmax, stride);
        }
        hipLaunchKernelGGL((k_exposure_carry<0>), dim3((std::max(lines[0], lines[1]) + 255u) / 256u, b1 - b0), threads, 0, s, suns, H.d_cmax.p, stride);
        for (int z = 0; z < 2; ++z) {
            if (lo[z] == hi[z]) continue;
            const dim3 grid(nchunks, (lines[z] + kShLines - 1u) / kShLines, hi[z] - lo[z]);
            const float *carry = H.d_cmax.p + (size_t)(lo[z] - b0) * stride;
            const ExposureSun *ps = H.d_suns.p + lo[z];
            if (z && H.incidence) hipLaunchKernelGGL((k_exposure_lit<true, true>), grid, threads, 0, s, ps, hblk, carry, stride, slope, sum);
            else if (z) hipLaunchKernelGGL((k_exposure_lit<true, false>), grid, threads, 0, s, ps, hblk, carry, stride, slope, sum);
            else if (H.incidence) hipLaunchKernelGGL((k_exposure_lit<false, true>), grid, threads, 0, s, ps, hblk, carry, stride, slope, sum);
            else hipLaunchKernelGGL((k_exposure_lit<false, false>), grid, threads, 0, s, ps, hblk, carry, stride, slope, sum);
        }
    }
    const dim3 flat((uint32_t)((nv + 255u) / 256u));
    if (nflat && H.incidence) hipLaunchKernelGGL((k_exposure_flat<true>), flat, threads, 0, s, (const ExposureSun *)H.d_suns.p + scans, nflat, slope, (uint32_t)nv, sum);
    else if (nflat) hipLaunchKernelGGL((k_exposure_flat<false>), flat, threads, 0, s, (const ExposureSun *)H.d_suns.p + scans, nflat, slope, (uint32_t)nv, sum);
    return H.sum.finish(t, s, H.wtot, key, B);
}

// The sun exposure's tint of a frame: the field if it is stale, then k_viewshed_tint on f = min(exposure / wtot, 1)
static int exposure_pass(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba)
{
    if (int rc = exposure_field(t, t->inputs.u, s)) return rc;
    return t->se.sum.tint(t, s, P, V, redo, rgba);
}

int vf_terrain_set_sun_exposure(vf_terrain *t, int enable, const float *suns_xyz, const float *weights, uint32_t count, int incidence, float softness,
                                float bias, const uint8_t high_rgba[4], const uint8_t low_rgba[4])
{
    if (!t || !suns_xyz || !high_rgba || !low_rgba) return fail(VF_ERR_INVALID, "NULL argument");
    vf_terrain::SunExposure &H = t->se;
    if (count < 1u || count > VF_SUN_EXPOSURE_MAX_SUNS) return fail(VF_ERR_INVALID, "sun exposure takes 1 to 65535 suns");
    for (size_t k = 0; k < (size_t)3u * count; ++k)
        if (!std::isfinite(suns_xyz[k])) return fail(VF_ERR_INVALID, "the suns must be finite");
    for (size_t k = 0; weights && k < count; ++k)
        if (!(weights[k] >= 0.0f && weights[k] <= 1.0f)) return fail(VF_ERR_INVALID, "the weights must lie in [0, 1]");
    if (!(std::isfinite(softness) && softness > 0.0f)) return fail(VF_ERR_INVALID, "softness must be a finite number > 0");
    if (!(std::isfinite(bias) && bias >= 0.0f)) return fail(VF_ERR_INVALID, "bias must be a finite number >= 0");
    if (enable && (t->shard_tiles || t->nranks != 1)) return fail(VF_ERR_INVALID, "sun exposure needs a whole-frame handle: sharded handles are not supported");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    if (enable) { if (int rc = ensure_vis(t)) return rc; }
    const uint32_t hi = pack_rgba8(high_rgba), lo = pack_rgba8(low_rgba);
    std::vector<float> suns(suns_xyz, suns_xyz + (size_t)3u * count), w(count, 1.0f);
    if (weights) w.assign(weights, weights + count);
    // (compared as bits, as the field's key is: -0 is not +0)
    const bool same = suns.size() == H.suns.size() && !std::memcmp(suns.data(), H.suns.data(), suns.size() * sizeof(float))
                      && !std::memcmp(w.data(), H.weights.data(), w.size() * sizeof(float));
    if (H.enabled != (enable != 0) || !same || H.incidence != (incidence != 0) || H.softness != softness || H.bias != bias || H.sum.high_rgba != hi || H.sum.low_rgba != lo)
        t->inputs_gen++;
    H.enabled = enable != 0; H.incidence = incidence != 0;
    H.suns.swap(suns); H.weights.swap(w);
    H.counted = 0; H.wtot = 0.0f;
    for (uint32_t o = 0; o < count; ++o)
        if (H.suns[3u * o + 1u] > 0.0f) { H.counted++; H.wtot += H.weights[o]; }
    H.softness = softness; H.bias = bias; H.sum.high_rgba = hi; H.sum.low_rgba = lo;
    return VF_OK;
}

int vf_terrain_clear_sun_exposure(vf_terrain *t)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    if (t->se.enabled) t->inputs_gen++;
    exposure_release(t);
    return VF_OK;
}

int vf_terrain_read_sun_exposure_field(vf_terrain *t, float *exposure) { return field_out(t, kFieldExposure, exposure, nullptr, nullptr); }
int vf_terrain_sun_exposure_field_device(vf_terrain *t, float *dev_exposure, void *stream) { return field_out(t, kFieldExposure, nullptr, dev_exposure, stream); }

int vf_terrain_sun_exposure_info(vf_terrain *t, vf_sun_exposure_info *out)
{
    if (!t || !out) return fail(VF_ERR_INVALID, "NULL argument");
    const vf_terrain::SunExposure &H = t->se;
    *out = vf_sun_exposure_info();
    out->enabled = H.enabled ? 1 : 0; out->incidence = H.incidence ? 1 : 0;
    out->count = (uint32_t)H.weights.size(); out->counted = H.counted; out->batch = H.sum.batch;
    out->weight_total = H.wtot; out->softness = H.softness; out->bias = H.bias;
    H.sum.colours(out->high_rgba, out->low_rgba);
    return VF_OK;
}

int vf_terrain_debug_sun_exposure_batch(vf_terrain *t, uint32_t batch)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    t->se.sum.force_batch(batch);
    return VF_OK;
}

int vf_terrain_debug_sun_exposure_scans(vf_terrain *t, uint32_t *count) { return field_scans(t, kFieldExposure, count); }

int vf_terrain_debug_sun_exposure_stage(vf_terrain *t, uint32_t repeats, float *ms) { return summed_stage(t, kFieldExposure, "sun exposure", repeats, ms); }

// ---- atmospheric haze (vf_haze.h) ---------------------------------------------------------

// contract item 4: y of -R^T t of the column-major view matrix, as mat_vec reads it
static float haze_eye_y(const float *u) { return -std::fmaf(u[6], u[14], std::fmaf(u[5], u[13], u[4] * u[12])); }

static HazeParams haze_params(const vf_terrain *t, const float *u)
{
    const vf_terrain::Haze &H = t->hz;
    HazeParams Z = {};
    Z.decode = t->ctx->d_decode;
    Z.rgba = H.rgba; Z.density = H.density; Z.start = H.start; Z.falloff = H.falloff; Z.base = H.base; Z.max_opacity = H.max_opacity;
    Z.eye_y = haze_eye_y(u);
    Z.background = H.background ? 1u : 0u;
    return Z;
}

// Both CLIPPED instantiations, in k_resolve's launch shape (gb_grid): into the colour buffer `rgba`, or (rgba == NULL) the opacities into `plane`
static void haze_launch(const vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, const float *u, uint32_t *rgba,
                        float *plane)
{
    const dim3 grid = gb_grid(t), threads(256);
    const HazeParams Z = haze_params(t, u);
    const float *thr = t->ctx->d_thresh;
    const uint32_t *vis = t->d_vis;
    if (rgba) {
        hipLaunchKernelGGL((k_haze<false, false>), grid, threads, 0, s, P, V, thr, vis, Z, redo, rgba, (float *)nullptr);
        hipLaunchKernelGGL((k_haze<true, false>), grid, threads, 0, s, P, V, thr, vis, Z, redo, rgba, (float *)nullptr);
    } else {
        hipLaunchKernelGGL((k_haze<false, true>), grid, threads, 0, s, P, V, thr, vis, Z, redo, (uint32_t *)nullptr, plane);
        hipLaunchKernelGGL((k_haze<true, true>), grid, threads, 0, s, P, V, thr, vis, Z, redo, (uint32_t *)nullptr, plane);
    }
}

// The haze of a frame, on the draw stream behind its tile kernels (which stored the visibility), the relight passes and the tints
static int haze_pass(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba)
{
    haze_launch(t, s, P, V, redo, t->inputs.u, rgba, nullptr);
    VF_HIP_TRY(hipGetLastError());
    return VF_OK;
}

// ---- hazed overlay layers (vf_overlay_haze.h) -----------------------------------------------

// overlay_pass's launches on a frame that hazes overlay layers: the side records behind k_ov_setup ...
static void ov_haze_setup_launch(vf_terrain *t, hipStream_t s, const FrameParams &P)
{
    vf_terrain::Overlays &O = t->ov;
    hipLaunchKernelGGL(k_ov_haze_setup<0>, dim3((O.nprims + 255u) / 256u), dim3(256), 0, s, P, axis(t), O.nprims, O.in.p, O.hzrec.p,
                       haze_params(t, t->inputs.u));
}

// ... and the composite in place of k_ov_composite / k_ov_composite_occlude, with the handle's current haze and the frame's eye
static void ov_haze_composite_launch(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, uint32_t nbx, uint32_t nbins, bool occlude)
{
    vf_terrain::Overlays &O = t->ov;
    const HazeParams Z = haze_params(t, t->inputs.u);
    const dim3 threads(256);
    if (occlude)
        hipLaunchKernelGGL(k_ov_composite_haze<true>, dim3(nbins), threads, 0, s, t->oW, t->oH, nbx, O.prim.p, O.d_cnt, O.d_start, O.list.p,
                           t->ctx->d_decode, t->ctx->d_thresh, O.mask.p, t->d_rgba, P, V, t->d_vis, O.dep.p, O.hzrec.p, Z);
    else
        hipLaunchKernelGGL(k_ov_composite_haze<false>, dim3(nbins), threads, 0, s, t->oW, t->oH, nbx, O.prim.p, O.d_cnt, O.d_start, O.list.p,
                           t->ctx->d_decode, t->ctx->d_thresh, O.mask.p, t->d_rgba, P, V, (const uint32_t *)nullptr, (const float4 *)nullptr,
                           O.hzrec.p, Z);
}

// A point / line / contour layer takes the handle's atmospheric haze, or stops taking it: a flag on its records.  The
// side records are made by the first hazed layer and grow with the primitives from then on (ov_append).
int vf_terrain_set_layer_haze(vf_terrain *t, uint32_t layer_id, int on)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (int rc = ov_usable(t)) return rc;
    vf_terrain::Overlays &O = t->ov;
    if (layer_id >= O.layer.size()) return fail(VF_ERR_INVALID, "no overlay layer with that id");
    vf_terrain::Overlays::Layer &L = O.layer[layer_id];
    if (L.polygon) return fail(VF_ERR_INVALID, "a polygon layer cannot take the haze: polygon fills have no depth");
    VF_HIP_TRY(wait_frame(t));                                // (a frame in flight reads the records)
    if (on) {
        const hipError_t e = O.hzrec.reserve(O.in.cap, O.in.cap);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(VF_ERR_NOMEM, std::string("overlay allocation failed: ") + hipGetErrorString(e)); }
    }
    if (L.hi > L.lo) {
        hipLaunchKernelGGL(k_ov_haze_flag<0>, dim3((L.hi - L.lo + 255u) / 256u), dim3(256), 0, t->ctx->stream, L.lo, L.hi, O.in.p, on ? 1u : 0u);
        VF_HIP_TRY(hipGetLastError());
        VF_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
    }
    if (L.haze != (on != 0)) O.hazed += on ? 1u : (uint32_t)-1;
    L.haze = on != 0;
    return VF_OK;
}

int vf_terrain_layer_haze(vf_terrain *t, uint32_t layer_id, int *on)
{
    if (!t || !on) return fail(VF_ERR_INVALID, "NULL argument");
    if (layer_id >= t->ov.layer.size()) return fail(VF_ERR_INVALID, "no overlay layer with that id");
    *on = t->ov.layer[layer_id].haze ? 1 : 0;
    return VF_OK;
}

int vf_terrain_set_haze(vf_terrain *t, int enable, float density, const uint8_t rgba[4], float start, float falloff, float base, float max_opacity,
                        int background)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (!rgba) return fail(VF_ERR_INVALID, "NULL argument: the haze colour");
    if (!(std::isfinite(density) && density >= 0.0f)) return fail(VF_ERR_INVALID, "density must be a finite number >= 0");
    if (!(std::isfinite(start) && start >= 0.0f)) return fail(VF_ERR_INVALID, "start must be a finite number >= 0");
    if (!(std::isfinite(falloff) && falloff >= 0.0f)) return fail(VF_ERR_INVALID, "falloff must be a finite number > 0, or 0 for uniform haze");
    if (!std::isfinite(base)) return fail(VF_ERR_INVALID, "base must be finite");
    if (!(max_opacity >= 0.0f && max_opacity <= 1.0f)) return fail(VF_ERR_INVALID, "max_opacity must lie in [0, 1]");
    if (enable && (t->shard_tiles || t->nranks != 1)) return fail(VF_ERR_INVALID, "haze needs a whole-frame handle: sharded handles are not supported");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    if (enable) { if (int rc = ensure_vis(t)) return rc; }
    vf_terrain::Haze &H = t->hz;
    const uint32_t c = pack_rgba8(rgba);
    if (H.enabled != (enable != 0) || H.density != density || H.rgba != c || H.start != start || H.falloff != falloff || H.base != base
        || H.max_opacity != max_opacity || H.background != (background != 0))
        t->inputs_gen++;
    H.enabled = enable != 0; H.background = background != 0;
    H.density = density; H.rgba = c; H.start = start; H.falloff = falloff; H.base = base; H.max_opacity = max_opacity;
    return VF_OK;
}

int vf_terrain_clear_haze(vf_terrain *t)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    if (t->hz.enabled) t->inputs_gen++;
    t->hz.d_plane.release();
    t->hz = vf_terrain::Haze();
    return VF_OK;
}

int vf_terrain_haze_info(vf_terrain *t, vf_haze_info *out)
{
    if (!t || !out) return fail(VF_ERR_INVALID, "NULL argument");
    const vf_terrain::Haze &H = t->hz;
    *out = vf_haze_info();
    out->enabled = H.enabled ? 1 : 0; out->background = H.background ? 1 : 0;
    out->density = H.density; out->start = H.start; out->falloff = H.falloff; out->base = H.base; out->max_opacity = H.max_opacity;
    for (int k = 0; k < 4; ++k) out->rgba[k] = (uint8_t)(H.rgba >> (8 * k));
    out->has_eye = t->have_uniforms ? 1 : 0;
    if (t->have_uniforms) out->eye_y = haze_eye_y(t->inputs.u);
    return VF_OK;
}

// The opacity plane, produced as the geometry buffers are: the frame rendered last drawn again with its visibility (gb_frame), then
// k_haze<., true> on `s` with the stored settings, enabled or not
static int haze_plane(vf_terrain *t, float *dev, hipStream_t s)
{
    GbFrame F;
    if (int rc = gb_frame(t, F)) return rc;
    haze_launch(t, s ? s : t->ctx->stream, F.P, F.V, t->ps[t->last_set].work_count + 3, (t->have_frame ? t->drawn_inputs : t->inputs).u, nullptr, dev);
    VF_HIP_TRY(hipGetLastError());
    return VF_OK;
}

int vf_terrain_read_haze_opacity(vf_terrain *t, float *dst)
{
    if (!t || !dst) return fail(VF_ERR_INVALID, "NULL argument");
    const size_t npx = (size_t)t->W * t->H;
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    if (t->hz.d_plane.reserve(npx, npx) != hipSuccess) { (void)hipGetLastError(); return fail(VF_ERR_NOMEM, "haze opacity allocation failed"); }
    hipStream_t s = t->ctx->stream;
    if (int rc = haze_plane(t, t->hz.d_plane.p, s)) return rc;
    VF_HIP_TRY(hipMemcpyAsync(dst, t->hz.d_plane.p, npx * sizeof(float), hipMemcpyDeviceToHost, s));
    VF_HIP_TRY(hipStreamSynchronize(s));
    return VF_OK;
}

int vf_terrain_haze_opacity_device(vf_terrain *t, float *dev, void *stream)
{
    if (!t || !dev) return fail(VF_ERR_INVALID, "NULL argument");
    hipStream_t s = stream ? (hipStream_t)stream : t->ctx->stream;
    if (int rc = haze_plane(t, dev, s)) return rc;
    VF_HIP_TRY(gb_order_after(t, s));
    return VF_OK;
}

int vf_terrain_debug_haze_stage(vf_terrain *t, uint32_t repeats, float *ms)
{
    if (!t || !ms) return fail(VF_ERR_INVALID, "NULL argument");
    if (repeats == 0) repeats = 1;
    RelightStage G;
    if (int rc = G.open(t)) return rc;
    float mean = 0.0f;
    const hipError_t err = time_launches(G.s, repeats, mean, [&](bool) { haze_launch(t, G.s, G.F.P, G.F.V, G.redo, G.u, t->d_rgba_scratch, nullptr); return hipGetLastError(); });
    if (err != hipSuccess) return fail(VF_ERR_HIP, std::string("haze diagnostics: ") + hipGetErrorString(err));
    *ms = mean;
    return VF_OK;
}

int vf_terrain_debug_item_stats(vf_terrain *t, uint32_t *dst, uint32_t max_items, uint32_t *count)
{
    if (!t || !dst || !count) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->timing || !t->stats_on || !t->rendered) return fail(VF_ERR_INVALID, "statistics not enabled or nothing rendered");
    int rc = vf_terrain_sync(t);
    if (rc != VF_OK) return rc;
    uint32_t n = 0;
    VF_HIP_TRY(hipMemcpy(&n, t->ps[t->last_set].work_count, sizeof n, hipMemcpyDeviceToHost));
    if (n > max_items) n = max_items;
    if (n) VF_HIP_TRY(hipMemcpy(dst, t->d_stats + 4, 4 * (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *count = n;
    return VF_OK;
}

// The set-up pass's output of the plan state the last frame was drawn from (include/vf_hip.h).  Host copies behind a full wait:
// nothing of this is on a frame's path.
int vf_terrain_debug_band_masks(vf_terrain *t, uint32_t *recs, uint64_t *masks, int32_t *xy, uint32_t max_blocks, uint32_t *count)
{
    static_assert(VF_BAND_SLOTS == (uint32_t)kBandSlots, "the header's slot count is the kernels'");
    if (!t || !count) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->rendered) return fail(VF_ERR_INVALID, "nothing rendered");
    if (max_blocks < t->nblocks) return fail(VF_ERR_INVALID, "max_blocks is smaller than the grid's blocks");
    const vf_terrain::PlanState &S = t->ps[t->last_set];
    if (!S.slab) return fail(VF_ERR_INVALID, "nothing rendered");
    VF_HIP_TRY(wait_frame(t));
    VF_HIP_TRY(sync_sides(t));
    const size_t nb = t->nblocks;
    if (recs) VF_HIP_TRY(hipMemcpy(recs, S.recs, nb * sizeof(BlockRec), hipMemcpyDeviceToHost));
    if (masks) VF_HIP_TRY(hipMemcpy(masks, S.band, nb * kBandSlots * sizeof(ulonglong2), hipMemcpyDeviceToHost));
    if (xy) {
        std::vector<VertexRec> v(nb * kBlockStride);
        VF_HIP_TRY(hipMemcpy(v.data(), S.vtx, v.size() * sizeof(VertexRec), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < v.size(); ++k) { xy[2 * k] = v[k].X; xy[2 * k + 1] = v[k].Y; }
    }
    *count = (uint32_t)nb;
    return VF_OK;
}

// The words the next plan reads, written into both plan states (include/vf_hip.h).  Host copies behind a full wait: nothing of this
// is on a frame's path.
int vf_terrain_debug_set_plan_feedback(vf_terrain *t, const uint32_t *tile_ticks, const uint8_t *strips_log2, const uint32_t *piece_ticks,
                                       uint32_t ntiles)
{
    if (!t || !tile_ticks || !strips_log2) return fail(VF_ERR_INVALID, "NULL argument");
    if (ntiles != t->local_tiles) return fail(VF_ERR_INVALID, "ntiles must be the handle's local tiles");
    for (uint32_t k = 0; k < ntiles; ++k) if (strips_log2[k] > 4u) return fail(VF_ERR_INVALID, "strips_log2 must be 0 .. 4");
    if (t->cursor.frames_since_reset < vf_terrain::kPlanStates)
        return fail(VF_ERR_INVALID, "the handle's first frames are planned from the static estimate: render two frames first");
    for (const auto &S : t->ps) if (!S.slab) return fail(VF_ERR_INVALID, "a plan state has not been used yet: render two frames first");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    VF_HIP_TRY(sync_sides(t));
    VF_HIP_TRY(drop_preplan(t));                            // (its waits and its memset are queued on one of the streams waited for next)
    VF_HIP_TRY(wait_frame(t));
    VF_HIP_TRY(sync_sides(t));
    if (!ntiles) return VF_OK;                              // (a shard without tiles)
    const size_t all_tiles = (size_t)t->ntx * t->nty;
    std::vector<uint32_t> pieces((size_t)ntiles * 64u, 0u), flags(ntiles);
    if (piece_ticks) std::memcpy(pieces.data(), piece_ticks, pieces.size() * sizeof(uint32_t));
    for (auto &S : t->ps) {
        VF_HIP_TRY(hipMemcpy(S.feedback, tile_ticks, (size_t)ntiles * sizeof(uint32_t), hipMemcpyHostToDevice));
        VF_HIP_TRY(hipMemcpy(S.feedback + all_tiles + 1u, pieces.data(), pieces.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        VF_HIP_TRY(hipMemcpy(flags.data(), S.background, (size_t)ntiles * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < ntiles; ++k) flags[k] = (flags[k] & 0xFFu) | ((uint32_t)strips_log2[k] << 8);
        VF_HIP_TRY(hipMemcpy(S.background, flags.data(), (size_t)ntiles * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    return VF_OK;
}

int vf_terrain_debug_plan_mode(const vf_terrain *t, uint32_t *mode)
{
    if (!t || !mode) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->rendered) return fail(VF_ERR_INVALID, "nothing rendered yet");
    *mode = t->last_plan_mode;
    return VF_OK;
}

// The candidate lists of the plan state drawn last (include/vf_hip.h).  Host copies behind a full wait.
int vf_terrain_debug_tile_lists(vf_terrain *t, vf_tile_list_info *out)
{
    if (!t || !out) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->rendered) return fail(VF_ERR_INVALID, "nothing rendered yet");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    std::memset(out, 0, sizeof *out);
    const vf_terrain::PlanState &S = t->ps[t->last_set];
    out->used = (t->last_plan_mode & VF_PLAN_TILE_LISTS) ? 1u : 0u;
    out->built = lists_valid(t, S) ? 1u : 0u;
    if (!out->built && !out->used) return VF_OK;
    VF_HIP_TRY(hipEventSynchronize(S.listed));
    uint32_t ctl[8];
    VF_HIP_TRY(hipMemcpy(ctl, S.tl_ctl, sizeof ctl, hipMemcpyDeviceToHost));
    out->tiles_listed = ctl[2]; out->tiles_fallback = ctl[3]; out->entries = ctl[4];
    out->capacity = S.tl_cap;
    const unsigned long long asked = (unsigned long long)ctl[0] | ((unsigned long long)ctl[1] << 32);
    out->units_asked = asked > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)asked;
    return VF_OK;
}

int vf_terrain_debug_set_tile_list_capacity(vf_terrain *t, uint32_t units)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    VF_HIP_TRY(sync_sides(t));
    VF_HIP_TRY(drop_preplan(t));                            // (a plan made ahead may hold "read the lists": planned again, without)
    VF_HIP_TRY(wait_frame(t));
    VF_HIP_TRY(sync_sides(t));
    t->tl_cap_debug = units;
    t->tl_job.pending = false;
    for (auto &S : t->ps) S.list_stamp = 0;                 // both states build theirs again, with the new capacity
    return VF_OK;
}

int vf_terrain_debug_phase_cycles(vf_terrain *t, uint64_t *dst, uint32_t n)
{
    if (!t || !dst) return fail(VF_ERR_INVALID, "NULL argument");
#ifndef VF_PHASE_PROF
    (void)n;
    return fail(VF_ERR_INVALID, "library built without -DVF_PHASE_PROF");
#else
    if (!t->timing || !t->stats_on || !t->rendered) return fail(VF_ERR_INVALID, "statistics not enabled or nothing rendered");
    int rc = vf_terrain_sync(t);
    if (rc != VF_OK) return rc;
    if (n > kPhaseSlots) n = kPhaseSlots;
    VF_HIP_TRY(hipMemcpy(dst, t->d_stats + stats_layout(t).phases, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VF_OK;
#endif
}

int vf_terrain_enable_timing(vf_terrain *t, int enable)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (enable != 0 && !t->ev[0].begin) {                   // the event ring is made when timing is first asked for
        VF_HIP_TRY(hipSetDevice(t->ctx->device));
        for (auto &f : t->ev) { VF_HIP_TRY(hipEventCreate(&f.begin)); VF_HIP_TRY(hipEventCreate(&f.end)); }
    }
    if (enable != 0) for (auto &S : t->ps) for (auto &e : S.pev) if (!e) VF_HIP_TRY(hipEventCreate(&e));
    if (enable < 0 || enable > 3) return fail(VF_ERR_INVALID, "enable must be 0 .. 3");
    t->timing = enable != 0;
    t->stats_on = enable == 1;   // 2, 3: HIP events only -- the tile kernel runs exactly as it does untimed (no per-item statistics)
    t->timing_every = enable == 3 ? 4u : 1u;
    t->timed_frames = 0;     // (re)start the averaging window
    return VF_OK;
}

int vf_terrain_timings(vf_terrain *t, vf_timings *out)
{
    if (!t || !out) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->timing || !t->rendered || t->timed_frames == 0) return fail(VF_ERR_INVALID, "timing not enabled or nothing rendered");
    int rc = vf_terrain_sync(t);
    if (rc != VF_OK) return rc;
    // average over the frames recorded since vf_terrain_enable_timing (at most the last kTimingRing)
    const uint32_t nf = t->timed_frames < (uint32_t)vf_terrain::kTimingRing ? t->timed_frames : (uint32_t)vf_terrain::kTimingRing;
    double ranges = 0, plan = 0, tile = 0, total = 0;
    uint32_t nplan = 0;
    for (uint32_t f = 0; f < nf; ++f) {
        float c = 0;
        VF_HIP_TRY(hipEventSynchronize(t->ev[f].end));
        VF_HIP_TRY(hipEventElapsedTime(&c, t->ev[f].begin, t->ev[f].end));      // clear + tile kernels, on the caller's stream
        tile += c; total += c;
    }
    // the plan chain: the last plan of each plan state (the frames drawn last, or the plan queued ahead of the next call)
    VF_HIP_TRY(sync_sides(t));
    for (auto &S : t->ps) {
        if (!S.pev_valid || !S.pev[2]) continue;
        float a = 0, b = 0;
        if (hipEventSynchronize(S.pev[2]) != hipSuccess || hipEventElapsedTime(&a, S.pev[0], S.pev[1]) != hipSuccess ||
            hipEventElapsedTime(&b, S.pev[1], S.pev[2]) != hipSuccess) { (void)hipGetLastError(); continue; }
        ranges += a; plan += b; ++nplan;
    }
    if (nf == 1u && t->ps[t->last_set].pev_valid) {         // a single timed frame: plan start -> RGBA8 complete
        float d = 0;
        if (hipEventElapsedTime(&d, t->ps[t->last_set].pev[0], t->ev[0].end) == hipSuccess && d > 0.0f) total = d;
        else (void)hipGetLastError();
    }
    out->ranges_ms = nplan ? (float)(ranges / nplan) : 0.0f; out->plan_ms = nplan ? (float)(plan / nplan) : 0.0f; out->tile_ms = (float)(tile / nf);
    out->total_ms = (float)(total / nf);
    if (nf >= 2 && t->timed_frames <= (uint32_t)vf_terrain::kTimingRing) {
        // frames rendered back to back overlap (frame f+1 plans while frame f draws): the frame period is what a frame costs
        float span = 0;
        VF_HIP_TRY(hipEventElapsedTime(&span, t->ev[0].end, t->ev[nf - 1].end));
        out->total_ms = span / (float)((nf - 1) * t->timing_every);
    }
    out->frames = nf;
    out->blocks_rasterised = 0; out->blocks_distinct = 0;
    out->tiles = t->local_tiles;
    if (t->stats_on) {
        uint32_t c[4];
        VF_HIP_TRY(hipMemcpy(c, t->d_stats, sizeof c, hipMemcpyDeviceToHost));
        out->blocks_rasterised = c[0];   // distinct blocks behind those pairs (last frame): the bitmap behind the per-item statistics
        std::vector<uint32_t> bits((t->nblocks + 31) / 32);
        VF_HIP_TRY(hipMemcpy(bits.data(), t->d_stats + stats_layout(t).block_bits, bits.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint32_t n = 0;
        for (uint32_t w : bits) n += (uint32_t)__builtin_popcount(w);
        out->blocks_distinct = n;
    }
    return VF_OK;
}

int vf_terrain_frame_times(vf_terrain *t, float *tile_ms, float *period_ms, uint32_t max_frames, uint32_t *count)
{
    if (!t || !count) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->timing || !t->rendered || t->timed_frames == 0) return fail(VF_ERR_INVALID, "timing not enabled or nothing rendered");
    int rc = vf_terrain_sync(t);
    if (rc != VF_OK) return rc;
    const uint32_t ring = (uint32_t)vf_terrain::kTimingRing;
    const uint32_t nf = std::min(std::min(t->timed_frames, ring), max_frames);
    const uint32_t first = t->timed_frames - nf;            // frame numbers first .. timed_frames - 1 live in ring slot (number % ring)
    for (uint32_t k = 0; k < nf; ++k) {
        const vf_terrain::FrameEvents &e = t->ev[(first + k) % ring];
        VF_HIP_TRY(hipEventSynchronize(e.end));
        if (tile_ms) VF_HIP_TRY(hipEventElapsedTime(&tile_ms[k], e.begin, e.end));
        if (period_ms) {
            period_ms[k] = 0.0f;
            if (k) { VF_HIP_TRY(hipEventElapsedTime(&period_ms[k], t->ev[(first + k - 1u) % ring].end, e.end)); period_ms[k] /= (float)t->timing_every; }
        }
    }
    *count = nf;
    return VF_OK;
}

// ------------------------------------------------------------------------------------------------

int vf_grid_generate_device(vf_ctx *ctx, uint32_t nx, uint32_t nz, float dx, float dy, float *dev_xy, float *dev_uv,
                            uint32_t *dev_idx, void *stream)
{
    if (!ctx || !dev_xy || !dev_uv || !dev_idx) return fail(VF_ERR_INVALID, "NULL argument");
    if (nx < 2 || nz < 2) return fail(VF_ERR_INVALID, "nx and nz must be >= 2");
    if ((uint64_t)nx * nz > 0xFFFFFFFFull) return fail(VF_ERR_INVALID, "vertex count exceeds u32 indices");
    VF_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    size_t nv = (size_t)nx * nz, nc = (size_t)(nx - 1) * (nz - 1);
    hipLaunchKernelGGL(k_grid_vertices, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, nx, nz, dx, dy, (float2 *)dev_xy, (float2 *)dev_uv);
    hipLaunchKernelGGL(k_grid_indices, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, nx, nz, dev_idx);
    VF_HIP_TRY(hipGetLastError());
    return VF_OK;
}

int vf_grid_generate(vf_ctx *ctx, uint32_t nx, uint32_t nz, float dx, float dy, float *xy, float *uv, uint32_t *idx)
{
    if (!ctx || !xy || !uv || !idx) return fail(VF_ERR_INVALID, "NULL argument");
    if (nx < 2 || nz < 2) return fail(VF_ERR_INVALID, "nx and nz must be >= 2");
    VF_HIP_TRY(hipSetDevice(ctx->device));
    size_t nv = (size_t)nx * nz, ni = 6 * (size_t)(nx - 1) * (nz - 1);
    float *d_xy = nullptr, *d_uv = nullptr;
    uint32_t *d_idx = nullptr;
    hipError_t err = hipMalloc(&d_xy, nv * 8);
    if (err == hipSuccess) err = hipMalloc(&d_uv, nv * 8);
    if (err == hipSuccess) err = hipMalloc(&d_idx, ni * 4);
    int rc = VF_OK;
    if (err != hipSuccess) rc = fail(VF_ERR_NOMEM, std::string("grid_generate allocation failed: ") + hipGetErrorString(err));
    if (rc == VF_OK) rc = vf_grid_generate_device(ctx, nx, nz, dx, dy, d_xy, d_uv, d_idx, ctx->stream);
    if (rc == VF_OK) {
        err = hipStreamSynchronize(ctx->stream);
        if (err == hipSuccess) err = hipMemcpy(xy, d_xy, nv * 8, hipMemcpyDeviceToHost);
        if (err == hipSuccess) err = hipMemcpy(uv, d_uv, nv * 8, hipMemcpyDeviceToHost);
        if (err == hipSuccess) err = hipMemcpy(idx, d_idx, ni * 4, hipMemcpyDeviceToHost);
        if (err != hipSuccess) rc = fail(VF_ERR_HIP, std::string("grid_generate readback failed: ") + hipGetErrorString(err));
    }
    if (d_xy) (void)hipFree(d_xy);
    if (d_uv) (void)hipFree(d_uv);
    if (d_idx) (void)hipFree(d_idx);
    return rc;
}

int vf_triangle_render(vf_ctx *ctx, uint32_t width, uint32_t height, uint8_t *rgba_host)
{
    if (!ctx || !rgba_host) return fail(VF_ERR_INVALID, "NULL argument");
    if (width == 0 || height == 0 || width > 16384 || height > 16384) return fail(VF_ERR_INVALID, "width/height must be in 1..16384");
    VF_HIP_TRY(hipSetDevice(ctx->device));
    size_t npx = (size_t)width * height;
    uint32_t *d = nullptr;
    VF_HIP_TRY(hipMalloc(&d, npx * 4));
    hipLaunchKernelGGL(k_triangle, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, ctx->stream, width, height, ctx->d_thresh, d);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    if (err == hipSuccess) err = hipMemcpy(rgba_host, d, npx * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (err != hipSuccess) return fail(VF_ERR_HIP, std::string("triangle render failed: ") + hipGetErrorString(err));
    return VF_OK;
}

// ---- seeded fills: what the flood and the spill share (SeededFill) -----------------------

static_assert(VF_FLOOD_SEEDS == SeededFill::kSeeds && VF_SPILL_SEEDS == SeededFill::kSeeds && VF_FLOOD_MAX_SEEDS == VF_SPILL_MAX_SEEDS, "one seed-list rule");

std::vector<uint32_t> SeededFill::vertices(const vf_terrain *t, const float *u) const
{
    const float spacing = spacing_of(u);
    std::vector<uint32_t> v(xz.size());
    for (size_t k = 0; k < xz.size(); ++k) v[k] = viewshed_index(t, xz[k], spacing);
    return v;
}

int SeededFill::read_seeds(const vf_terrain *t, uint32_t *out, const char *none) const
{
    if (xz.empty()) return fail(VF_ERR_INVALID, none);
    if (!t->have_uniforms) return fail(VF_ERR_INVALID, "uniforms not set");
    const std::vector<uint32_t> v = vertices(t, t->inputs.u);
    std::memcpy(out, v.data(), v.size() * sizeof(uint32_t));
    return VF_OK;
}

int SeededFill::set(vf_terrain *t, int enable, int new_mode, const float *seeds_xz, uint32_t count, const uint8_t shallow[4], const uint8_t deep[4], float full,
                    bool other_changed, const Words &W)
{
    if (!(std::isfinite(full) && full > 0.0f)) return fail(VF_ERR_INVALID, "depth_full must be a finite number > 0");
    if (new_mode < 0 || new_mode > kSeeds || !((W.modes >> new_mode) & 1)) return fail(VF_ERR_INVALID, W.unknown_mode);
    if (new_mode == kSeeds) {
        if (!seeds_xz) return fail(VF_ERR_INVALID, "NULL argument: the seeds");
        if (count < 1u || count > VF_FLOOD_MAX_SEEDS) return fail(VF_ERR_INVALID, W.count);
        for (size_t k = 0; k < (size_t)2u * count; ++k)
            if (!std::isfinite(seeds_xz[k])) return fail(VF_ERR_INVALID, "the seeds must be finite");
    } else count = 0u;
    if (enable && (t->shard_tiles || t->nranks != 1)) return fail(VF_ERR_INVALID, W.sharded);
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    if (enable) { if (int rc = ensure_vis(t)) return rc; }
    const uint32_t sh = pack_rgba8(shallow), dp = pack_rgba8(deep);
    std::vector<float> seeds;
    if (count) seeds.assign(seeds_xz, seeds_xz + (size_t)2u * count);
    if (enabled != (enable != 0) || !have || other_changed || mode != new_mode || xz != seeds || shallow_rgba != sh || deep_rgba != dp || depth_full != full)
        t->inputs_gen++;
    enabled = enable != 0; have = true;
    mode = new_mode;
    xz.swap(seeds);
    shallow_rgba = sh; deep_rgba = dp; depth_full = full;
    return VF_OK;
}

// The tint of a frame by the fill of field f, on the draw stream behind its tile kernels (which stored the visibility): the field if
// it is stale, then `launch`, the feature's tint pass over the covered pixels
using FillLaunch = void(const vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba);
static int fill_pass(vf_terrain *t, Field f, FillLaunch *launch, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba)
{
    if (int rc = kFieldTable[f].compute(t, t->inputs.u, s, false)) return rc;
    launch(t, s, P, V, redo, rgba);
    VF_HIP_TRY(hipGetLastError());
    return VF_OK;
}

static SeededFill &flood_fill(vf_terrain *t) { return t->fd.fill; }
static SeededFill &spill_fill(vf_terrain *t) { return t->sp.fill; }

// The vf_terrain_clear_* call of a fill: off, the defaults again, the buffers freed (`release`)
static int fill_clear(vf_terrain *t, SeededFill &(*fill)(vf_terrain *), void (*release)(vf_terrain *))
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    VF_HIP_TRY(wait_frame(t));
    if (fill(t).enabled) t->inputs_gen++;
    release(t);
    return VF_OK;
}

// The vf_terrain_debug_*_stage call of a fill: ms[0] its field f computed anyway, ms[1] its tint pass on the frame rendered last
static int fill_stage(vf_terrain *t, Field f, SeededFill &(*fill)(vf_terrain *), const char *label, const char *none, FillLaunch *launch, uint32_t repeats, float ms[2])
{
    if (!t || !ms) return fail(VF_ERR_INVALID, "NULL argument");
    if (!fill(t).have || !fill(t).enabled) return fail(VF_ERR_INVALID, none);
    if (repeats == 0) repeats = 1;
    RelightStage G;
    if (int rc = G.open(t)) return rc;
    if (int rc = kFieldTable[f].compute(t, G.u, G.s, false)) return rc;          // (the tint's launches below read what the current field left)
    return G.time_pair(repeats, ms, label, [&] { return kFieldTable[f].compute(t, G.u, G.s, true); },
                       [&] { launch(t, G.s, G.F.P, G.F.V, G.redo, t->d_rgba_scratch); });
}

// ---- flood analysis (vf_flood.h) -------------------------------------------------------------

static uint32_t flood_tiles(const vf_terrain *t) { return (t->n + kFloodTile - 1u) / kFloodTile; }

// The field holds the depth of the handle's heights, level and sources once this returns (the height cache must be current and ordered
// before `s`, as for shadow_field); d_fl and d_wd hold what the tint reads.  force: compute it anyway.
static int flood_field(vf_terrain *t, const float *u, hipStream_t s, bool force)
{
    vf_terrain::Flood &H = t->fd;
    SeededFill &S = H.fill;
    if (!S.have) return fail(VF_ERR_INVALID, "no flood set (vf_terrain_set_flood)");
    std::vector<uint32_t> key = key_of({ H.level });
    std::vector<uint32_t> ij = S.key_tail(t, u, key);
    bool current;
    if (int rc = S.field.prepare(t, key, force, "flood field allocation failed", &current)) return rc;
    if (current) return VF_OK;
    const uint32_t n = t->n, ftx = flood_tiles(t), tiles = ftx * ftx;
    const size_t words = (size_t)tiles * kFloodTile, nv = (size_t)n * n;
    // (k_flood_depth packs the two counts into the halves of one 64-bit word and vf_flood_info reports them as uint32: vf_terrain_create
    //  holds the grid to 8192, n x n to 2^26)
    if (nv >> 32) return fail(VF_ERR_INVALID, "the grid is too large for the flood's 32-bit vertex counts");
    if (H.d_wet.reserve(words, words) != hipSuccess || H.d_fl.reserve(words, words) != hipSuccess || H.d_wd.reserve(nv, nv) != hipSuccess
        || S.reserve(2u, ij.size()) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VF_ERR_NOMEM, "flood mask allocation failed");
    }
    const dim3 rows(ftx, ftx * (kFloodTile / 4u)), threads(256);
    const float *hblk = t->d_hblk;
    if (S.mode == VF_FLOOD_EVERYWHERE)
        hipLaunchKernelGGL((k_flood_wet<true>), rows, threads, 0, s, n, t->nb, ftx, ftx * kFloodTile, H.level, hblk, H.d_wet.p, H.d_fl.p, H.d_wd.p);
    else
        hipLaunchKernelGGL((k_flood_wet<false>), rows, threads, 0, s, n, t->nb, ftx, ftx * kFloodTile, H.level, hblk, H.d_wet.p, H.d_fl.p, H.d_wd.p);
    VF_HIP_TRY(hipGetLastError());
    uint32_t passes = 0;
    if (S.mode != VF_FLOOD_EVERYWHERE) {
        if (S.mode == VF_FLOOD_SEEDS) {
            const uint32_t count = (uint32_t)(ij.size() / 2u);
            VF_HIP_TRY(S.upload(ij, s));
            hipLaunchKernelGGL((k_flood_seed<false>), dim3((count + 255u) / 256u), threads, 0, s, n, ftx, (const uint32_t *)S.d_seeds.p, count,
                               (const uint32_t *)H.d_wet.p, (uint32_t *)H.d_fl.p);
        } else
            hipLaunchKernelGGL((k_flood_seed<true>), dim3((4u * n + 255u) / 256u), threads, 0, s, n, ftx, (const uint32_t *)nullptr, 4u * n,
                               (const uint32_t *)H.d_wet.p, (uint32_t *)H.d_fl.p);
        VF_HIP_TRY(hipGetLastError());
        // (every pass that changes something floods at least one more vertex)
        if (int rc = S.fixpoint(s, nv, "flood propagation did not reach a fixpoint within n x n + 1 passes", &passes, [&](uint32_t, uint32_t *changed) {
                hipLaunchKernelGGL((k_flood_pass<0>), dim3(tiles), dim3(64), 0, s, ftx, ftx, (const uint64_t *)H.d_wet.p, H.d_fl.p, changed);
            })) return rc;
    }
    unsigned long long counts = 0ull;
    VF_HIP_TRY(hipMemsetAsync(S.counts(), 0, sizeof counts, s));
    hipLaunchKernelGGL((k_flood_depth<0>), dim3(ftx, (n + 3u) / 4u), threads, 0, s, n, ftx, (const uint64_t *)H.d_wet.p, (const uint64_t *)H.d_fl.p,
                       (const float *)H.d_wd.p, S.field.d.p, (unsigned long long *)S.counts());
    VF_HIP_TRY(hipGetLastError());
    VF_HIP_TRY(hipMemcpyAsync(&counts, S.counts(), sizeof counts, hipMemcpyDeviceToHost, s));
    VF_HIP_TRY(hipStreamSynchronize(s));
    S.passes = passes; H.flooded = (uint32_t)counts; H.wettable = (uint32_t)(counts >> 32);
    S.field.computed(t, key);
    return VF_OK;
}

static void flood_launch(const vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba)
{
    const vf_terrain::Flood &H = t->fd;
    FloodTint T = {};
    T.fl = (const uint32_t *)H.d_fl.p; T.wd = H.d_wd.p; T.decode = t->ctx->d_decode;
    T.ntx = flood_tiles(t);
    T.shallow_rgba = H.fill.shallow_rgba; T.deep_rgba = H.fill.deep_rgba; T.depth_full = H.fill.depth_full;
    tint_launch(t, s, P, V, redo, rgba, T, k_flood_tint<false>, k_flood_tint<true>);
}

// The water of a frame, on the draw stream behind its tile kernels (which stored the visibility) and the relight passes: the field if
// it is stale, then the tint pass over the covered pixels
static int flood_pass(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba)
{
    return fill_pass(t, kFieldFlood, flood_launch, s, P, V, redo, rgba);
}

int vf_terrain_set_flood(vf_terrain *t, int enable, float level, int mode, const float *seeds_xz, uint32_t count, const uint8_t shallow_rgba[4],
                         const uint8_t deep_rgba[4], float depth_full)
{
    if (!t || !shallow_rgba || !deep_rgba) return fail(VF_ERR_INVALID, "NULL argument");
    if (!std::isfinite(level)) return fail(VF_ERR_INVALID, "level must be finite");
    static const SeededFill::Words W = { 1 << VF_FLOOD_EVERYWHERE | 1 << VF_FLOOD_EDGES | 1 << VF_FLOOD_SEEDS, "unknown flood mode",
                                         "a flood takes 1 to 65535 seeds", "a flood needs a whole-frame handle: sharded handles are not supported" };
    vf_terrain::Flood &H = t->fd;
    if (int rc = H.fill.set(t, enable, mode, seeds_xz, count, shallow_rgba, deep_rgba, depth_full, key_bits(H.level) != key_bits(level), W)) return rc;
    H.level = level;
    return VF_OK;
}

int vf_terrain_clear_flood(vf_terrain *t) { return fill_clear(t, flood_fill, flood_release); }
int vf_terrain_read_flood_field(vf_terrain *t, float *depth) { return field_out(t, kFieldFlood, depth, nullptr, nullptr); }
int vf_terrain_flood_field_device(vf_terrain *t, float *dev_depth, void *stream) { return field_out(t, kFieldFlood, nullptr, dev_depth, stream); }

int vf_terrain_flood_info(vf_terrain *t, vf_flood_info *out)
{
    if (!t || !out) return fail(VF_ERR_INVALID, "NULL argument");
    const vf_terrain::Flood &H = t->fd;
    *out = vf_flood_info();
    H.fill.info(out);
    out->has_flood = H.fill.have ? 1 : 0; out->level = H.level;
    out->flooded_vertices = H.flooded; out->wettable_vertices = H.wettable;
    return VF_OK;
}

int vf_terrain_read_flood_seeds(vf_terrain *t, uint32_t *vertices)
{
    if (!t || !vertices) return fail(VF_ERR_INVALID, "NULL argument");
    return t->fd.fill.read_seeds(t, vertices, "no seeds set (vf_terrain_set_flood with VF_FLOOD_SEEDS)");
}

int vf_terrain_debug_flood_scans(vf_terrain *t, uint32_t *count) { return field_scans(t, kFieldFlood, count); }

int vf_terrain_debug_flood_stage(vf_terrain *t, uint32_t repeats, float ms[2])
{
    return fill_stage(t, kFieldFlood, flood_fill, "flood", "no flood enabled (vf_terrain_set_flood)", flood_launch, repeats, ms);
}

int vf_terrain_debug_flood_group(vf_terrain *t, uint32_t group)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    return t->fd.fill.force_group(group);
}

// ---- spill analysis (vf_spill.h) -------------------------------------------------------------

static uint32_t spill_tiles(const vf_terrain *t) { return (t->n + kSpillTile - 1u) / kSpillTile; }

// The field holds the spill of the handle's heights and sources once this returns (the height cache must be current and ordered before
// `s`, as for shadow_field); d_sd holds what the tint reads.  force: compute it anyway.
static int spill_field(vf_terrain *t, const float *u, hipStream_t s, bool force)
{
    vf_terrain::Spill &H = t->sp;
    SeededFill &S = H.fill;
    if (!S.have) return fail(VF_ERR_INVALID, "no spill set (vf_terrain_set_spill)");
    std::vector<uint32_t> key;
    std::vector<uint32_t> ij = S.key_tail(t, u, key);
    bool current;
    if (int rc = S.field.prepare(t, key, force, "spill field allocation failed", &current)) return rc;
    if (current) return VF_OK;
    const uint32_t n = t->n, ftx = spill_tiles(t), tiles = ftx * ftx;
    const size_t words = (size_t)tiles * kSpillTileWords, nv = (size_t)n * n;
    // (k_spill_out packs the two counts into the halves of one 64-bit word and vf_spill_info reports them as uint32: vf_terrain_create
    //  holds the grid to 8192, n x n to 2^26)
    if (nv >> 32) return fail(VF_ERR_INVALID, "the grid is too large for the spill's 32-bit vertex counts");
    if (H.d_hk.reserve(words, words) != hipSuccess || H.d_w.reserve(words, words) != hipSuccess || H.d_sd.reserve(nv, nv) != hipSuccess
        || H.d_act.reserve(2u * (size_t)tiles, 2u * (size_t)tiles) != hipSuccess || S.reserve(3u, ij.size()) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VF_ERR_NOMEM, "spill buffer allocation failed");
    }
    const dim3 cols(tiles, kSpillTile / 4u), threads(256);
    const float *hblk = t->d_hblk;
    uint32_t *const runs = S.counts() + 2u;
    VF_HIP_TRY(hipMemsetAsync(S.counts(), 0, 3u * sizeof(uint32_t), s));
    if (S.mode == VF_SPILL_EDGES)
        hipLaunchKernelGGL((k_spill_init<true>), cols, threads, 0, s, n, t->nb, ftx, tiles, hblk, H.d_hk.p, H.d_w.p, H.d_act.p);
    else {
        hipLaunchKernelGGL((k_spill_init<false>), cols, threads, 0, s, n, t->nb, ftx, tiles, hblk, H.d_hk.p, H.d_w.p, H.d_act.p);
        const uint32_t count = (uint32_t)(ij.size() / 2u);
        VF_HIP_TRY(S.upload(ij, s));
        hipLaunchKernelGGL((k_spill_seed<0>), dim3((count + 255u) / 256u), threads, 0, s, n, ftx, (const uint32_t *)S.d_seeds.p, count,
                           (const uint32_t *)H.d_hk.p, H.d_w.p);
    }
    VF_HIP_TRY(hipGetLastError());
    uint32_t passes = 0;
    // (every pass that changes something lowers at least one vertex to one of the at most n x n keys of h: the relaxation ends; the
    //  bound is the issue's and guards the loop, it is not reached)
    if (int rc = S.fixpoint(s, nv, "spill relaxation did not reach a fixpoint within n x n + 1 passes", &passes, [&](uint32_t pass, uint32_t *changed) {
            // (pass p reads array p & 1 and sets words of the other one)
            hipLaunchKernelGGL((k_spill_pass<0>), dim3(tiles), dim3(64), 0, s, ftx, ftx, H.no_flags ? 1u : 0u, (const uint32_t *)H.d_hk.p, H.d_w.p,
                               H.d_act.p + (size_t)(pass & 1u) * tiles, H.d_act.p + (size_t)((pass + 1u) & 1u) * tiles, changed, runs);
        })) return rc;
    uint32_t tail[3] = {};
    hipLaunchKernelGGL((k_spill_out<0>), dim3(ftx, (n + 3u) / 4u), threads, 0, s, n, t->nb, ftx, hblk, (const uint32_t *)H.d_w.p, S.field.d.p, H.d_sd.p,
                       (unsigned long long *)S.counts());
    VF_HIP_TRY(hipGetLastError());
    VF_HIP_TRY(hipMemcpyAsync(tail, S.counts(), sizeof tail, hipMemcpyDeviceToHost, s));
    VF_HIP_TRY(hipStreamSynchronize(s));
    S.passes = passes; H.reached = tail[0]; H.sinks = tail[1]; H.tile_runs = tail[2];
    S.field.computed(t, key);
    return VF_OK;
}

static void spill_launch(const vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba)
{
    const vf_terrain::Spill &H = t->sp;
    SpillTint T = {};
    T.sd = H.d_sd.p; T.decode = t->ctx->d_decode;
    T.shallow_rgba = H.fill.shallow_rgba; T.deep_rgba = H.fill.deep_rgba; T.depth_full = H.fill.depth_full;
    tint_launch(t, s, P, V, redo, rgba, T, k_spill_tint<false>, k_spill_tint<true>);
}

// The sinks of a frame, on the draw stream behind the flood's water: the field if it is stale, then the tint pass over the covered pixels
static int spill_pass(vf_terrain *t, hipStream_t s, const FrameParams &P, const SetupView &V, const uint32_t *redo, uint32_t *rgba)
{
    return fill_pass(t, kFieldSpill, spill_launch, s, P, V, redo, rgba);
}

int vf_terrain_set_spill(vf_terrain *t, int enable, int mode, const float *seeds_xz, uint32_t count, const uint8_t shallow_rgba[4],
                         const uint8_t deep_rgba[4], float depth_full)
{
    if (!t || !shallow_rgba || !deep_rgba) return fail(VF_ERR_INVALID, "NULL argument");
    static const SeededFill::Words W = { 1 << VF_SPILL_EDGES | 1 << VF_SPILL_SEEDS, "unknown spill mode", "the spill takes 1 to 65535 seeds",
                                         "the spill needs a whole-frame handle: sharded handles are not supported" };
    return t->sp.fill.set(t, enable, mode, seeds_xz, count, shallow_rgba, deep_rgba, depth_full, false, W);
}

int vf_terrain_clear_spill(vf_terrain *t) { return fill_clear(t, spill_fill, spill_release); }
int vf_terrain_read_spill_field(vf_terrain *t, float *spill) { return field_out(t, kFieldSpill, spill, nullptr, nullptr); }
int vf_terrain_spill_field_device(vf_terrain *t, float *dev_spill, void *stream) { return field_out(t, kFieldSpill, nullptr, dev_spill, stream); }

// the public sink depth: sd where it is finite, 0 elsewhere (d_sd stands with the field that field_out has just made current)
int vf_terrain_read_sink_depth(vf_terrain *t, float *depth)
{
    if (!t || !depth) return fail(VF_ERR_INVALID, "NULL argument");
    const size_t nv = (size_t)t->n * t->n;
    std::vector<float> spill(nv);
    if (int rc = field_out(t, kFieldSpill, spill.data(), nullptr, nullptr)) return rc;
    VF_HIP_TRY(hipMemcpy(depth, t->sp.d_sd.p, nv * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < nv; ++k)
        if (!std::isfinite(depth[k])) depth[k] = 0.0f;
    return VF_OK;
}

int vf_terrain_spill_info(vf_terrain *t, vf_spill_info *out)
{
    if (!t || !out) return fail(VF_ERR_INVALID, "NULL argument");
    const vf_terrain::Spill &H = t->sp;
    *out = vf_spill_info();
    H.fill.info(out);
    out->has_spill = H.fill.have ? 1 : 0;
    out->reached_vertices = H.reached; out->sink_vertices = H.sinks; out->tile_runs = H.tile_runs;
    return VF_OK;
}

int vf_terrain_read_spill_seeds(vf_terrain *t, uint32_t *vertices)
{
    if (!t || !vertices) return fail(VF_ERR_INVALID, "NULL argument");
    return t->sp.fill.read_seeds(t, vertices, "no seeds set (vf_terrain_set_spill with VF_SPILL_SEEDS)");
}

int vf_terrain_debug_spill_scans(vf_terrain *t, uint32_t *count) { return field_scans(t, kFieldSpill, count); }

int vf_terrain_debug_spill_stage(vf_terrain *t, uint32_t repeats, float ms[2])
{
    return fill_stage(t, kFieldSpill, spill_fill, "spill", "no spill enabled (vf_terrain_set_spill)", spill_launch, repeats, ms);
}

int vf_terrain_debug_spill_group(vf_terrain *t, uint32_t group)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    const bool no_flags = (group & VF_SPILL_GROUP_NO_FLAGS) != 0u;
    if (int rc = t->sp.fill.force_group(group & ~VF_SPILL_GROUP_NO_FLAGS)) return rc;
    if (t->sp.no_flags != no_flags) t->sp.fill.field.valid = false;             // (the next call computes the field again)
    t->sp.no_flags = no_flags;
    return VF_OK;
}

// ---- Renderer DEM path -------------------------------------------------------------------------------------
} // extern "C"   (struct definition below is C++)

struct vf_dem {
    vf_ctx *ctx = nullptr;
    float *d_h = nullptr;        // heights (already multiplied by the exaggeration), w*h
    float *d_tex = nullptr;      // R32F "texture" written by upload_height_r32f
    void *d_stage = nullptr;     // staging for the ingest (raw f32 / f64 samples)
    size_t stage_bytes = 0;
    uint32_t w = 0, h = 0, tex_w = 0, tex_h = 0;
    size_t cap = 0, tex_cap = 0;
    uint32_t *d_mm = nullptr;    // min / max as ordered ints
    double *d_partial = nullptr; // one partial sum per reduction block
};
static constexpr int kDemBlocks = 2048;

extern "C" {

int vf_dem_create(vf_ctx *ctx, vf_dem **out)
{
    if (!ctx || !out) return fail(VF_ERR_INVALID, "NULL argument");
    VF_HIP_TRY(hipSetDevice(ctx->device));
    vf_dem *d = new (std::nothrow) vf_dem;
    if (!d) return fail(VF_ERR_NOMEM, "out of host memory");
    d->ctx = ctx;
    hipError_t e = hipMalloc(&d->d_mm, 2 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&d->d_partial, kDemBlocks * sizeof(double));
    if (e != hipSuccess) { vf_dem_destroy(d); return fail(VF_ERR_NOMEM, std::string("dem allocation failed: ") + hipGetErrorString(e)); }
    *out = d;
    return VF_OK;
}

void vf_dem_destroy(vf_dem *d)
{
    if (!d) return;
    (void)hipSetDevice(d->ctx->device);
    (void)hipDeviceSynchronize();
    void *ptrs[] = { d->d_h, d->d_tex, d->d_stage, d->d_mm, d->d_partial };
    for (void *p : ptrs) if (p) (void)hipFree(p);
    delete d;
}

} // extern "C"

template <typename T>
static int dem_ingest(vf_dem *d, const T *host, uint32_t w, uint32_t h, float exaggeration)
{
    if (!d || !host) return fail(VF_ERR_INVALID, "NULL argument");
    if (w == 0 || h == 0) return fail(VF_ERR_INVALID, "heightmap cannot be empty");
    VF_HIP_TRY(hipSetDevice(d->ctx->device));
    const size_t n = (size_t)w * h;
    if (n > d->cap) {
        if (d->d_h) VF_HIP_TRY(hipFree(d->d_h));
        d->d_h = nullptr; d->cap = 0;
        VF_HIP_TRY(hipMalloc(&d->d_h, n * sizeof(float)));
        d->cap = n;
    }
    if (n * sizeof(T) > d->stage_bytes) {
        if (d->d_stage) VF_HIP_TRY(hipFree(d->d_stage));
        d->d_stage = nullptr; d->stage_bytes = 0;
        VF_HIP_TRY(hipMalloc(&d->d_stage, n * sizeof(T)));
        d->stage_bytes = n * sizeof(T);
    }
    hipStream_t s = d->ctx->stream;
    VF_HIP_TRY(hipMemcpyAsync(d->d_stage, host, n * sizeof(T), hipMemcpyHostToDevice, s));
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_dem_ingest<T>, dim3(blocks), dim3(256), 0, s, (const T *)d->d_stage, d->d_h, n, exaggeration);
    VF_HIP_TRY(hipGetLastError());
    VF_HIP_TRY(hipStreamSynchronize(s));     // the host buffer is only borrowed for this call
    d->w = w; d->h = h;
    return VF_OK;
}

extern "C" {

int vf_dem_set_heights_f32(vf_dem *d, const float *host, uint32_t w, uint32_t h, float ex) { return dem_ingest<float>(d, host, w, h, ex); }
int vf_dem_set_heights_f64(vf_dem *d, const double *host, uint32_t w, uint32_t h, float ex) { return dem_ingest<double>(d, host, w, h, ex); }

static int dem_stats_impl(vf_dem *d, float out[4])
{
    if (!d->d_h || d->w == 0) return fail(VF_ERR_INVALID, "no terrain uploaded; call add_terrain() first");
    VF_HIP_TRY(hipSetDevice(d->ctx->device));
    const size_t n = (size_t)d->w * d->h;
    hipStream_t s = d->ctx->stream;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)kDemBlocks);
    const uint32_t init[2] = { 0xFFFFFFFFu, 0u };
    VF_HIP_TRY(hipMemcpyAsync(d->d_mm, init, sizeof init, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_dem_minmaxsum, dim3(blocks), dim3(256), 0, s, d->d_h, n, d->d_mm, d->d_partial);
    VF_HIP_TRY(hipGetLastError());
    std::vector<double> part(blocks);
    uint32_t mm[2];
    VF_HIP_TRY(hipMemcpyAsync(part.data(), d->d_partial, blocks * sizeof(double), hipMemcpyDeviceToHost, s));
    VF_HIP_TRY(hipMemcpyAsync(mm, d->d_mm, sizeof mm, hipMemcpyDeviceToHost, s));
    VF_HIP_TRY(hipStreamSynchronize(s));
    double sum = 0.0;
    for (double v : part) sum += v;
    const float mean = (float)(sum / (double)n);
    hipLaunchKernelGGL(k_dem_sqdev, dim3(blocks), dim3(256), 0, s, d->d_h, n, mean, d->d_partial);
    VF_HIP_TRY(hipGetLastError());
    VF_HIP_TRY(hipMemcpyAsync(part.data(), d->d_partial, blocks * sizeof(double), hipMemcpyDeviceToHost, s));
    VF_HIP_TRY(hipStreamSynchronize(s));
    double var = 0.0;
    for (double v : part) var += v;
    auto unorder = [](uint32_t u) { uint32_t b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u; float f; std::memcpy(&f, &b, 4); return f; };
    // a NaN first sample leaves 0 / 0xFFFFFFFF (k_dem_minmaxsum), which unorder to NaNs by themselves: the reference reports its first
    // element then.  The init pattern survives no map (sample 0 is a number or a NaN); it is mapped to NaN all the same.
    out[0] = mm[0] == 0xFFFFFFFFu ? NAN : unorder(mm[0]);
    out[1] = mm[1] == 0u ? NAN : unorder(mm[1]);
    out[2] = mean;
    out[3] = std::sqrt((float)(var / (double)n));
    return VF_OK;
}
int vf_dem_stats(vf_dem *d, float out[4])
{
    if (!d || !out) return fail(VF_ERR_INVALID, "NULL argument");
    return dem_stats_impl(d, out);
}

int vf_dem_percentile_range(vf_dem *d, float *p1, float *p99)
{
    if (!d || !p1 || !p99) return fail(VF_ERR_INVALID, "NULL argument");
    if (!d->d_h || d->w == 0) return fail(VF_ERR_INVALID, "no terrain uploaded; call add_terrain() first");
    VF_HIP_TRY(hipSetDevice(d->ctx->device));
    const size_t n = (size_t)d->w * d->h, SAMPLE = 65536;
    const size_t step = n > SAMPLE ? n / SAMPLE : 1;                 // src/terrain_stats.rs:24-29
    const size_t m = (n + step - 1) / step;                          // iter().step_by(step).count()
    std::vector<float> buf(m);
    hipStream_t s = d->ctx->stream;
    if (step == 1) {
        VF_HIP_TRY(hipMemcpyAsync(buf.data(), d->d_h, n * sizeof(float), hipMemcpyDeviceToHost, s));
    } else {
        if (m * sizeof(float) > d->stage_bytes) {
            if (d->d_stage) VF_HIP_TRY(hipFree(d->d_stage));
            d->d_stage = nullptr; d->stage_bytes = 0;
            VF_HIP_TRY(hipMalloc(&d->d_stage, m * sizeof(float)));
            d->stage_bytes = m * sizeof(float);
        }
        hipLaunchKernelGGL(k_dem_sample, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, d->d_h, n, step, (float *)d->d_stage, m);
        VF_HIP_TRY(hipGetLastError());
        VF_HIP_TRY(hipMemcpyAsync(buf.data(), d->d_stage, m * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    VF_HIP_TRY(hipStreamSynchronize(s));
    // the sample is at most ~131071 values: ordering it is host logic, exactly like the reference's sort_by
    std::stable_sort(buf.begin(), buf.end(), [](float a, float b) { return a < b; });
    *p1 = buf[(size_t)((float)buf.size() * 0.01f)];
    *p99 = buf[(size_t)((float)buf.size() * 0.99f)];
    return VF_OK;
}

int vf_dem_normalize(vf_dem *d, int mode, float lo, float hi, float eps)
{
    if (!d) return fail(VF_ERR_INVALID, "NULL argument");
    if (mode != 0 && mode != 1) return fail(VF_ERR_INVALID, "mode must be 'minmax' or 'zscore'");
    float st[4];
    int rc = dem_stats_impl(d, st);
    if (rc != VF_OK) return rc;
    const size_t n = (size_t)d->w * d->h;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipStream_t s = d->ctx->stream;
    if (mode == 0) {
        const float denom = std::fmax(std::fabs(st[1] - st[0]), eps);    // src/lib.rs:938-939
        const float scale = (hi - lo) / denom;
        hipLaunchKernelGGL(k_dem_normalize, dim3(blocks), dim3(256), 0, s, d->d_h, n, 0, st[0], scale, lo);
    } else {
        const float denom = std::fmax(st[3], eps);                       // :945
        hipLaunchKernelGGL(k_dem_normalize, dim3(blocks), dim3(256), 0, s, d->d_h, n, 1, st[2], denom, 0.0f);
    }
    VF_HIP_TRY(hipGetLastError());
    VF_HIP_TRY(hipStreamSynchronize(s));
    return VF_OK;
}

int vf_dem_upload_height(vf_dem *d)
{
    if (!d) return fail(VF_ERR_INVALID, "NULL argument");
    if (!d->d_h || d->w == 0) return fail(VF_ERR_INVALID, "no terrain uploaded; call add_terrain() first");
    VF_HIP_TRY(hipSetDevice(d->ctx->device));
    const size_t n = (size_t)d->w * d->h;
    if (n > d->tex_cap) {
        if (d->d_tex) VF_HIP_TRY(hipFree(d->d_tex));
        d->d_tex = nullptr; d->tex_cap = 0;
        VF_HIP_TRY(hipMalloc(&d->d_tex, n * sizeof(float)));
        d->tex_cap = n;
    }
    VF_HIP_TRY(hipMemcpyAsync(d->d_tex, d->d_h, n * sizeof(float), hipMemcpyDeviceToDevice, d->ctx->stream));
    VF_HIP_TRY(hipStreamSynchronize(d->ctx->stream));
    d->tex_w = d->w; d->tex_h = d->h;
    return VF_OK;
}

int vf_dem_texture_size(const vf_dem *d, uint32_t *w, uint32_t *h)
{
    if (!d || !w || !h) return fail(VF_ERR_INVALID, "NULL argument");
    *w = d->tex_w; *h = d->tex_h;
    return VF_OK;
}

int vf_dem_read_patch(vf_dem *d, uint32_t x, uint32_t y, uint32_t w, uint32_t h, float *dst)
{
    if (!d || !dst) return fail(VF_ERR_INVALID, "NULL argument");
    if (w == 0 || h == 0) return fail(VF_ERR_INVALID, "patch dimensions must be > 0");
    if (!d->d_tex) return fail(VF_ERR_INVALID, "no height texture uploaded; call upload_height_r32f() first");
    if ((uint64_t)x + w > d->tex_w)
        return fail(VF_ERR_INVALID, "requested patch exceeds texture bounds in x: x+w (" + std::to_string((uint64_t)x + w) + ") > width (" + std::to_string(d->tex_w) + ")");
    if ((uint64_t)y + h > d->tex_h)
        return fail(VF_ERR_INVALID, "requested patch exceeds texture bounds in y: y+h (" + std::to_string((uint64_t)y + h) + ") > height (" + std::to_string(d->tex_h) + ")");
    VF_HIP_TRY(hipSetDevice(d->ctx->device));
    VF_HIP_TRY(hipMemcpy2D(dst, (size_t)w * 4, d->d_tex + (size_t)y * d->tex_w + x, (size_t)d->tex_w * 4, (size_t)w * 4, h, hipMemcpyDeviceToHost));
    return VF_OK;
}

int vf_stitch_bands_device(vf_ctx *ctx, const void *dev_gathered, void *dev_image, uint32_t width, uint32_t height,
                           uint32_t nranks, uint32_t band_h, void *stream)
{
    if (!ctx || !dev_gathered || !dev_image) return fail(VF_ERR_INVALID, "NULL argument");
    if (!is_pow2(band_h) || nranks == 0) return fail(VF_ERR_INVALID, "band_h must be a power of two, nranks > 0");
    if (width % 4 != 0) return fail(VF_ERR_INVALID, "width must be a multiple of 4");
    if (height % (band_h * nranks) != 0) return fail(VF_ERR_INVALID, "height must be a multiple of band_h*nranks");
    VF_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    uint32_t row_vec4 = width / 4;
    size_t nvec = (size_t)height * row_vec4;
    hipLaunchKernelGGL(k_stitch_bands, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s, (const uint4 *)dev_gathered,
                       (uint4 *)dev_image, row_vec4, height, nranks, ilog2(band_h), band_h, height / nranks);
    VF_HIP_TRY(hipGetLastError());
    return VF_OK;
}

int vf_stitch_tiles_device(vf_ctx *ctx, const void *dev_gathered, void *dev_image, uint32_t width, uint32_t height,
                           uint32_t nranks, uint32_t skew, uint32_t stride_tiles, void *stream)
{
    if (!ctx || !dev_gathered || !dev_image) return fail(VF_ERR_INVALID, "NULL argument");
    if (width == 0 || height == 0 || nranks == 0) return fail(VF_ERR_INVALID, "empty frame or nranks == 0");
    const uint32_t ntx = (width + kTileW - 1) / kTileW, nty = (height + kTileH - 1) / kTileH;
    uint32_t most = 0;
    for (uint32_t r = 0; r < nranks; ++r) {
        uint32_t n = 0;
        int rc = vf_tile_layout(width, height, r, nranks, skew, nullptr, 0, &n);
        if (rc != VF_OK) return rc;
        most = n > most ? n : most;
    }
    if (stride_tiles < most) return fail(VF_ERR_INVALID, "stride_tiles is smaller than the largest shard");
    VF_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    // persistent, about one small workgroup per CU (VF_STITCH_WGS overrides): it has to fit beside the next frame's tile kernel
    uint32_t wgs = (uint32_t)std::max(1, ctx->prop.multiProcessorCount);
    if (const char *e = std::getenv("VF_STITCH_WGS")) wgs = (uint32_t)std::max(1, std::atoi(e));
    const uint8_t *d_owner = nullptr;
    if (const StripeMap *m = layout_map(skew)) {            // a registered stripe map: its owner table on this device (uploaded once per context)
        const uint32_t id = (skew >> 21) & 0x3Fu;
        std::lock_guard<std::mutex> lk(ctx->lazy_mu);
        if (!ctx->d_maps) VF_HIP_TRY(hipMalloc(&ctx->d_maps, (size_t)kMaxStripeMaps * kMaxStripes));
        if (!((ctx->maps_uploaded >> id) & 1ull)) {
            VF_HIP_TRY(hipMemcpy(ctx->d_maps + (size_t)id * kMaxStripes, m->owner.data(), m->owner.size(), hipMemcpyHostToDevice));
            ctx->maps_uploaded |= 1ull << id;
        }
        d_owner = ctx->d_maps + (size_t)id * kMaxStripes;
    }
    hipLaunchKernelGGL(k_stitch_tiles, dim3(std::min(ntx * nty, wgs)), dim3(256), 0, s, (const uint32_t *)dev_gathered, (uint32_t *)dev_image, width, height,
                       ntx, nty, nranks, layout_skew(skew), layout_shift(skew), stride_tiles, d_owner);
    VF_HIP_TRY(hipGetLastError());
    return VF_OK;
}

} // extern "C"

// ---- multi-GPU exchange over RCCL ---------------------------------------------------------------------------------------
namespace {
struct Rccl {
    bool ok = false;
    std::string why;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*CommCuDevice)(const ncclComm_t, int *) = nullptr;   // (optional)
    ncclResult_t (*GetVersion)(int *) = nullptr;                       // (optional)
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
// librccl.so.1 as already loaded in the process (PyTorch brings its own copy; a second one would not share its state), else
// the ROCm installation's through this library's run path
const Rccl &resolve_rccl()
{
    static const Rccl r = [] {
        Rccl x;
        void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) { x.why = std::string("RCCL not found: ") + (dlerror() ? dlerror() : "dlopen failed"); return x; }
        bool all = true;
        auto sym = [&](const char *name) { void *p = dlsym(h, name); if (!p) { all = false; x.why = std::string("RCCL lacks ") + name; } return p; };
        x.GetUniqueId = reinterpret_cast<decltype(x.GetUniqueId)>(sym("ncclGetUniqueId"));
        x.CommInitRank = reinterpret_cast<decltype(x.CommInitRank)>(sym("ncclCommInitRank"));
        x.CommDestroy = reinterpret_cast<decltype(x.CommDestroy)>(sym("ncclCommDestroy"));
        x.CommCount = reinterpret_cast<decltype(x.CommCount)>(sym("ncclCommCount"));
        x.CommUserRank = reinterpret_cast<decltype(x.CommUserRank)>(sym("ncclCommUserRank"));
        x.CommCuDevice = reinterpret_cast<decltype(x.CommCuDevice)>(dlsym(h, "ncclCommCuDevice"));
        x.GetVersion = reinterpret_cast<decltype(x.GetVersion)>(dlsym(h, "ncclGetVersion"));
        x.GroupStart = reinterpret_cast<decltype(x.GroupStart)>(sym("ncclGroupStart"));
        x.GroupEnd = reinterpret_cast<decltype(x.GroupEnd)>(sym("ncclGroupEnd"));
        x.Send = reinterpret_cast<decltype(x.Send)>(sym("ncclSend"));
        x.Recv = reinterpret_cast<decltype(x.Recv)>(sym("ncclRecv"));
        x.GetErrorString = reinterpret_cast<decltype(x.GetErrorString)>(sym("ncclGetErrorString"));
        x.ok = all;
        return x;
    }();
    return r;
}
#define VF_RCCL_TRY(R, expr)                                                                                   \
    do {                                                                                                       \
        ncclResult_t r_ = (expr);                                                                              \
        if (r_ != ncclSuccess) return fail(VF_ERR_HIP, std::string(#expr) + ": " + (R).GetErrorString(r_));   \
    } while (0)

// rank and size of the communicator must be the handle's shard: a mismatch would exchange the wrong slabs silently
int check_comm(const Rccl &R, const vf_terrain *t, void *comm, int root)
{
    if (!R.ok) return fail(VF_ERR_HIP, R.why);
    if (!comm) return fail(VF_ERR_INVALID, "communicator is NULL");
    int n = 0, r = -1;
    VF_RCCL_TRY(R, R.CommCount((ncclComm_t)comm, &n));
    VF_RCCL_TRY(R, R.CommUserRank((ncclComm_t)comm, &r));
    if ((uint32_t)n != t->nranks || (uint32_t)r != t->rank) return fail(VF_ERR_INVALID, "communicator rank/size differ from the handle's shard");
    if (root < 0 || root >= n) return fail(VF_ERR_INVALID, "root must be a rank of the communicator");
    return VF_OK;
}
} // namespace

extern "C" {

int vf_dist_available(void) { return resolve_rccl().ok ? 1 : 0; }

int vf_dist_version(int *version)
{
    if (!version) return fail(VF_ERR_INVALID, "NULL argument");
    *version = 0;
    const Rccl &R = resolve_rccl();
    if (!R.ok) return fail(VF_ERR_HIP, R.why);
    if (!R.GetVersion) return fail(VF_ERR_HIP, "RCCL lacks ncclGetVersion");
    VF_RCCL_TRY(R, R.GetVersion(version));
    return VF_OK;
}

int vf_dist_unique_id(uint8_t id[VF_DIST_UNIQUE_ID_BYTES])
{
    if (!id) return fail(VF_ERR_INVALID, "NULL argument");
    const Rccl &R = resolve_rccl();
    if (!R.ok) return fail(VF_ERR_HIP, R.why);
    static_assert(sizeof(ncclUniqueId) == VF_DIST_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    VF_RCCL_TRY(R, R.GetUniqueId(&u));
    std::memcpy(id, u.internal, sizeof u.internal);
    return VF_OK;
}

int vf_dist_comm_init(vf_ctx *ctx, const uint8_t id[VF_DIST_UNIQUE_ID_BYTES], int rank, int nranks, void **comm)
{
    if (!ctx || !id || !comm) return fail(VF_ERR_INVALID, "NULL argument");
    *comm = nullptr;
    if (nranks <= 0 || rank < 0 || rank >= nranks) return fail(VF_ERR_INVALID, "rank must be < nranks");
    const Rccl &R = resolve_rccl();
    if (!R.ok) return fail(VF_ERR_HIP, R.why);
    VF_HIP_TRY(hipSetDevice(ctx->device));
    ncclUniqueId u;
    std::memcpy(u.internal, id, sizeof u.internal);
    ncclComm_t c = nullptr;
    VF_RCCL_TRY(R, R.CommInitRank(&c, nranks, u, rank));
    *comm = c;
    return VF_OK;
}

void vf_dist_comm_destroy(void *comm)
{
    const Rccl &R = resolve_rccl();
    if (!R.ok || !comm) return;
    int dev = -1, was = -1;                                 // the communicator's own device, whatever the calling thread has current ...
    const bool have_was = hipGetDevice(&was) == hipSuccess;
    if (R.CommCuDevice && R.CommCuDevice((ncclComm_t)comm, &dev) == ncclSuccess && dev >= 0) (void)hipSetDevice(dev);
    (void)R.CommDestroy((ncclComm_t)comm);
    if (have_was && was >= 0) (void)hipSetDevice(was);     // ... which is the caller's again afterwards
}

int vf_dist_gather_tiles(vf_terrain *t, void *rccl_comm, int root, void *dev_gathered, uint32_t stride_tiles, void *stream)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->shard_tiles) return fail(VF_ERR_INVALID, "handle is not tile-sharded");
    if (!t->rendered) return fail(VF_ERR_INVALID, "nothing rendered yet");
    const Rccl &R = resolve_rccl();
    int rc = check_comm(R, t, rccl_comm, root);
    if (rc != VF_OK) return rc;
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    ncclComm_t comm = (ncclComm_t)rccl_comm;
    hipStream_t s = stream ? (hipStream_t)stream : t->ctx->stream;
    if (s != t->last_stream && t->last_stream) {            // the slab is being drawn on another stream: order the exchange after it
        VF_HIP_TRY(hipStreamWaitEvent(s, t->ps[t->last_set].drawn, 0));
    }
    const size_t tile_bytes = (size_t)kTileW * kTileH * 4;
    const bool is_root = (uint32_t)root == t->rank;
    // Checked on EVERY rank, from what every rank can compute locally, before anything is posted: a rank that returned here
    // while the others had queued their ncclSend would leave them waiting for a receive that never comes.  (The one check only
    // the root can make -- its gather buffer -- must hold by construction: a root that passes NULL fails alone and the senders
    // hang; vf_hip.h says so.)
    for (uint32_t r = 0; r < t->nranks; ++r) {
        uint32_t n = 0;
        rc = vf_tile_layout(t->W, t->H, r, t->nranks, t->skew, nullptr, 0, &n);
        if (rc != VF_OK) return rc;
        if (n > stride_tiles) return fail(VF_ERR_INVALID, "stride_tiles is smaller than the largest shard");
    }
    if (is_root && !dev_gathered) return fail(VF_ERR_INVALID, "the root needs the gather buffer");
    uint8_t *const slots = (uint8_t *)dev_gathered;
    uint8_t *const own_slot = is_root ? slots + (size_t)root * stride_tiles * tile_bytes : nullptr;
    const bool in_place = is_root && (uint8_t *)t->d_rgba == own_slot;
    VF_RCCL_TRY(R, R.GroupStart());
    ncclResult_t res = ncclSuccess;
    if (is_root) {
        for (uint32_t r = 0; r < t->nranks && res == ncclSuccess; ++r) {
            if (r == t->rank && in_place) continue;         // the root drew straight into its slot
            uint32_t n = 0;
            (void)vf_tile_layout(t->W, t->H, r, t->nranks, t->skew, nullptr, 0, &n);
            if (n) res = R.Recv(slots + (size_t)r * stride_tiles * tile_bytes, (size_t)n * tile_bytes, ncclUint8, (int)r, comm, s);
        }
    }
    if (res == ncclSuccess && (!is_root || !in_place) && t->local_tiles)
        res = R.Send(t->d_rgba, (size_t)t->local_tiles * tile_bytes, ncclUint8, root, comm, s);
    const ncclResult_t end = R.GroupEnd();
    if (res != ncclSuccess) return fail(VF_ERR_HIP, std::string("ncclSend/ncclRecv: ") + R.GetErrorString(res));
    if (end != ncclSuccess) return fail(VF_ERR_HIP, std::string("ncclGroupEnd: ") + R.GetErrorString(end));
    return VF_OK;
}

int vf_dist_gather_bands(vf_terrain *t, void *rccl_comm, int root, void *dev_image, void *stream)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (t->shard_tiles) return fail(VF_ERR_INVALID, "handle is tile-sharded: gather with vf_dist_gather_tiles");
    if (t->ss > 1u) return fail(VF_ERR_INVALID, "the handle is supersampled: it is a whole-frame handle, there are no bands to gather");
    if (!t->rendered) return fail(VF_ERR_INVALID, "nothing rendered yet");
    const Rccl &R = resolve_rccl();
    int rc = check_comm(R, t, rccl_comm, root);
    if (rc != VF_OK) return rc;
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    ncclComm_t comm = (ncclComm_t)rccl_comm;
    hipStream_t s = stream ? (hipStream_t)stream : t->ctx->stream;
    if (s != t->last_stream && t->last_stream) VF_HIP_TRY(hipStreamWaitEvent(s, t->ps[t->last_set].drawn, 0));
    const bool is_root = (uint32_t)root == t->rank;
    if (is_root && !dev_image) return fail(VF_ERR_INVALID, "the root needs the image buffer");
    const size_t row_bytes = (size_t)t->W * 4;
    std::vector<uint32_t> local(t->nranks, 0u);             // rows a rank has stored so far, band by band
    // the root's own bands first, as plain device copies on the stream: nothing but RCCL calls inside the group
    if (is_root) {
        uint32_t ly0 = 0;
        for (uint32_t b = t->rank; b * t->band_h < t->H; b += t->nranks) {
            const uint32_t y0 = b * t->band_h, rows = std::min(t->band_h, t->H - y0);
            uint8_t *dst = (uint8_t *)dev_image + (size_t)y0 * row_bytes;
            const uint8_t *src = (const uint8_t *)t->d_rgba + (size_t)ly0 * row_bytes;
            if ((const uint8_t *)dst != src) VF_HIP_TRY(hipMemcpyAsync(dst, src, rows * row_bytes, hipMemcpyDeviceToDevice, s));
            ly0 += rows;
        }
    }
    VF_RCCL_TRY(R, R.GroupStart());
    ncclResult_t res = ncclSuccess;
    for (uint32_t b = 0; b * t->band_h < t->H && res == ncclSuccess; ++b) {
        const uint32_t y0 = b * t->band_h, rows = std::min(t->band_h, t->H - y0), owner = b % t->nranks, ly0 = local[owner];
        local[owner] += rows;
        uint8_t *dst = is_root ? (uint8_t *)dev_image + (size_t)y0 * row_bytes : nullptr;
        const uint8_t *src = (const uint8_t *)t->d_rgba + (size_t)ly0 * row_bytes;
        if (owner == t->rank && is_root) continue;          // copied above
        else if (is_root) res = R.Recv(dst, rows * row_bytes, ncclUint8, (int)owner, comm, s);
        else if (owner == t->rank) res = R.Send(src, rows * row_bytes, ncclUint8, root, comm, s);
    }
    const ncclResult_t end = R.GroupEnd();
    if (res != ncclSuccess) return fail(VF_ERR_HIP, std::string("ncclSend/ncclRecv: ") + R.GetErrorString(res));
    if (end != ncclSuccess) return fail(VF_ERR_HIP, std::string("ncclGroupEnd: ") + R.GetErrorString(end));
    return VF_OK;
}

// Tile shards (column stripes: skew 0) -> the row-major frame on rank `root` without any rank copying the whole frame: the stitch is
// sharded like the rendering.  (The steps are those of vulkan_forge_amd/dist.py::BandStitchExchange, here on RCCL directly.)
int vf_dist_exchange_bands(vf_terrain *t, void *rccl_comm, int root, void *dev_image, void *stream)
{
    if (!t) return fail(VF_ERR_INVALID, "NULL argument");
    if (!t->shard_tiles) return fail(VF_ERR_INVALID, "handle is not tile-sharded");
    if (!t->rendered) return fail(VF_ERR_INVALID, "nothing rendered yet");
    const Rccl &R = resolve_rccl();
    int rc = check_comm(R, t, rccl_comm, root);
    if (rc != VF_OK) return rc;
    const uint32_t N = t->nranks;
    // every rank can check the layout for itself, before anything is posted: all ranks fail together
    if (layout_skew(t->skew) != 0u) return fail(VF_ERR_INVALID, "the band exchange needs column stripes (tile shard with skew 0)");
    if (t->W % (uint32_t)kTileW || t->H % (uint32_t)kTileH || t->ntx % (N << layout_shift(t->skew)) || t->nty % N)
        return fail(VF_ERR_INVALID, "the band exchange needs whole tiles, stripes that divide the tile columns evenly among the ranks and tile rows that divide by the number of ranks");
    const bool is_root = (uint32_t)root == t->rank;
    if (is_root && !dev_image) return fail(VF_ERR_INVALID, "the root needs the image buffer");
    VF_HIP_TRY(hipSetDevice(t->ctx->device));
    ncclComm_t comm = (ncclComm_t)rccl_comm;
    hipStream_t s = stream ? (hipStream_t)stream : t->ctx->stream;
    if (s != t->last_stream && t->last_stream) VF_HIP_TRY(hipStreamWaitEvent(s, t->ps[t->last_set].drawn, 0));
    const size_t tile_bytes = (size_t)kTileW * kTileH * 4;
    const uint32_t band_tile_rows = t->nty / N, chunk_tiles = band_tile_rows * (t->ntx / N);   // tiles one rank holds of one band
    const size_t chunk_bytes = (size_t)chunk_tiles * tile_bytes;
    const uint32_t band_rows = t->H / N;
    const size_t band_bytes = (size_t)band_rows * t->W * 4;
    // the handle's own staging: what this rank receives ([N][chunk_tiles] tile slots) and, off the root, the band it stitches.
    // Reused by every call: calls on one handle are ordered on one stream (or by the caller's events).
    if (t->xrecv_bytes < chunk_bytes * N) {
        if (t->d_xrecv) { VF_HIP_TRY(hipStreamSynchronize(s)); (void)hipFree(t->d_xrecv); t->d_xrecv = nullptr; t->xrecv_bytes = 0; }
        hipError_t e = hipMalloc(&t->d_xrecv, chunk_bytes * N);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? VF_ERR_NOMEM : VF_ERR_HIP, std::string("exchange buffer: ") + hipGetErrorString(e));
        t->xrecv_bytes = chunk_bytes * N;
    }
    if (!is_root && t->xband_bytes < band_bytes) {
        if (t->d_xband) { VF_HIP_TRY(hipStreamSynchronize(s)); (void)hipFree(t->d_xband); t->d_xband = nullptr; t->xband_bytes = 0; }
        hipError_t e = hipMalloc(&t->d_xband, band_bytes);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? VF_ERR_NOMEM : VF_ERR_HIP, std::string("exchange buffer: ") + hipGetErrorString(e));
        t->xband_bytes = band_bytes;
    }
    // 1. all-to-all: a rank's slab lists its tiles row-major by (ty, tx), so the tiles of band b are the contiguous chunk b; it goes
    //    to rank b -- 1 / N of a slab per peer, every xGMI link busy in both directions, none a hot spot.  (Own chunk: a device copy.)
    const uint8_t *slab = (const uint8_t *)t->d_rgba;
    // (a one-rank communicator sends its only chunk through RCCL to itself: the loop-back test then exercises the very calls N ranks make)
    if (N > 1u) VF_HIP_TRY(hipMemcpyAsync(t->d_xrecv + (size_t)t->rank * chunk_bytes, slab + (size_t)t->rank * chunk_bytes, chunk_bytes, hipMemcpyDeviceToDevice, s));
    {
        VF_RCCL_TRY(R, R.GroupStart());
        ncclResult_t res = ncclSuccess;
        for (uint32_t r = 0; r < N && res == ncclSuccess; ++r) {
            if (r == t->rank && N > 1u) continue;
            res = R.Send(slab + (size_t)r * chunk_bytes, chunk_bytes, ncclUint8, (int)r, comm, s);
            if (res == ncclSuccess) res = R.Recv(t->d_xrecv + (size_t)r * chunk_bytes, chunk_bytes, ncclUint8, (int)r, comm, s);
        }
        const ncclResult_t end = R.GroupEnd();
        if (res != ncclSuccess) return fail(VF_ERR_HIP, std::string("ncclSend/ncclRecv: ") + R.GetErrorString(res));
        if (end != ncclSuccess) return fail(VF_ERR_HIP, std::string("ncclGroupEnd: ") + R.GetErrorString(end));
    }
    // 2. every rank stitches ITS band (a frame of H / N rows whose tile (tx, ty) sits in slot [tx % N][ty * (ntx / N) + tx / N]):
    //    1 / N of the copy each; the root writes its band straight into the image
    uint8_t *const band = is_root ? (uint8_t *)dev_image + (size_t)t->rank * band_bytes : t->d_xband;
    rc = vf_stitch_tiles_device(t->ctx, t->d_xrecv, band, t->W, band_rows, N, t->skew, chunk_tiles, s);
    if (rc != VF_OK) return rc;
    // 3. the bands are contiguous slabs of the final image: the root receives them in place
    if (N > 1u) {
        VF_RCCL_TRY(R, R.GroupStart());
        ncclResult_t res = ncclSuccess;
        if (is_root) {
            for (uint32_t r = 0; r < N && res == ncclSuccess; ++r)
                if (r != t->rank) res = R.Recv((uint8_t *)dev_image + (size_t)r * band_bytes, band_bytes, ncclUint8, (int)r, comm, s);
        } else res = R.Send(band, band_bytes, ncclUint8, root, comm, s);
        const ncclResult_t end = R.GroupEnd();
        if (res != ncclSuccess) return fail(VF_ERR_HIP, std::string("ncclSend/ncclRecv: ") + R.GetErrorString(res));
        if (end != ncclSuccess) return fail(VF_ERR_HIP, std::string("ncclGroupEnd: ") + R.GetErrorString(end));
    }
    return VF_OK;
}

} // extern "C"

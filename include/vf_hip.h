/*
 * vf_hip.h -- C-ABI of the MI355X-native terrain rasteriser (libvf_hip.so).
 *
 * This is the drop-in boundary underneath the reference's `_vulkan_forge` extension module:
 * plain pointers and sizes, opaque handles, int status codes; no C++/torch/pybind types.
 * The reference has no C-ABI of its own (its boundary is PyO3, src/lib.rs:961-976); each entry
 * point below cites the reference code it replaces.  A Rust host (as BASELINE.json's north_star
 * words it) binds this header with `extern "C"` unchanged -- see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns VF_OK (0) or a negative VF_ERR_* code; vf_last_error() returns a
 *     thread-local, NUL-terminated description of the last failure on the calling thread.
 *   - host buffers are caller-owned and only borrowed for the duration of the call; device
 *     buffers passed to *_device entry points are borrowed until replaced or the object dies.
 *   - `stream` arguments are `hipStream_t` passed as `void*`; NULL = the object's own stream (a non-blocking stream of the context:
 *     NOT the legacy default stream -- a host that orders its own work by "the default stream", whose raw handle is 0 in HIP and in
 *     torch.cuda, must create an explicit stream and pass that, or synchronise with vf_terrain_sync).
 *     Calls on one handle are not re-entrant.  Rendering is asynchronous on the stream; the
 *     read_* entry points synchronise.
 *   - no CPU fallback exists: without a HIP device vf_ctx_create fails with VF_ERR_NO_DEVICE.
 */
#ifndef VF_HIP_H
#define VF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VF_OK 0
#define VF_ERR_NO_DEVICE (-1) /* no HIP device / runtime: reference message "No suitable GPU adapter" (src/terrain/mod.rs:285) */
#define VF_ERR_HIP (-2)       /* a HIP runtime call failed */
#define VF_ERR_INVALID (-3)   /* bad argument */
#define VF_ERR_NOMEM (-4)

typedef struct vf_ctx vf_ctx;         /* one HIP device + default stream; replaces the wgpu Instance/Adapter/Device/Queue
                                         (src/terrain/mod.rs:277-294, src/scene/mod.rs:62-70, src/lib.rs:23-61) */
typedef struct vf_terrain vf_terrain; /* render target + pipeline state + mesh + bind groups of TerrainSpike/Scene
                                         (src/terrain/mod.rs:221-253, src/scene/mod.rs:25-55) */

typedef struct vf_device_info {
    char name[256];
    char arch[64];          /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
    int32_t device_ordinal;
    int32_t compute_units;
    int32_t wavefront_size;
    int32_t clock_khz;
    uint64_t total_mem_bytes;
    uint64_t lds_bytes_per_cu;
    int32_t pci_bus_id;
    int32_t pci_device_id;
} vf_device_info;

/* device time (HIP events), averaged over the frames rendered since vf_terrain_enable_timing(t, 1 or 2) -- at most the last 64.
 * A frame's plan kernels run on a stream of the handle's own and overlap the previous frame's tile kernel, so the first two
 * figures are elapsed times on that stream (they include waiting for free CUs when frames are rendered back to back). */
typedef struct vf_timings {
    float ranges_ms;    /* k_block_boxes (per-block pixel boxes and capsules) up to the launch of k_block_setup (the plan's stream, elapsed) */
    float plan_ms;      /* k_plan + k_plan_sort: background flags, busy-tile list, heaviest first (the plan's stream, elapsed); both: the last
                         * plan of each of the handle's two plan states (round 6: a plan may be queued ahead of its frame's call) */
    float tile_ms;      /* k_clear + k_tile (both variants) on the caller's stream: background clear, LDS raster from the set-up pass's records, fragment stage */
    float total_ms;     /* frame period when >= 2 frames were timed back to back, else plan start -> RGBA8 complete */
    uint32_t blocks_rasterised; /* (tile, block) pairs the tile kernel processed (after early-out); 0 at timing level 2 */
    uint32_t tiles;             /* workgroups launched = owned screen tiles */
    uint32_t frames;            /* frames averaged */
    uint32_t blocks_distinct;   /* distinct grid blocks behind blocks_rasterised in the last frame (of grid blocks in total: ceil((n-1)/8)^2) */
} vf_timings;

const char *vf_last_error(void);

/* ---- context ----------------------------------------------------------------------------- */
/* replaces wgpu adapter enumeration (src/lib.rs:746-777) */
int vf_device_count(int *count);
int vf_device_query(int device_ordinal, vf_device_info *out);
/* replaces Instance::new + request_adapter + request_device (src/terrain/mod.rs:277-294) */
int vf_ctx_create(int device_ordinal, vf_ctx **out);
void vf_ctx_destroy(vf_ctx *ctx);
int vf_ctx_device_info(const vf_ctx *ctx, vf_device_info *out);
/* The context's own stream (what a NULL `stream` argument means), as a hipStream_t: for a host that wants to order its own work
 * -- events, copies, collectives -- on the stream the frames are drawn on without creating one more (torch:
 * torch.cuda.ExternalStream(handle)).  Streams are a scarce resource here: the HIP runtime maps them onto GPU_MAX_HW_QUEUES
 * hardware queues (default 4) round-robin, a handle uses three (this one and two of its own for the next frame's plan and set-up
 * pass), and two streams that land on one queue run their kernels one after the other -- the next frame's set-up then no longer
 * hides under this frame's tile kernel (C4: 0.87 -> 0.99 ms per frame, measured).  A host with streams of its own should raise
 * GPU_MAX_HW_QUEUES (environment, before the HIP runtime starts; bench.py sets 8). */
int vf_ctx_stream(const vf_ctx *ctx, void **stream);

/* ---- terrain object ---------------------------------------------------------------------- */
/*
 * Replaces TerrainSpike::new / Scene::new minus the Python-side validation
 * (src/terrain/mod.rs:259-407, src/scene/mod.rs:60-206): colour target W x H (Rgba8UnormSrgb),
 * fixed pipeline state (src/terrain/pipeline.rs:97-139), the procedural n x n grid of
 * build_grid_xyuv (src/terrain/mod.rs:553-598; never materialised), the 256x1 LUT
 * (ColormapLUT::new, src/terrain/mod.rs:31-110).  lut_is_srgb = 1: bytes are sRGB-encoded and
 * decoded per texel before filtering (Rgba8UnormSrgb); 0: bytes are used as UNORM (the
 * VF_FORCE_LUT_UNORM fallback).  The height texture starts as a 1x1 zero texel
 * (src/terrain/mod.rs:342-378); uniforms start zeroed -- call vf_terrain_set_uniforms.
 * grid < 2 is raised to 2 like the reference (`.max(2)`).
 */
int vf_terrain_create(vf_ctx *ctx, uint32_t width, uint32_t height, uint32_t grid,
                      const uint8_t lut_rgba8[1024], int lut_is_srgb, vf_terrain **out);
void vf_terrain_destroy(vf_terrain *t);

/* queue.write_buffer(ubo, TerrainUniforms) -- 44 floats, layout of src/terrain/mod.rs:114-123 */
int vf_terrain_set_uniforms(vf_terrain *t, const float uniforms[44]);

/* Scene::set_height_from_r32f (src/scene/mod.rs:226-276): R32F texture (th rows x tw cols, tightly
 * packed float32, no 256-byte row padding needed), nearest, clamp-to-edge.  Copies host -> HBM. */
int vf_terrain_set_height(vf_terrain *t, const float *host_height, uint32_t tw, uint32_t th);
/* same, borrowing a texture already resident in HBM (e.g. a torch tensor's data_ptr) */
int vf_terrain_set_height_device(vf_terrain *t, const float *dev_height, uint32_t tw, uint32_t th);

/* Fragment-stage variant.  VF_SHADE_REFERENCE (default) is fs_main as coded (src/shaders/terrain.wgsl:69-91): analytic
 * normals, no tonemap -- the only mode for which parity with the reference is claimed.  VF_SHADE_SPEC_T32 is the stage the
 * reference documents but never implemented (ROADMAP.md:421-436 forward-difference normals from the height texture;
 * README.md:128,174-175 Reinhard in linear before the sRGB store); it is validated against this build's oracle only. */
#define VF_SHADE_REFERENCE 0
#define VF_SHADE_SPEC_T32 1
int vf_terrain_set_shade_mode(vf_terrain *t, int mode);
/* Fragment-stage arithmetic (new; the reference leaves it to the driver's shader compiler, src/shaders/terrain.wgsl:69-91).
 * VF_PRECISION_FAST (default): hardware reciprocal / rsq / sin / cos / log / exp and fused multiply-adds -- visibility is
 * unaffected, RGBA stays within 1 LSB per channel of VF_PRECISION_EXACT (BASELINE.json: "RGBA within +-1 LSB of reference"),
 * which evaluates every operation as a correctly rounded IEEE binary32 one in a fixed order and reproduces the CPU oracle bit
 * for bit.  VF_SHADE_SPEC_T32 frames are always drawn with the exact arithmetic. */
#define VF_PRECISION_EXACT 0
#define VF_PRECISION_FAST 1
int vf_terrain_set_shade_precision(vf_terrain *t, int precision);
/* The raster stage's line loop exists twice (round 4): with and without a first pass that tests a triangle's lines in groups of four
 * against the final-pixel masks.  Which one is faster depends on the view and on how the frame is cut (wide items with many-line
 * triangles gain, a multi-GPU rank's narrow strips lose); the picture never differs.  mode -1 (default): the handle times both on
 * its own frames (one HIP event at the end of a frame's work on the draw stream; the time between two consecutive frames of one
 * variant -- the frame period -- read back frames later, never a wait) and keeps the faster one per view; re-measured when the shard
 * layout, the heights or (at the start of a motion) the camera change;
 * 0 / 1: fixed.  No reference counterpart: the fixed-function raster behind draw_indexed, src/terrain/mod.rs:435. */
int vf_terrain_set_raster_groups(vf_terrain *t, int mode);
/* which variant drew the last frame (0 / 1) and, when measured, the frame period with each in this view (ms; 0 = not measured) */
int vf_terrain_raster_groups(const vf_terrain *t, int *in_use, float ms[2]);

/* Multi-GPU screen split (new; the reference is single-device).  Pixel row y belongs to this
 * object iff ((y / band_h) % nranks) == rank; owned rows are stored densely ("local rows") in
 * band order.  band_h must be a power of two.  Default: rank 0 of 1 (all rows). */
int vf_terrain_set_shard(vf_terrain *t, uint32_t rank, uint32_t nranks, uint32_t band_h);
int vf_terrain_local_rows(const vf_terrain *t, uint32_t *rows);

/* Multi-GPU screen split by interleaved 64 x 64 tiles ("screen-tile split", BASELINE.json configs[3]; new, the reference
 * is single-device).  The `layout` argument of vf_terrain_set_tile_shard, vf_tile_layout and vf_stitch_tiles_device is ONE WORD,
 * VF_TILE_LAYOUT(skew, stripe_log2) = skew | stripe_log2 << 16:
 *     tile (tx, ty) belongs to rank ((tx >> stripe_log2) + skew * ty) % nranks
 * -- column stripes 2^stripe_log2 tiles wide dealt round-robin to the ranks, each tile row shifted by `skew` stripes.  A plain
 * number < 65536 is therefore a skew with single-tile stripes (the meaning the argument had before round 4).  skew 0 = column
 * stripes (what vf_dist_exchange_bands needs, and bench.py's default with a period of eight tile columns: stripe_log2 2 / 1 / 0
 * for 2 / 4 / 8 ranks).  skew < 65536 and stripe_log2 <= 15; a word with any higher bit set is refused (VF_ERR_INVALID).
 * A rank stores its tiles densely, row-major by (ty, tx), each as 64 x 64 RGBA8 words (edge tiles keep the full slot): local
 * tile k starts at byte k * 16384.  vf_tile_layout lists a rank's tiles (tx | ty << 16; pure host arithmetic, no device needed;
 * tiles may be NULL to count).  A tile-sharded handle is read with vf_terrain_read_tiles; rows come back after
 * vf_stitch_tiles_device. */
#define VF_TILE_LAYOUT(skew, stripe_log2) ((uint32_t)(skew) | ((uint32_t)(stripe_log2) << 16))
int vf_terrain_set_tile_shard(vf_terrain *t, uint32_t rank, uint32_t nranks, uint32_t layout);
/* Load-balanced stripes (round 5; SURVEY.md 8(e) "a load-balanced map").  The round-robin deal gives every rank the same NUMBER of
 * stripes, not the same work: at C4's top-down camera the slowest of 4 ranks carries 15 % more than the fastest.  Three pieces:
 *   vf_terrain_tile_times      the time (ms) the handle's last frame spent on each of its local tiles (what its own frame plan
 *                              feeds on); summed per stripe and added up over the ranks by the host (an all-reduce of <= 256 floats)
 *                              they are the per-stripe cost every rank agrees on.  *count = local tiles; ms may be NULL to count.
 *   vf_balance_stripes         the deterministic rule: heaviest stripe first, each to the least loaded rank that still has room --
 *                              every rank keeps nstripes / nranks stripes, so slabs and exchanged chunks keep their sizes; the same
 *                              times give the same table on every rank.
 *   vf_tile_layout_register_map  an owner table (owner[sc] for the stripe sc = tx >> stripe_log2) -> a layout WORD (bit 20 set) that
 *                              every entry point taking a layout accepts: vf_terrain_set_tile_shard, vf_tile_layout,
 *                              vf_stitch_tiles_device, and through the handle vf_dist_exchange_bands / vf_dist_gather_tiles.  Tables
 *                              are immutable and process-wide (64 at most); registering the same table again returns the same word.
 * No reference counterpart (single device: src/terrain/mod.rs:277-294). */
int vf_terrain_tile_times(vf_terrain *t, float *ms, uint32_t capacity, uint32_t *count);
int vf_balance_stripes(const float *stripe_ms, uint32_t nstripes, uint32_t nranks, uint8_t *stripe_owner);
int vf_tile_layout_register_map(const uint8_t *stripe_owner, uint32_t nstripes, uint32_t stripe_log2, uint32_t nranks, uint32_t *layout);
int vf_terrain_local_tiles(const vf_terrain *t, uint32_t *tiles);
int vf_terrain_read_tiles(vf_terrain *t, uint8_t *dst, uint32_t first, uint32_t count);
int vf_tile_layout(uint32_t width, uint32_t height, uint32_t rank, uint32_t nranks, uint32_t layout, uint32_t *tiles,
                   uint32_t capacity, uint32_t *count);

/* Render into a caller-provided device buffer of local_rows*W*4 bytes (tile shards: local_tiles*16384 bytes);
 * NULL = internal buffer. */
int vf_terrain_set_output_device(vf_terrain *t, void *dev_rgba);
int vf_terrain_rgba_device(const vf_terrain *t, void **dev_rgba);

/*
 * The render pass of render_png (src/terrain/mod.rs:412-437, src/scene/mod.rs:280-298): clear to
 * linear (0.02,0.02,0.03,1), one indexed draw of 6(n-1)^2 indices, vs_main / raster / fs_main
 * (src/shaders/terrain.wgsl:44-91), sRGB store.  Leaves tightly packed RGBA8 (local rows) in HBM.
 * Asynchronous on `stream` (NULL = the context's stream): the output is complete when work queued on `stream` after this
 * call runs.  How the frame's work is ordered and split follows the times measured on this handle's earlier frames -- that
 * steers speed only, never a pixel.  Where the planning kernels run (round 6): for a caller that WAITS for every frame, on
 * `stream` itself -- and the plan of its next frame, when the inputs have not changed, behind the copy of its next read-back
 * (vf_terrain_read_rgba / _read_png_scanlines return when the copy is done, not when that plan is); for a caller that submits
 * a frame while the previous one is in flight, on two streams of the context (made once per process, 17-20 ms), under the
 * previous frame's tile kernel.
 */
int vf_terrain_render(vf_terrain *t, void *stream);
/* BASELINE.json configs[4] ("batch of 64 camera look-ats over one terrain"): n render passes with n uniform blocks over the handle's
 * terrain, queued back to back on `stream` -- the loop Scene.set_camera_look_at + render_png runs per pose (src/scene/mod.rs:208-224,
 * :278-335) without the per-pose FFI round trips and read-backs.  uniforms: n x 44 floats (vf_terrain_set_uniforms layout);
 * dev_rgba: n device buffers, frame k goes to dev_rgba[k] (NULL: every frame into the current output buffer, the last one stays).
 * Every pose is planned from the tile times of the pose before last, looked up through the camera motion between the two (the
 * homography of the ground plane): no pose waits for its predecessor's times, the plan and the set-up pass of pose k + 1 run under
 * pose k's tile kernel.  Afterwards the handle's uniforms are the last pose's and its output buffer is dev_rgba[n - 1].
 * Multi-GPU (pose-parallel replicas, no collective): rank r passes the poses k = r mod N. */
int vf_terrain_render_batch(vf_terrain *t, const float *uniforms, uint32_t n, void *const *dev_rgba, void *stream);
/* The same batch with every frame read back (the per-pose copy_texture_to_buffer + map of src/terrain/mod.rs:439-485): pose k is drawn
 * into one of three device frames owned by the handle and copied to host_rgba[k] (H*W*4 bytes each; page-locked destinations --
 * vf_host_alloc -- travel by DMA while the next poses are drawn).  Returns when every frame has arrived.  Whole-frame handles only.
 * The handle's own output buffer is left untouched (and "nothing rendered yet" holds for it afterwards). */
int vf_terrain_render_batch_host(vf_terrain *t, const float *uniforms, uint32_t n, uint8_t *const *host_rgba);
int vf_terrain_sync(vf_terrain *t);

/* Overlays (new; the reference plans them, ROADMAP.md Milestone B2, and never implemented them): points and polylines in the
 * terrain's world frame, drawn over every frame the handle renders -- vf_terrain_render, _render_batch, _render_batch_host, and so
 * every read-back -- as pixel-sized screen-space primitives with analytic anti-aliasing, blended in linear light in layer order
 * (layers in the order they were added, features in input order), straight alpha; the terrain does not occlude them.  The
 * conventions, bit for bit, are DESIGN.md "Overlays"; visibility read-backs and the fragment-stage diagnostics never show them.
 * Data is copied to HBM by the call.  A handle has at most 2^24 primitives (a point is one; a path of m vertices at most 2m - 1).
 * Overlays need a whole-frame handle: on a band- or tile-sharded handle these calls, and vf_terrain_set_shard /
 * vf_terrain_set_tile_shard on a handle with overlays, fail with VF_ERR_INVALID.  A handle with overlays waits once per frame, between
 * binning passes, for the number of (primitive, bin) pairs; a handle without overlays launches and allocates nothing for them.
 *   vf_terrain_add_points: n points xyz[3n]; size_px[n] (diameter / side in pixels, clamped to [1, 64]) or NULL for default_size;
 *     rgba[4n] sRGB8 bytes with alpha or NULL for default_rgba; shape VF_SHAPE_*; drape != 0: y is an offset above the rendered
 *     surface.  Points with a non-finite coordinate are dropped.
 *   vf_terrain_add_lines: npaths paths, path p = vertices path_offsets[p] .. path_offsets[p + 1] - 1 of xyz (>= 2 each, all finite);
 *     width_px clamped to [1, 64]; one colour; cap VF_CAP_*; round joins.
 *   *layer_id (may be NULL): the layer's number, counting from 0 since the handle's last vf_terrain_clear_overlays.
 *   vf_terrain_clear_overlays: removes every layer and frees their memory (frames are then byte-identical to a handle that never had any). */
#define VF_SHAPE_CIRCLE 0
#define VF_SHAPE_SQUARE 1
#define VF_CAP_BUTT 0
#define VF_CAP_SQUARE 1
#define VF_CAP_ROUND 2
int vf_terrain_add_points(vf_terrain *t, const float *xyz, uint32_t n, const float *size_px, const uint8_t *rgba, float default_size,
                          const uint8_t default_rgba[4], int shape, int drape, uint32_t *layer_id);
int vf_terrain_add_lines(vf_terrain *t, const float *xyz, const uint32_t *path_offsets, uint32_t npaths, float width_px,
                         const uint8_t rgba[4], int cap, int drape, uint32_t *layer_id);
int vf_terrain_clear_overlays(vf_terrain *t);
/* Polygon overlays (new; the reference plans add_polygons in ROADMAP.md Milestone B2 and never implemented it): filled polygons with
 * optional outlines, in the same layer order as points and lines.  The conventions, bit for bit, are DESIGN.md 4c.
 *   vf_terrain_add_polygons: nfeatures polygons; polygon f is rings feature_offsets[f] .. feature_offsets[f + 1] - 1 (>= 1 each,
 *     feature_offsets ascending, <= nrings), ring r is vertices ring_offsets[r] .. ring_offsets[r + 1] - 1 of xyz (>= 3 each, all
 *     finite; the ring closes back to its first vertex by itself).  Any number of exteriors and holes: the fill rule is even-odd over
 *     all of a polygon's rings, so orientation does not matter and a MultiPolygon is one polygon.  Fill colour: fill_rgba[4 nfeatures]
 *     (one per polygon) or, if NULL, default_fill; both NULL: no fill.  line_rgba: the outline colour (NULL: no outline), drawn as
 *     vf_terrain_add_lines of each closed ring with width line_width_px (clamped to [1, 64]), round caps and joins.  At least one of
 *     fill and outline is required.  drape != 0: y is an offset above the rendered surface at each vertex (edges stay straight on
 *     screen).  The layer holds every fill, in polygon order, then every outline.  Fills are clipped at the near plane only.  A fill
 *     takes 1 + 2 primitives per ring edge of the 2^24 budget, an outline 2 per ring vertex + 1.  A handle with polygon fills reads
 *     back, with the pair count, the number of (polygon, screen bin) backdrop masks of the frame (the same single wait per frame). */
int vf_terrain_add_polygons(vf_terrain *t, const float *xyz, const uint32_t *ring_offsets, uint32_t nrings, const uint32_t *feature_offsets,
                            uint32_t nfeatures, const uint8_t *fill_rgba, const uint8_t default_fill[4], const uint8_t line_rgba[4],
                            float line_width_px, int drape, uint32_t *layer_id);
/* Occlusion of a point or line layer by the terrain (new; opt-in, per layer; DESIGN.md 4d has the conventions bit for bit).  With
 * occlude != 0 the layer's points and segments are not drawn at pixels where the rendered terrain is in front of them: hidden where
 * the terrain's interpolated 1/w exceeds the primitive's 1/w times kb = 1 + depth_bias (depth_bias >= 0, finite; the library's
 * default is VF_OCCLUSION_DEPTH_BIAS).  occlude == 0 restores the layer's plain compositing.  Updates the layer's records in place
 * (no upload).  A handle with an occluding layer draws its frames with the visibility store on and holds one W x H id buffer.
 * VF_ERR_INVALID for an unknown layer, a polygon layer (polygon fills have no depth), a negative or non-finite depth_bias, and a
 * sharded handle. */
#define VF_OCCLUSION_DEPTH_BIAS 1e-2f
int vf_terrain_set_layer_occlusion(vf_terrain *t, uint32_t layer_id, int occlude, float depth_bias);
/* Hazed overlay layers (new; opt-in, per layer; DESIGN.md 4r has the conventions bit for bit).  Overlays are not hazed unless their
 * layer asks: with on != 0 a point, line or contour layer takes the handle's atmospheric haze (vf_terrain_set_haze, below).  At every
 * pixel a feature of the layer covers, its colour is first blended towards the haze colour by the haze opacity of the feature's own
 * depth and world height there -- the 1/w and y/w of a point's centre, or of a segment's clipped ends interpolated along it, through
 * the same opacity function as the terrain's pass (density, start, falloff, base, max_opacity, the colour's alpha; `background` plays
 * no part) -- and then goes over the pixel with the feature's own alpha, which is not changed.
 * vf_terrain_set_layer_haze: sets (on != 0) or clears the layer's flag; updates the layer's records in place (no upload).  The flag
 *   rests with the layer until vf_terrain_clear_overlays.  It does nothing while the handle's haze is disabled, cleared, never set or
 *   has density 0: such frames are the unhazed ones byte for byte and launch what they launched before.  While haze is enabled every
 *   frame uses the handle's current haze parameters: no layer is added again after vf_terrain_set_haze.  A layer may both occlude and
 *   take the haze, and supersampled handles take hazed layers (the overlay pass runs at the output size).  The first hazed layer of a
 *   handle allocates one 16-byte side record per primitive, filled on the frames that haze overlays.  Always the exact arithmetic:
 *   it does not follow vf_terrain_set_shade_precision.  VF_ERR_INVALID, nothing changed: an unknown layer, a polygon layer (a polygon
 *   layer cannot take the haze: polygon fills have no depth), a sharded handle.
 * vf_terrain_layer_haze: *on = 1 if the layer's flag is set, else 0.  VF_ERR_INVALID for an unknown layer. */
int vf_terrain_set_layer_haze(vf_terrain *t, uint32_t layer_id, int on);
int vf_terrain_layer_haze(vf_terrain *t, uint32_t layer_id, int *on);
/* Contour lines (new; isolines of the rendered surface, DESIGN.md 4e has the contract bit for bit).  The lines are extracted on the
 * device from the surface the handle draws -- the displaced height h of every grid vertex on the renderer's own triangulation, not the
 * uploaded texture -- and appended as one layer of draped line records, which every later frame draws like a line layer's.
 *   levels[nlevels]: finite, strictly ascending, 1 <= nlevels <= 65536, in units of h before exaggeration (what the colormap sees; world
 *     y = h * exaggeration).  width_px clamped to [1, 64]; one colour; lift: world-space offset above the surface (finite).
 *   join VF_JOIN_ROUND: a disc at the start of every segment (2 primitives per segment; every joint of a chain is closed);
 *     VF_JOIN_NONE: segments only (1 primitive per segment; for dense layers).
 *   occlude / depth_bias: as vf_terrain_add_lines followed by vf_terrain_set_layer_occlusion, which also works on the layer afterwards.
 *   The layer is one feature: its coverage is folded with max over the whole layer, so a translucent contour does not darken at
 *     joints or where two contours touch.
 *   Snapshot: the layer is made from the heights and the grid spacing the handle holds when the call is made (a height texture handed
 *     over in device memory must be complete by then).  It follows a later change of exaggeration (draped records); it does not follow
 *     a later height upload: vf_terrain_clear_overlays and add again.
 *   *nsegments (may be NULL): the number of segments found.  Zero segments is not an error: an empty layer with its id.
 *   VF_ERR_INVALID, nothing added: bad levels / width / lift / join / depth_bias, a sharded handle, and a layer that would exceed the
 *     handle's 2^24 primitives (the message names the number of segments found).
 * vf_terrain_height_bounds: min / max of h over the grid's vertices, non-finite heights left out (lo = inf, hi = -inf when there is
 *   none).  vf_terrain_layer_primitive_count: the primitive records of a layer (any kind).  Both wait for the frame in flight. */
#define VF_JOIN_ROUND 0
#define VF_JOIN_NONE 1
int vf_terrain_add_contours(vf_terrain *t, const float *levels, uint32_t nlevels, float width_px, const uint8_t rgba[4], float lift, int join,
                            int occlude, float depth_bias, uint32_t *layer_id, uint32_t *nsegments);
int vf_terrain_height_bounds(vf_terrain *t, float *lo, float *hi);
int vf_terrain_layer_primitive_count(vf_terrain *t, uint32_t layer_id, uint32_t *count);

/* copy_texture_to_buffer + map + un-pad (src/terrain/mod.rs:439-485): local rows [y0, y0+rows)
 * into dst (rows*W*4 bytes).  Waits for the last render and for the copy (work the library queues behind the copy for the
 * caller's NEXT frame may still be running when this returns: later calls on the handle are ordered after it). */
int vf_terrain_read_rgba(vf_terrain *t, uint8_t *dst, uint32_t y0, uint32_t rows);
/* Page-locked host memory for read-back destinations (new; the reference maps a fresh staging buffer per call,
 * src/terrain/mod.rs:446-451).  vf_terrain_read_rgba into such a buffer is ONE DMA transfer (C4: 64 MiB in 1.2 ms); into ordinary
 * pageable memory it goes through the handle's ring of pinned chunks and a copy by host threads, and a frame-sized fresh
 * destination is page-fault bound (2-5 ms).  Any hipHostMalloc / hipHostRegister memory of the caller's is recognised as well.
 * Buffers of 4 MiB and more are 2 MiB-aligned MADV_HUGEPAGE memory registered with the runtime (2.6 ms to make for 64 MiB, where
 * hipHostMalloc takes 9 and its first copy another 11-16); free them with vf_host_free only. */
int vf_host_alloc(size_t bytes, void **host);
void vf_host_free(void *host);
/* Read-back for render_png (src/terrain/mod.rs:439-490): the last frame as PNG scanlines -- per row one filter-type byte
 * (row-adaptive: the filter with the smallest sum of absolute residuals, chosen on the GPU) followed by W*4 filtered
 * bytes -- in pinned host memory owned by the handle (allocated once, not per call as the reference's read-back buffer
 * :446-451), valid until the next call on the handle.  The host only deflates.  Whole-frame handles only. */
int vf_terrain_read_png_scanlines(vf_terrain *t, const uint8_t **host_scanlines, size_t *nbytes);
/* debug/parity: per-pixel visible primitive id + 1 (0 = background), local rows.  The visibility tile never leaves LDS in a
 * normal frame, so this draws a frame again into scratch buffers: the frame vf_terrain_render drew last (its uniforms and
 * shade mode, whatever was set since), or -- before the first vf_terrain_render on this shard layout -- the current uniforms.
 * The caller's output buffer and the `rendered` state are left as they were. */
int vf_terrain_read_visibility(vf_terrain *t, uint32_t *dst);

/* enable: 0 off; 1 device times (HIP events around the frame's kernels) and the per-item statistics behind
 * vf_terrain_debug_item_stats / vf_timings.blocks_* (the tile kernel then writes them: a few atomics per drawn block);
 * 2 device times only -- the kernels run exactly as they do untimed (blocks_* read 0);
 * 3 as 2, for every FOURTH frame only (what bench.py times: the two event records a timed frame puts on the draw stream keep
 *   the next kernel from being launched under the previous one and cost a C4 frame 2 %, tools/exp_timing_cost.py); the frame
 *   periods vf_timings.total_ms / vf_terrain_frame_times report are then per frame, from events four frames apart; the plan chain
 *   carries no events at this level (ranges_ms / plan_ms read 0: measure them at level 2). */
int vf_terrain_enable_timing(vf_terrain *t, int enable);
int vf_terrain_timings(vf_terrain *t, vf_timings *out);
/* The same HIP events frame by frame (timing enabled; the frames since vf_terrain_enable_timing, at most the last 64, oldest
 * first): tile_ms[f] = k_clear + k_tile of frame f on the caller's stream, period_ms[f] = end of frame f - 1 -> end of frame f
 * (frames rendered back to back overlap: the period is what a frame costs; period_ms[0] = 0).  Either array may be NULL.
 * For the median / p95 report of python/tools/perf_sanity.py:45-69. */
int vf_terrain_frame_times(vf_terrain *t, float *tile_ms, float *period_ms, uint32_t max_frames, uint32_t *count);
/* diagnostics (timing enabled): per work item of the last frame (a busy tile, or one column strip of a heavy tile), in
 * launch order, 4 words: item code (local tile | strip << 20 | log2(strips) << 24 | depth slice << 27 | log2(slices) << 29), candidate blocks processed,
 * raster-phase time, raster+fragment time (10 ns ticks of the constant 100 MHz clock).  *count = items written. */
int vf_terrain_debug_item_stats(vf_terrain *t, uint32_t *dst, uint32_t max_items, uint32_t *count);
/* debug/tests (band masks): what the set-up pass left in the plan state the frame rendered last was drawn from, copied
 * after a full wait.  Per block of the grid, row-major (by * blocks_per_side + bx): recs 8 words -- the pixel box as four int16
 * {x0, y0, x1, y1} (x0 > x1: nothing to draw), flags, count, alive_even and alive_odd (64 bits each, low word first); masks
 * VF_BAND_SLOTS x {even, odd} 64-bit words -- slot s: the alive primitives that reach a row of tiles r with r % VF_BAND_SLOTS == s;
 * xy 81 x {X, Y} int32, the block's 9 x 9 snapped vertices (24.8 fixed point).  Any of the three may be NULL.  Blocks the frame's
 * set-up pass did not visit (nothing of them can reach this shard's pixels: count 0, an empty box) keep whatever an earlier frame left.
 * *count = blocks of the grid; VF_ERR_INVALID when max_blocks is smaller or nothing was rendered.  Host copies only. */
#define VF_BAND_SLOTS 8u
int vf_terrain_debug_band_masks(vf_terrain *t, uint32_t *recs, uint64_t *masks, int32_t *xy, uint32_t max_blocks, uint32_t *count);
/* debug/tests: set the scheduling feedback the NEXT frame's plan reads, instead of whatever the machine measured.
 * Per local tile (storage order, ntiles = vf_terrain_local_tiles): tile_ticks[k] the tile's time in 10 ns ticks, strips_log2[k] the
 * log2 (0 .. 4) of the strips that time was "recorded" with, piece_ticks[64 k + p] the time of its piece p (NULL: all zero).
 * The call waits for the handle's queued work, throws away a plan queued ahead of its frame (the next plan then takes the previous
 * frame's times, as after any such drop) and writes the words into BOTH plan states -- tile words, piece words, bits 8.. of the
 * per-tile flag words (bit 0, background, stays) -- so that the next plan reads them whichever state it takes them from.  The split
 * quantum is not set: the next plan derives it from the tile words as always.  Nothing else moves: which mode the next frame is
 * planned in follows from the calls made, as without this one.  vf_terrain_tile_times reports the injected words until the next frame.
 * VF_ERR_INVALID, and nothing is changed: a NULL pointer, ntiles != local tiles, strips_log2 > 4, or a handle on its first two frames
 * since create / set_shard / set_tile_shard (those are planned from a static estimate that overwrites the words).
 * Scheduling only: no frame may differ by a pixel for anything passed here. */
int vf_terrain_debug_set_plan_feedback(vf_terrain *t, const uint32_t *tile_ticks, const uint8_t *strips_log2, const uint32_t *piece_ticks,
                                       uint32_t ntiles);
/* debug/tests: how the frame vf_terrain_render drew last was planned, VF_PLAN_* bits.  VF_ERR_INVALID before the first frame. */
#define VF_PLAN_FIRST        1u   /* no tile times yet: the static estimate */
#define VF_PLAN_FRESH        2u   /* tile times of the frame before it (the plan waited for that frame) */
#define VF_PLAN_MOTION_MAP   4u   /* tile times looked up through the camera motion */
#define VF_PLAN_DILATE       8u   /* every tile takes the heaviest time of its neighbourhood */
#define VF_PLAN_QUEUED_AHEAD 16u  /* the plan was queued ahead of the call, behind the frame before it */
#define VF_PLAN_GEOMETRY_REUSED 32u /* block boxes and set-up records of this plan state were built from the same geometry inputs: not rebuilt */
#define VF_PLAN_TILE_LISTS   64u  /* the tile kernel read this plan state's per-tile candidate lists */
int vf_terrain_debug_plan_mode(const vf_terrain *t, uint32_t *mode);
/* debug/tests (candidate lists): while a plan state's set-up records stand, the blocks that can reach each local tile are
 * listed once, off the frames' chain, and later frames drawn from that state read the lists instead of testing the block ranges.
 * For the plan state the last frame was drawn from -- built: its lists exist (or are queued) for the live geometry; used: the last
 * frame read them; tiles_listed / tiles_fallback: local tiles with a list (an empty one counts) / without, because the shared buffer
 * was full; entries: listed (tile, block) pairs; capacity: the buffer's 16-byte units handed to the builder; units_asked: what all
 * tiles together asked for (entries + offset words; saturates).  The counts are zero when neither built nor used.  The call waits for
 * the builder.  VF_NO_TILE_LISTS=1 in the environment when a handle is created: that handle never builds a list.
 * VF_ERR_INVALID before the first frame. */
typedef struct vf_tile_list_info { uint32_t built, used, tiles_listed, tiles_fallback, entries, capacity, units_asked, reserved; } vf_tile_list_info;
int vf_terrain_debug_tile_lists(vf_terrain *t, vf_tile_list_info *out);
/* debug/tests: the capacity (16-byte units) the NEXT builders get, at most the buffer's own size; UINT32_MAX: the default.  Waits for
 * the handle's queued work, throws away a plan queued ahead and marks both plan states' lists as not built: each is built again
 * behind the next frame drawn from it.  0: every tile that a block reaches falls back.  No frame may differ by a pixel. */
int vf_terrain_debug_set_tile_list_capacity(vf_terrain *t, uint32_t units);
/* diagnostics, only in libraries built with -DVF_PHASE_PROF (VF_ERR_INVALID otherwise): shader-clock cycles summed over
 * all waves of the last frame's tile kernel, per phase (set-up, pull/cull, vertex stage, classification, span raster,
 * completion/rescan, end-of-chunk wait, fragment stage), then 8 event counts, then up to 8 parts of the set-up phase; n <= 32 */
int vf_terrain_debug_phase_cycles(vf_terrain *t, uint64_t *dst, uint32_t n);

/* ---- grid_generate ----------------------------------------------------------------------- */
/* make_grid (src/terrain/mesh.rs:35-90) computed on the GPU; outputs as the PyO3 wrapper returns
 * them (:149-203): xy (nx*nz,2) f32, uv (nx*nz,2) f32, idx 6(nx-1)(nz-1) u32.  Argument validation
 * (ValueError strings) is done by the host layer.  Host-pointer form copies back; device form
 * leaves results in HBM. */
int vf_grid_generate(vf_ctx *ctx, uint32_t nx, uint32_t nz, float dx, float dy,
                     float *xy, float *uv, uint32_t *idx);
int vf_grid_generate_device(vf_ctx *ctx, uint32_t nx, uint32_t nz, float dx, float dy,
                            float *dev_xy, float *dev_uv, uint32_t *dev_idx, void *stream);

/* ---- triangle smoke path ------------------------------------------------------------------ */
/* Renderer::render_triangle_rgba (src/lib.rs:286-309, :685-721; src/shaders/triangle.wgsl):
 * white clear, one colour-varying triangle, tightly packed (H,W,4) u8 into host memory. */
int vf_triangle_render(vf_ctx *ctx, uint32_t width, uint32_t height, uint8_t *rgba_host);

/* ---- Renderer DEM path ------------------------------------------------- */
/* HBM-resident heightmap of Renderer::add_terrain and its statistics / normalisation / R32F texture
 * round trip (src/lib.rs:336-682, 905-951; src/renderer.rs; src/terrain_stats.rs).  Not connected to any draw in
 * the reference either. */
typedef struct vf_dem vf_dem;
int vf_dem_create(vf_ctx *ctx, vf_dem **out);
void vf_dem_destroy(vf_dem *d);
/* add_terrain ingest (src/lib.rs:351-388): heights = (f32)src * exaggeration, row-major h rows x w cols */
int vf_dem_set_heights_f32(vf_dem *d, const float *host, uint32_t w, uint32_t h, float exaggeration);
int vf_dem_set_heights_f64(vf_dem *d, const double *host, uint32_t w, uint32_t h, float exaggeration);
/* terrain_stats -> dem_stats_from_slice (src/lib.rs:905-932): out = {min, max, mean, std}.
 * min / max: the reference starts both at heights[0] and replaces them by `<` / `>`, so a NaN FIRST sample gives min = max = NaN
 * (and minmax-normalising that map gives all NaN); a NaN anywhere else is passed over.  The same here.  One difference remains:
 * among zeros of both signs the reference keeps the first zero it meets, the reduction here orders floats as integers and
 * reports -0 as min and +0 as max -- equal as numbers (==), not as bits.
 * mean = (f32)(sum in f64 / n); std = sqrt((f32)(sum in f64 of (f32)((h - mean) * (h - mean)) / n)), h - mean and the square in f32
 * with the f32 mean, as the reference forms them; the reference adds both sums in f32 in index order. */
int vf_dem_stats(vf_dem *d, float out[4]);
/* terrain_stats::min_max(data, clamp=true) (src/terrain_stats.rs:11-35): 1st / 99th percentile, stride-sampled above 65536:
 * step = n / 65536 (1 up to 65536 samples), the samples h[0], h[step], ... sorted, elements (size_t)((f32)m * 0.01f) and
 * (size_t)((f32)m * 0.99f) of the m of them.  With a NaN among the samples the result is unspecified, as the reference's own
 * sort (partial_cmp with Equal for the unordered) is. */
int vf_dem_percentile_range(vf_dem *d, float *p1, float *p99);
/* normalize_terrain -> normalize_in_place (src/lib.rs:934-951): mode 0 = minmax to [lo, hi], 1 = zscore */
int vf_dem_normalize(vf_dem *d, int mode, float lo, float hi, float eps);
/* upload_height_r32f (src/lib.rs:496-571): heights -> R32F texture (device copy, no row padding) */
int vf_dem_upload_height(vf_dem *d);
int vf_dem_texture_size(const vf_dem *d, uint32_t *w, uint32_t *h);   /* 0 x 0 before the first upload */
/* debug_read_height_patch (src/lib.rs:574-666): texture sub-rectangle -> dst (h rows x w cols) */
int vf_dem_read_patch(vf_dem *d, uint32_t x, uint32_t y, uint32_t w, uint32_t h, float *dst);

/* ---- multi-GPU helper --------------------------------------------------------------------- */
/* De-interleave a rank-major gather buffer [nranks][local_rows][W][4] into the final (H,W,4)
 * image on the device (used after an RCCL all-gather/gather when receiving in place is not
 * possible).  All pointers are device pointers. */
int vf_stitch_bands_device(vf_ctx *ctx, const void *dev_gathered, void *dev_image, uint32_t width,
                           uint32_t height, uint32_t nranks, uint32_t band_h, void *stream);
/* Same for tile shards: gather buffer [nranks][stride_tiles][64][64][4] (stride_tiles >= the largest shard) -> (H,W,4);
 * `layout` = the VF_TILE_LAYOUT word the shards were made with. */
int vf_stitch_tiles_device(vf_ctx *ctx, const void *dev_gathered, void *dev_image, uint32_t width, uint32_t height,
                           uint32_t nranks, uint32_t layout, uint32_t stride_tiles, void *stream);

/* ---- multi-GPU exchange over RCCL (new: the reference creates one device per object,
 * src/terrain/mod.rs:277-294, and has no exchange) -------------------------------------------------------------
 * One process per GPU.  The library resolves RCCL at run time (librccl.so.1: the copy already loaded in the process,
 * e.g. PyTorch's, else the ROCm one); nothing here needs torch.  A communicator is an `ncclComm_t` passed as void*:
 * either one the host already owns (torch.distributed's, a Rust host's own binding) or one made by vf_dist_comm_init.
 *
 *   rank 0:  vf_dist_unique_id(id)            -> hand the 128 bytes to every rank (any host channel)
 *   all:     vf_dist_comm_init(ctx, id, rank, nranks, &comm)
 *   frame:   vf_terrain_set_tile_shard(t, rank, nranks, layout); vf_terrain_set_output_device(t, slab); vf_terrain_render(t, s);
 *            vf_dist_gather_tiles(t, comm, 0, gathered, stride_tiles, s);      (all ranks; `gathered` used on the root)
 *            root: vf_stitch_tiles_device(ctx, gathered, image, W, H, nranks, layout, stride_tiles, s);
 *   or, with column stripes (skew 0) and a tile grid that divides by nranks -- the default of bench.py:
 *            vf_dist_exchange_bands(t, comm, 0, image, s);                     (all ranks; `image` used on the root; no root stitch)
 */
#define VF_DIST_UNIQUE_ID_BYTES 128
int vf_dist_available(void);                                   /* 1 when RCCL could be resolved in this process */
int vf_dist_version(int *version);                             /* ncclGetVersion of the RCCL this process resolved (e.g. 22703) */
int vf_dist_unique_id(uint8_t id[VF_DIST_UNIQUE_ID_BYTES]);    /* ncclGetUniqueId */
int vf_dist_comm_init(vf_ctx *ctx, const uint8_t id[VF_DIST_UNIQUE_ID_BYTES], int rank, int nranks, void **comm);   /* ncclCommInitRank on ctx's device */
void vf_dist_comm_destroy(void *comm);                         /* ncclCommDestroy on the communicator's own device */
/* Every rank of the communicator calls the gather with the SAME root, stride_tiles and shard layout.  What a rank can check
 * locally (handle sharded and rendered, communicator rank/size == the handle's shard, root in range, stride_tiles >= the
 * largest shard of the layout) is checked on every rank before anything is posted, so all ranks fail together.  The root's
 * buffer pointer can only be checked on the root: a root that passes NULL returns VF_ERR_INVALID while the other ranks have
 * queued their sends and wait -- pass a valid buffer.
 * Tile shards -> rank `root`, point to point (every sender on its own xGMI link to the root, no ring): one
 * ncclGroupStart / ncclSend | ncclRecv x (nranks - 1) / ncclGroupEnd on `stream`, ordered after the render queued there.
 * The handle must be tile-sharded (vf_terrain_set_tile_shard); it sends exactly its local tiles (local_tiles * 16384
 * bytes) from its current output buffer.  On the root `dev_gathered` is [nranks][stride_tiles][64][64][4]: rank r's slab lands in
 * slot r; the root's own slab is not moved when it rendered straight into slot `root` (vf_terrain_set_output_device), and
 * goes through RCCL to itself otherwise.  `dev_gathered` is ignored on the other ranks. */
int vf_dist_gather_tiles(vf_terrain *t, void *rccl_comm, int root, void *dev_gathered, uint32_t stride_tiles, void *stream);
/* Band shards (vf_terrain_set_shard) -> rank `root`: every band is a contiguous band_h * W * 4-byte slab of the final image,
 * so the root receives each remote band in place in `dev_image` ((H, W, 4), no stitch pass) and copies its own. */
int vf_dist_gather_bands(vf_terrain *t, void *rccl_comm, int root, void *dev_image, void *stream);
/* Tile shards in column stripes (vf_terrain_set_tile_shard with skew 0, any stripe width) -> the row-major (H, W, 4) frame in `dev_image` on rank
 * `root`, with the stitch sharded like the rendering -- no rank copies the whole frame (round 3 measured +40..107 us on the root
 * of eight for a whole-frame stitch, +11 us per rank this way).  One call per frame on every rank, all queued on `stream`:
 *   1. all-to-all (one ncclGroupStart / ncclSend + ncclRecv per peer / ncclGroupEnd): the frame is cut into nranks horizontal
 *      bands of whole tile rows; a rank's slab holds the tiles of band b contiguously and sends that chunk to rank b;
 *   2. k_stitch_tiles on the rank's band (H / nranks rows; the root stitches straight into `dev_image`);
 *   3. the bands are contiguous slabs of the frame: one more group moves them to the root in place.
 * Needs W, H multiples of 64, tile columns that divide by nranks * stripe width and tile rows that divide by nranks (C4: 2, 4, 8
 * ranks with stripes of 4, 2, 1 tiles); every rank checks that, the
 * communicator (rank / size == the handle's shard) and `root` before anything is posted, so all ranks fail together.  The
 * receive chunks and (off the root) the band live in the handle and are reused by the next call: calls on one handle are
 * ordered on one stream or by the caller's events.  `dev_image` is ignored off the root.
 * There is no reference counterpart (single device: src/terrain/mod.rs:277-294); the module surface it extends is
 * src/lib.rs:961-976. */
int vf_dist_exchange_bands(vf_terrain *t, void *rccl_comm, int root, void *dev_image, void *stream);

/* ---- diagnostics: the fragment stage on its own (BASELINE.json north_star names it) ----------------------------
 * Renders the frame vf_terrain_render drew last (the current uniforms before the first render) once with the visibility store enabled (into scratch buffers: the handle's output, feedback
 * and timing state stay as they were), then runs `repeats` launches of the resolve kernel -- visibility (H, W) u32 ->
 * RGBA8 through fs_main + sRGB store (src/shaders/terrain.wgsl:69-91), the same device code the tile kernel runs on its
 * LDS tile -- and reports the average launch time (HIP events) and the number of covered pixels.  Whole-frame handles only.
 * Algorithmic bytes of a launch: 4 W H (visibility) + 4 W H (RGBA8) + 4 Tw Th (heights). */
typedef struct vf_fragment_timing {
    float resolve_ms;        /* average of `repeats` launches */
    uint32_t covered_pixels; /* pixels with a visible primitive */
    uint32_t repeats;
    uint32_t equal_to_frame; /* 1 when the resolved RGBA8 equals the frame the tile kernel produced, byte for byte */
} vf_fragment_timing;
int vf_terrain_debug_fragment_stage(vf_terrain *t, uint32_t repeats, vf_fragment_timing *out);

/* ---- geometry buffers: per-pixel depth, world position, normal and primitive id of a frame ----------
 * Four planes, tightly packed, row-major:
 *   depth      float32 (H, W)      view depth = clip w of the surface at the pixel centre; +inf on background
 *   position   float32 (H, W, 3)   world (x, y, z) of the surface at the pixel centre; 0 on background
 *   normal     float32 (H, W, 3)   unit geometric normal of the visible triangle in world space, n.y >= 0; 0 on background
 *   primitive  uint32  (H, W)      the visibility id: primitive id + 1, 0 = background (what vf_terrain_read_visibility returns)
 * Overlays never show in them.  The arithmetic is fixed bit for bit and does not follow
 * vf_terrain_set_shade_precision.  All three calls describe the frame vf_terrain_render drew last (before the first render: the
 * current uniforms) by drawing it again with the visibility store on, into scratch buffers: the caller's output buffer, the
 * `rendered` state, timing and plan feedback stay as they were (the rule of vf_terrain_read_visibility).  Whole-frame handles
 * only (VF_ERR_INVALID on a band- or tile-sharded handle).  A handle that never calls them allocates and launches nothing for them.
 *
 * vf_terrain_gbuffer_device: device destinations (e.g. a torch tensor's data_ptr); any may be NULL, at least one not; a NULL plane
 * is not computed.  The planes are written asynchronously on `stream` (NULL: the context's stream); later calls on the handle are
 * ordered behind that work by the library.
 * vf_terrain_read_gbuffer: the same into host memory; returns when the planes are there.
 * vf_terrain_pick: "what is under these pixels" -- n pixels (x, y) in, n records of eight 32-bit words out:
 * {depth, x, y, z, nx, ny, nz, id}, the eighth word the id's bits as a uint32_t (not a converted float).  A pixel outside the
 * frame is VF_ERR_INVALID, and nothing is written. */
int vf_terrain_gbuffer_device(vf_terrain *t, float *dev_depth, float *dev_position, float *dev_normal, uint32_t *dev_primitive, void *stream);
int vf_terrain_read_gbuffer(vf_terrain *t, float *depth, float *position, float *normal, uint32_t *primitive);
int vf_terrain_pick(vf_terrain *t, const int32_t *pixels_xy, uint32_t n, float *out8);
/* diagnostics: the average time (HIP events, ms) of `repeats` launches of the geometry-buffer kernel for the plane set `planes`
 * (a combination of the bits below) on the frame rendered last, after one warm-up launch; nothing is read back. */
#define VF_GBUFFER_DEPTH 1u
#define VF_GBUFFER_POSITION 2u
#define VF_GBUFFER_NORMAL 4u
#define VF_GBUFFER_PRIMITIVE 8u
int vf_terrain_debug_gbuffer_stage(vf_terrain *t, uint32_t planes, uint32_t repeats, float *ms);

/* ---- cast sun shadows on the terrain -----------------------------------------------------------------
 * The shadow field is one float32 per grid vertex, (grid, grid) row-major (row j = z index, column i = x index): lit in [0, 1],
 * 1 = the sun reaches the vertex, 1 - strength = fully shadowed.  It comes from the displaced heights the renderer draws and the
 * sun of the uniforms (u[32..34]) by a horizon scan along sheared grid lines; `bias` (the excess of the horizon over the vertex
 * that is still lit) and `softness` (the excess over which lit falls to 1 - strength) are in world height units.  The arithmetic
 * is fixed bit for bit.  The field is computed by the first shadowed frame or field call that needs it and again
 * only after the heights, the sun, spacing, exaggeration or these parameters have changed.
 *
 * vf_terrain_set_shadows: enable != 0 -- vf_terrain_render draws the frame as before, with the visibility store on, then writes
 * again every covered pixel whose interpolated lit is below 1: fs_main with lambert * lit, always in the exact arithmetic, whatever
 * vf_terrain_set_shade_precision says (both shade modes).  Other pixels keep the frame's bytes.  Overlays composite afterwards
 * and are not shadowed; geometry buffers and the diagnostics frames are unaffected.  strength in [0, 1], softness > 0, bias >= 0,
 * all finite, else VF_ERR_INVALID and nothing changes.  Whole-frame handles only: enabling on a band- or tile-sharded handle,
 * sharding a handle with shadows enabled, and vf_terrain_render_batch / _batch_host on a handle with shadows enabled are
 * VF_ERR_INVALID and change nothing.  The parameters are stored also with enable == 0 (the field calls below use them).
 * A handle that never calls any of these allocates and launches nothing for them.
 * vf_terrain_read_shadow_field: the field for the current heights, uniforms and parameters into host memory (grid * grid
 * floats), whether or not shadows are enabled for drawing.
 * vf_terrain_shadow_field_device: the same into device memory, copied asynchronously on `stream` (NULL: the context's stream);
 * later calls on the handle are ordered behind the copy by the library. */
#define VF_SHADOW_STRENGTH 0.7f
#define VF_SHADOW_SOFTNESS 0.02f
#define VF_SHADOW_BIAS 0.002f
int vf_terrain_set_shadows(vf_terrain *t, int enable, float strength, float softness, float bias);
int vf_terrain_read_shadow_field(vf_terrain *t, float *lit);
int vf_terrain_shadow_field_device(vf_terrain *t, float *dev_lit, void *stream);
/* diagnostics: ms[0] the average time (HIP events) of `repeats` computations of the field, ms[1] of `repeats` shade passes, for the
 * frame rendered last (drawn again into scratch buffers), each after one warm-up; and how many times the handle has computed its
 * field so far (the diagnostic launches are not counted). */
int vf_terrain_debug_shadow_stage(vf_terrain *t, uint32_t repeats, float ms[2]);
int vf_terrain_debug_shadow_scans(vf_terrain *t, uint32_t *count);

/* ---- ambient occlusion from a sky-view scan of the height field ------------------------------------
 * The sky-view field is one float32 per grid vertex, (grid, grid) row-major (row j = z index, column i = x index): sky in [0, 1],
 * 1 = open sky.  It comes from the displaced heights the renderer draws and `ndirs` horizontal directions (ux, uz): along the
 * sheared grid line of each direction (the lines of the cast shadows) a vertex looks back `reach` grid cells of Euclidean distance
 * for its horizon slope T; the direction is occluded by 1 - 1 / (1 + T^2), and sky is 1 minus the mean over the directions.  The
 * arithmetic is fixed bit for bit.  The field is computed by the first frame or field call that needs it and again
 * only after the heights, spacing, exaggeration, `reach` or the directions have changed -- not for the sun, the camera or `strength`.
 *
 * vf_terrain_set_ambient: enable != 0 -- vf_terrain_render draws the frame as before, with the visibility store on, then writes
 * again every covered pixel whose interpolated amb = 1 - strength (1 - sky), or whose lit when cast shadows are on as well, is below
 * 1: fs_main with lambert * lit and its shade times amb, always in the exact arithmetic (both shade modes).  Other pixels keep the
 * frame's bytes; with ambient occlusion off nothing changes.  Overlays composite afterwards and are not darkened; geometry buffers
 * and the diagnostics frames are unaffected.  dirs_xz: ndirs pairs (ux, uz), used as given (only the ratio matters), or NULL for
 * the default set, azimuth 360 t / ndirs degrees.  strength in [0, 1], reach in [1, 1024], ndirs in [1, 64], all finite, every
 * direction finite and not (0, 0), else VF_ERR_INVALID and nothing changes.  Whole-frame handles only: enabling on a band- or
 * tile-sharded handle, sharding a handle with it enabled, and vf_terrain_render_batch / _batch_host with it enabled are
 * VF_ERR_INVALID and change nothing.  The parameters are stored also with enable == 0 (the field calls below use them).
 * A handle that never calls any of these allocates and launches nothing for them.
 * vf_terrain_read_sky_view_field: the field for the current heights, uniforms and parameters into host memory (grid * grid floats),
 * whether or not ambient occlusion is enabled for drawing.
 * vf_terrain_sky_view_field_device: the same into device memory, copied asynchronously on `stream` (NULL: the context's stream);
 * later calls on the handle are ordered behind the copy by the library. */
#define VF_AMBIENT_STRENGTH 0.6f
#define VF_AMBIENT_REACH 64.0f
#define VF_AMBIENT_DIRECTIONS 16
#define VF_AMBIENT_REACH_MAX 1024
#define VF_AMBIENT_DIRECTIONS_MAX 64
int vf_terrain_set_ambient(vf_terrain *t, int enable, float strength, float reach, uint32_t ndirs, const float *dirs_xz);
int vf_terrain_read_sky_view_field(vf_terrain *t, float *sky);
int vf_terrain_sky_view_field_device(vf_terrain *t, float *dev_sky, void *stream);
/* diagnostics: ms[0] the average time (HIP events) of `repeats` computations of the field, ms[1] of `repeats` shade passes (with
 * the cast shadows when they are on), for the frame rendered last (drawn again into scratch buffers), each after one warm-up; and
 * how many times the handle has computed its field so far (the diagnostic launches are not counted). */
int vf_terrain_debug_ambient_stage(vf_terrain *t, uint32_t repeats, float ms[2]);
int vf_terrain_debug_ambient_scans(vf_terrain *t, uint32_t *count);

/* ---- a draped image layer: an RGBA raster as the terrain's albedo ----------------------------------
 * One image per handle: (ih, iw) texels of sRGB bytes with straight alpha, row-major, row 0 at the extent's z0 and column 0 at its
 * x0 (as the height array: row = z index, column = x index).  extent = (x0, z0, x1, z1) in the world plane of the grid, whose
 * vertices lie at -1.5 ... 1.5 in x and z; NULL: the whole grid.  It may reach outside the grid or cover a part of it.  The extent
 * is in grid coordinates and is not multiplied by the grid spacing, unlike overlay coordinates, which are in the spaced world.
 *
 * vf_terrain_set_drape: the handle keeps a device copy made at the call (a snapshot; a second call replaces it).  channels 3: RGB,
 * alpha 255.  From then on vf_terrain_render draws the frame as before, with the visibility store on, then writes again every
 * covered pixel the image reaches with a sample that is not transparent: fs_main with the colormap value of each channel replaced
 * by opacity * sample + (1 - opacity * alpha) * colormap, the sample filtered on premultiplied linear values, always in the exact
 * arithmetic (both shade modes), with cast shadows and ambient occlusion as their passes apply them.  Other pixels keep the frame's
 * bytes.  Overlays composite afterwards; geometry buffers and the diagnostics frames are unaffected.
 * 1 <= iw, ih <= VF_DRAPE_SIZE_MAX; extent finite with x1 > x0 and z1 > z0; opacity in [0, 1]; filter VF_DRAPE_NEAREST or
 * VF_DRAPE_LINEAR.  Anything else, a sharded handle (and sharding a handle that holds a drape), and vf_terrain_render_batch /
 * _render_batch_host on a handle that holds a drape are refused with VF_ERR_INVALID and change nothing.
 * vf_terrain_set_drape_device: the same from device memory (iw * ih * 4 bytes, RGBA), copied device to device on `stream` (NULL:
 * the context's stream); later frames of the handle are ordered behind the copy by the library.
 * vf_terrain_clear_drape: frees the copy; the handle draws as before.  A handle that never sets a drape allocates and launches
 * nothing for it.
 * vf_terrain_drape_info: the drape as set; *iw = 0: none (the other outputs are not written then).  Any output may be NULL. */
#define VF_DRAPE_SIZE_MAX 16384
#define VF_DRAPE_NEAREST 0
#define VF_DRAPE_LINEAR 1
int vf_terrain_set_drape(vf_terrain *t, const uint8_t *rgba, uint32_t iw, uint32_t ih, uint32_t channels /* 3 | 4 */,
                         const float extent[4], float opacity, int filter);
int vf_terrain_set_drape_device(vf_terrain *t, const void *dev_rgba /* iw*ih*4 bytes */, uint32_t iw, uint32_t ih,
                                const float extent[4], float opacity, int filter, void *stream);
int vf_terrain_clear_drape(vf_terrain *t);
int vf_terrain_drape_info(const vf_terrain *t, uint32_t *iw, uint32_t *ih, float extent[4], float *opacity, int *filter);  /* iw = 0: none */
/* Diagnostics: mean time in ms of `repeats` back-to-back launches of the drape shade pass alone (with the cast shadows and the
 * ambient occlusion that are on), for the frame rendered last (drawn again into scratch buffers), after one warm-up. */
int vf_terrain_debug_drape_stage(vf_terrain *t, uint32_t repeats, float *ms);   /* the shade pass alone, like the shadow one */

/* ---- a mip pyramid under the draped image, and trilinear filtering ----------------------------------
 * A sampling state of the handle, off by default; like the shadow settings it survives vf_terrain_set_drape and _clear_drape.
 * With it on, a drape is sampled at the level of detail of each pixel's footprint on the image (measured on the surface, from the
 * same primitive one pixel to the right and one below), so an image denser than the frame no longer aliases: `linear` blends the
 * bilinear samples of two levels, `nearest` takes the nearest texel of the nearest level.  Where the image is magnified the sample
 * is the unmipped one, bit for bit.  The footprint is isotropic (the larger of the two axes): at grazing angles it blurs.
 * The pyramid: level 0 is the image; level k >= 1 is max(1, (w + 1) >> 1) x max(1, (h + 1) >> 1) of the level above it, premultiplied
 * linear (r, g, b, a) as four binary16 values per texel, each the mean of the 4, 2 or 1 parents that exist.  It exists only while
 * a drape is held and mipmaps are on, is built on the draw stream by the first frame (or read) after a new image or after enabling,
 * and is not built again while the image rests.  Memory: a third of the image's texel count at 8 bytes each -- 716 MB beside the
 * 1 GiB image at 16384 x 16384.  If that allocation fails the frame is refused with VF_ERR_NOMEM (mipmaps stay on; nothing is
 * drawn unfiltered in its place).
 * vf_terrain_set_drape_mips: bias is added to the level of detail, a finite number in [-16, 16]; anything else is refused with
 *     VF_ERR_INVALID and changes nothing.  Disabling frees the pyramid.  Sharded handles and render_batch stay refused as for the drape.
 * vf_terrain_drape_mip_info: *enabled; *levels (0 without a drape) and *bytes of the pyramid as it is or will be built; *builds
 *     counts the pyramid builds over the handle's life.  Any output may be NULL.
 * vf_terrain_read_drape_level: level 1 <= level < levels as (h, w, 4) binary16 values, after bringing the pyramid up to date; `out`
 *     NULL: the size alone.  Level 0 is the uploaded bytes and has no binary16 form. */
#define VF_DRAPE_MIP_BIAS_MAX 16.0f
#define VF_DRAPE_MIP_LEVELS_MAX 15
int vf_terrain_set_drape_mips(vf_terrain *t, int enabled, float bias);
int vf_terrain_drape_mip_info(const vf_terrain *t, int *enabled, uint32_t *levels, float *bias, uint64_t *bytes, uint32_t *builds);
int vf_terrain_read_drape_level(vf_terrain *t, uint32_t level, uint16_t *out /* h * w * 4, or NULL */, uint32_t *w, uint32_t *h);
/* Diagnostics: mean time in ms of `repeats` back-to-back builds of the whole pyramid, after one warm-up. */
int vf_terrain_debug_drape_mip_build(vf_terrain *t, uint32_t repeats, float *ms);

/* ---- anisotropic filtering of the mip sampling ----
 * An oblique view stretches a pixel's footprint on the image along one axis, and the pyramid's one sample at the level of the longer
 * axis blurs across the shorter.  With a largest anisotropy A > 1 (and mipmaps on) a pixel whose footprint is longer than 1.25 times
 * its width takes up to A samples along the longer of its two screen-axis derivatives, at the level of detail of the shorter
 * (raised where the ratio exceeds A), and writes their mean; every other pixel is the mipped one, bit for bit.  A setting of the
 * handle, 1 by default, that survives set_drape, set_drape_device, clear_drape and mipmaps off / on; with mipmaps off it is kept
 * and has no effect.  It leaves the pyramid as it is: nothing is built again.
 * vf_terrain_set_drape_anisotropy: max_anisotropy 1, 2, 4, 8 or 16; anything else is refused with VF_ERR_INVALID and changes nothing.
 *     1: the frames of vf_terrain_set_drape_mips alone, through the same kernel.
 * vf_terrain_drape_anisotropy: *max_anisotropy as set. */
#define VF_DRAPE_ANISOTROPY_MAX 16
int vf_terrain_set_drape_anisotropy(vf_terrain *t, uint32_t max_anisotropy);
int vf_terrain_drape_anisotropy(const vf_terrain *t, uint32_t *max_anisotropy);

/* ---- viewshed analysis: a line-of-sight field from an observer, and a tint of the frame ------------
 * The viewshed field is one float32 per grid vertex, (grid, grid) row-major (row j = z index, column i = x index): seen in [0, 1],
 * 1 = the observer sees the vertex, 0 = the terrain hides it.  One observer per handle: observer_xz = (x, z) in the overlays' world
 * frame (the one vf_terrain_add_points takes: grid coordinates times the spacing), snapped to the nearest grid vertex; the eye stands
 * eye_height above the surface there, a target target_height above its vertex, both in the units of y = h * exag.  The field comes
 * from the displaced heights the renderer draws by a horizon scan along lines that fan out from the observer's vertex (Franklin's R2
 * rule with true distances); `bias` (the height by which a target may lie below the horizon and still be seen) and `softness` (the
 * height over which seen falls to 0) are in the same units.  The arithmetic is fixed bit for bit.  The field is
 * computed by the first tinted frame or field call that needs it and again only after the heights, exaggeration, the observer's
 * vertex, eye_height, target_height, softness or bias have changed -- not for the colours, the radius, the camera or the sun.
 *
 * vf_terrain_set_viewshed: enable != 0 -- vf_terrain_render draws the frame as before, with the visibility store on, then (behind
 * the shadow, ambient and drape passes) blends over every covered pixel the hidden colour with coverage 1 - s and the visible colour
 * with coverage s, s the interpolated seen value, each as an overlay feature blends (alpha8 / 255 times the coverage, on linear
 * values, the exact sRGB encoder); a colour with alpha 0 blends nothing, and a pixel neither colour touches keeps the frame's bytes.
 * radius > 0: only pixels whose surface point lies within `radius` (world units, horizontal) of the observer's vertex; 0: all.
 * The tint is flat, neither lit nor shadowed; background pixels are never touched.  Overlays composite afterwards; geometry buffers
 * and the diagnostics frames are unaffected.  The colours are {r, g, b, a} bytes.  observer finite, eye_height >= 0,
 * target_height >= 0, radius >= 0, softness > 0, bias >= 0, all finite, else VF_ERR_INVALID and nothing changes.  Whole-frame handles
 * only: enabling on a band- or tile-sharded handle, sharding a handle with a viewshed enabled, and vf_terrain_render_batch /
 * _batch_host on a handle with a viewshed enabled are VF_ERR_INVALID and change nothing.  The parameters are stored also with
 * enable == 0 (the field calls below use them).  observer_xz == NULL (with enable == 0): the observer is forgotten, the defaults are
 * back and everything made for the viewshed is freed.  The setting survives height uploads.  A handle that never calls any of these
 * allocates and launches nothing for them.
 * vf_terrain_read_viewshed_field: the field for the current heights, uniforms, observer and parameters into host memory (grid * grid
 * floats), whether or not the viewshed is enabled for drawing; VF_ERR_INVALID before an observer is set.
 * vf_terrain_viewshed_field_device: the same into device memory, copied asynchronously on `stream` (NULL: the context's stream);
 * later calls on the handle are ordered behind the copy by the library.
 * vf_terrain_viewshed_info: the setting; with an observer (and uniforms) also its vertex (i, j), the vertex's world position
 * (x, y, z) -- where a marker goes -- and the eye's y. */
#define VF_VIEWSHED_EYE_HEIGHT 0.05f
#define VF_VIEWSHED_TARGET_HEIGHT 0.0f
#define VF_VIEWSHED_SOFTNESS 0.02f
#define VF_VIEWSHED_BIAS 0.002f
#define VF_VIEWSHED_VISIBLE_RGBA 0x6060FF40u   /* (64, 255, 96, 96) as r | g << 8 | b << 16 | a << 24 */
#define VF_VIEWSHED_HIDDEN_RGBA 0x00000000u    /* (0, 0, 0, 0): hidden ground keeps the frame's colour */
typedef struct vf_viewshed_info {
    int32_t enabled, has_observer;
    uint32_t vertex[2];       /* (i, j); this and the next two only with an observer */
    float observer_xyz[3];    /* world position of the observer's vertex */
    float eye_y;              /* observer_xyz[1] + eye_height */
    float eye_height, target_height, radius /* 0: none */, softness, bias;
    uint8_t visible_rgba[4], hidden_rgba[4];
} vf_viewshed_info;
int vf_terrain_set_viewshed(vf_terrain *t, int enable, const float observer_xz[2], float eye_height, float target_height, float radius,
                            const uint8_t visible_rgba[4], const uint8_t hidden_rgba[4], float softness, float bias);
int vf_terrain_read_viewshed_field(vf_terrain *t, float *seen);
int vf_terrain_viewshed_field_device(vf_terrain *t, float *dev_seen, void *stream);
int vf_terrain_viewshed_info(vf_terrain *t, vf_viewshed_info *out);
/* diagnostics: ms[0] the average time (HIP events) of `repeats` computations of the field, ms[1] of `repeats` tint passes, for the
 * frame rendered last (drawn again into scratch buffers), each after one warm-up; and how many times the handle has computed its
 * field so far (the diagnostic launches are not counted). */
int vf_terrain_debug_viewshed_stage(vf_terrain *t, uint32_t repeats, float ms[2]);
int vf_terrain_debug_viewshed_scans(vf_terrain *t, uint32_t *count);

/* ---- cumulative viewsheds: how many of N observers see each vertex, and a tint of the frame ---------
 * The count field is one float32 per grid vertex, (grid, grid) row-major as the viewshed field: count in [0, N], the sum over the
 * observers of each one's seen value.  Many observers per handle: observers_xz = count pairs (x, z) in the overlays' world frame, each
 * snapped to a grid vertex as vf_terrain_set_viewshed snaps its one; two observers on one vertex both count.  eye_height,
 * target_height, softness and bias are shared by all observers and mean what they mean there.  Each observer's field is the viewshed
 * field of that observer, bit for bit; it enters the sum as q = rint(seen * 65536), an unsigned 32-bit integer, so the sum does not
 * depend on the order of the observers or on how they are batched, and count = (float)sum / 65536.  radius > 0 (world units): an
 * observer counts only for the vertices within the radius of its own vertex, and no line is walked further than that; 0: no limit.
 * The arithmetic is fixed bit for bit.  The field is computed by the first tinted frame or field call that needs it and
 * again only after the heights, the exaggeration, the observers' vertices, eye_height, target_height, softness, bias or (with a
 * radius) the radius in cells have changed -- not for the colours, the camera or the sun.
 *
 * vf_terrain_set_cumulative_viewshed: enable != 0 -- vf_terrain_render draws the frame as before, with the visibility store on, then
 * (behind the shadow, ambient and drape passes, and behind the single observer's tint if that is on too) blends over every covered
 * pixel low_rgba with coverage 1 - s and high_rgba with coverage s, s the interpolated count / N, as vf_terrain_set_viewshed blends
 * its hidden and visible colours.  Overlays composite afterwards; geometry buffers and the diagnostics frames are unaffected.
 * 1 <= count <= 65535, observers finite, eye_height >= 0, target_height >= 0, radius >= 0, softness > 0, bias >= 0, all finite, else
 * VF_ERR_INVALID and nothing changes.  Whole-frame handles only: enabling on a band- or tile-sharded handle, sharding a handle with a
 * cumulative viewshed enabled, and vf_terrain_render_batch / _batch_host on such a handle are VF_ERR_INVALID and change nothing.  The
 * parameters are stored also with enable == 0 (the field calls below use them).  observers_xz == NULL (with enable == 0): the
 * observers are forgotten, the defaults are back and everything made for them is freed.  The setting survives height uploads.  A
 * handle that never calls any of these allocates and launches nothing for them.
 * vf_terrain_read_cumulative_viewshed_field: the count field for the current heights, uniforms, observers and parameters into host
 * memory (grid * grid floats), whether or not the cumulative viewshed is enabled for drawing; VF_ERR_INVALID before observers are set.
 * vf_terrain_cumulative_viewshed_field_device: the same into device memory, copied asynchronously on `stream` (NULL: the context's
 * stream); later calls on the handle are ordered behind the copy by the library.
 * vf_terrain_cumulative_viewshed_info: the setting, N, and the number of observers a launch took in the last computation (0 before it).
 * vf_terrain_read_cumulative_viewshed_vertices: the observers' vertices (i, j) for the current uniforms, count pairs of uint32. */
#define VF_CUMULATIVE_VIEWSHED_MAX_OBSERVERS 65535u
#define VF_CUMULATIVE_VIEWSHED_HIGH_RGBA 0xA060FF40u   /* (64, 255, 96, 160) as r | g << 8 | b << 16 | a << 24 */
#define VF_CUMULATIVE_VIEWSHED_LOW_RGBA 0x00000000u    /* (0, 0, 0, 0): ground that nobody sees keeps the frame's colour */
typedef struct vf_cumulative_viewshed_info {
    int32_t enabled;
    uint32_t count;           /* N; 0: no observers set */
    uint32_t batch;           /* observers per launch in the last computation */
    float eye_height, target_height, radius /* 0: none */, softness, bias;
    uint8_t high_rgba[4], low_rgba[4];
} vf_cumulative_viewshed_info;
int vf_terrain_set_cumulative_viewshed(vf_terrain *t, int enable, const float *observers_xz /* count x 2 */, uint32_t count, float eye_height,
                                       float target_height, float radius, const uint8_t high_rgba[4], const uint8_t low_rgba[4], float softness,
                                       float bias);
int vf_terrain_read_cumulative_viewshed_field(vf_terrain *t, float *count);
int vf_terrain_cumulative_viewshed_field_device(vf_terrain *t, float *dev_count, void *stream);
int vf_terrain_cumulative_viewshed_info(vf_terrain *t, vf_cumulative_viewshed_info *out);
int vf_terrain_read_cumulative_viewshed_vertices(vf_terrain *t, uint32_t *vertices /* count x 2 */);
/* diagnostics: the number of observers a launch takes (0: as many as the memory budget for the carries holds; the next call computes
 * the field again); how many times the handle has computed its field so far (the diagnostic launches are not counted); and the
 * average time (HIP events) of `repeats` computations of the field, after one warm-up. */
int vf_terrain_debug_cumulative_viewshed_batch(vf_terrain *t, uint32_t batch);
int vf_terrain_debug_cumulative_viewshed_scans(vf_terrain *t, uint32_t *count);
int vf_terrain_debug_cumulative_viewshed_stage(vf_terrain *t, uint32_t repeats, float *ms);

/* ---- sun exposure: the weighted sum of the shadow fields of N suns, and a tint of the frame ----------
 * The exposure field is one float32 per grid vertex, (grid, grid) row-major as the shadow field: exposure in [0, sum of weights], the
 * sum over the suns of lit_o * c_o * w_o.  suns_xyz = count direction vectors (x, y, z) towards the sun, as the uniforms hold the
 * handle's own; they need not be normalised.  lit_o is the shadow field (vf_terrain_read_shadow_field) of that sun at strength 1 with
 * the call's softness and bias, bit for bit.  A sun whose y is not > 0 (on or below the horizon, a zero vector) is not counted: it
 * adds nothing and costs nothing.  weights = count numbers in [0, 1], or NULL: all 1 -- the share of a time step, or the
 * transmittance, that the caller's ephemeris gives a sun.  incidence != 0: c_o is the cosine between the sun and the surface normal
 * of the height field (central differences, one-sided on the grid's edges), clamped to [0, 1], 0 where a height involved is not
 * finite; incidence == 0: c_o = 1.  Each sun's term enters the sum as q = rint(lit * c * w * 65536), an unsigned 32-bit integer, so
 * the sum does not depend on the order of the suns or on how they are batched, and exposure = (float)sum / 65536.  The arithmetic is
 * fixed bit for bit.  The field is computed by the first tinted frame or field call that needs it and again only after
 * the heights, the spacing, the exaggeration, a sun, a weight, incidence, softness or bias have changed -- not for the colours, the
 * camera or the handle's own sun.
 *
 * vf_terrain_set_sun_exposure: enable != 0 -- vf_terrain_render draws the frame as before, with the visibility store on, then (behind
 * the shadow, ambient and drape passes, under both viewshed tints if they are on too) blends over every covered pixel low_rgba with
 * coverage 1 - s and high_rgba with coverage s, s the interpolated f = min(exposure / W, 1), W the sum of the counted suns' weights
 * in list order (f = 0 when W is 0), as vf_terrain_set_viewshed blends its hidden and visible colours.  Overlays composite
 * afterwards; geometry buffers and the diagnostics frames are unaffected.  1 <= count <= 65535, suns and weights finite, weights in
 * [0, 1], softness > 0, bias >= 0, both finite, else VF_ERR_INVALID and nothing changes.  Whole-frame handles only: enabling on a
 * band- or tile-sharded handle, sharding a handle with sun exposure enabled, and vf_terrain_render_batch / _batch_host on such a
 * handle are VF_ERR_INVALID and change nothing.  The parameters are stored also with enable == 0 (the field calls below use them).
 * The setting survives height uploads.  A handle that never calls any of these allocates and launches nothing for them.
 * vf_terrain_clear_sun_exposure: the suns are forgotten, the defaults are back and everything made for them is freed.
 * vf_terrain_read_sun_exposure_field: the exposure field for the current heights, uniforms, suns and parameters into host memory
 * (grid * grid floats), whether or not sun exposure is enabled for drawing; VF_ERR_INVALID before suns are set.
 * vf_terrain_sun_exposure_field_device: the same into device memory, copied asynchronously on `stream` (NULL: the context's stream);
 * later calls on the handle are ordered behind the copy by the library.
 * vf_terrain_sun_exposure_info: the setting, N, the number of counted suns, W, and the number of suns a launch took in the last
 * computation (0 before it). */
#define VF_SUN_EXPOSURE_MAX_SUNS 65535u
#define VF_SUN_EXPOSURE_HIGH_RGBA 0xA040D0FFu   /* (255, 208, 64, 160) as r | g << 8 | b << 16 | a << 24 */
#define VF_SUN_EXPOSURE_LOW_RGBA 0x00000000u    /* (0, 0, 0, 0): ground that no sun reaches keeps the frame's colour */
typedef struct vf_sun_exposure_info {
    int32_t enabled;
    uint32_t count;           /* N; 0: no suns set */
    uint32_t counted;         /* suns above the horizon (y > 0) */
    float weight_total;       /* W: the sum of their weights */
    int32_t incidence;
    uint32_t batch;           /* suns per launch in the last computation */
    float softness, bias;
    uint8_t high_rgba[4], low_rgba[4];
} vf_sun_exposure_info;
int vf_terrain_set_sun_exposure(vf_terrain *t, int enable, const float *suns_xyz /* count x 3 */, const float *weights /* count, or NULL */,
                                uint32_t count, int incidence, float softness, float bias, const uint8_t high_rgba[4], const uint8_t low_rgba[4]);
int vf_terrain_clear_sun_exposure(vf_terrain *t);
int vf_terrain_read_sun_exposure_field(vf_terrain *t, float *exposure);
int vf_terrain_sun_exposure_field_device(vf_terrain *t, float *dev_exposure, void *stream);
int vf_terrain_sun_exposure_info(vf_terrain *t, vf_sun_exposure_info *out);
/* diagnostics: the number of suns a launch takes (0: as many as the memory budget for the carries holds; the next call computes the
 * field again); how many times the handle has computed its field so far (the diagnostic launches are not counted); and the average
 * time (HIP events) of `repeats` computations of the field, after one warm-up. */
int vf_terrain_debug_sun_exposure_batch(vf_terrain *t, uint32_t batch);
int vf_terrain_debug_sun_exposure_scans(vf_terrain *t, uint32_t *count);
int vf_terrain_debug_sun_exposure_stage(vf_terrain *t, uint32_t repeats, float *ms);

/* ---- supersampled terrain frames: factor x factor samples per pixel, resolved on the GPU ----------
 * A handle made with factor f in 1..VF_SUPERSAMPLE_MAX draws its terrain -- set-up, plan, tile kernels, the shadow / ambient / drape
 * passes and the three tints, in their usual order, with the caller's uniforms -- at the SAMPLE SIZE (f width, f height) into a
 * sample buffer of its own, on an ordered grid of f x f samples per pixel.  One kernel then resolves the samples into the
 * width x height frame (the caller's output buffer if one is set, vf_terrain_set_output_device), and the overlays composite onto that
 * frame at width x height: sizes and widths in pixels, the overlays' anti-aliasing and the layer order mean what they mean on any
 * handle.  The resolve, per output pixel and colour channel, bit for bit: the f f sample bytes decoded to linear light through the
 * sRGB8 table, added in binary32 rows outer, columns inner, starting from the first sample; the sum multiplied by the binary32
 * 1.0f / (f f), no fused multiply-add anywhere; encoded as every frame store encodes.  Alpha is the integer mean of the f f alpha
 * bytes, half up.  Every output pixel is rewritten by every frame.
 *
 * vf_terrain_read_rgba, vf_terrain_read_png_scanlines, vf_terrain_rgba_device and vf_terrain_set_output_device deal in
 * width x height.  vf_terrain_read_visibility, the geometry buffers and their device variants describe the samples: their planes
 * are (f height, f width).  vf_terrain_pick takes output pixels and answers for the sample (f x + f / 2, f y + f / 2), integer
 * division.  vf_terrain_local_rows gives the frame's rows, `height`.  factor 1 is vf_terrain_create in every respect: no sample
 * buffer, no resolve, the same launches.
 *
 * VF_ERR_INVALID, with a message that says why and the handle (if any) left as it was: factor outside 1..VF_SUPERSAMPLE_MAX;
 * f width or f height above 16384; and on a handle with f > 1: vf_terrain_set_shard with more than one rank,
 * vf_terrain_set_tile_shard, vf_dist_gather_bands, vf_terrain_render_batch / _batch_host, and any occluding overlay layer
 * (vf_terrain_set_layer_occlusion(..., 1, ...), vf_terrain_add_contours with occlude != 0): the depth test of an occluding layer reads
 * the frame's visibility and set-up records at the output pixel's centre, and those of a supersampled frame are the samples'.
 *
 * vf_terrain_supersampling: the factor and the sample size (any pointer may be NULL).
 * vf_terrain_read_samples: the samples the last vf_terrain_render drew, before the resolve -- terrain and passes, no overlays --
 * into host memory, (f height, f width, 4) bytes row-major.  VF_ERR_INVALID before the first render and on a handle with factor 1,
 * which keeps no samples apart from its frame.
 * vf_terrain_samples_device: the same into device memory, copied asynchronously on `stream` (NULL: the context's stream); later calls
 * on the handle are ordered behind the copy by the library.
 * vf_terrain_debug_resolve_stage: diagnostics -- the average time (HIP events, ms) of `repeats` launches of the resolve kernel on the
 * samples of the frame rendered last, into a scratch frame, after one warm-up launch; the handle's frame stays as it was. */
#define VF_SUPERSAMPLE_MAX 4
int vf_terrain_create_supersampled(vf_ctx *ctx, uint32_t width, uint32_t height, uint32_t grid, const uint8_t lut_rgba8[1024],
                                   int lut_is_srgb, uint32_t factor, vf_terrain **out);
int vf_terrain_supersampling(const vf_terrain *t, uint32_t *factor, uint32_t *sample_width, uint32_t *sample_height);
int vf_terrain_read_samples(vf_terrain *t, uint8_t *dst);
int vf_terrain_samples_device(vf_terrain *t, void *dev_dst, void *stream);
int vf_terrain_debug_resolve_stage(vf_terrain *t, uint32_t repeats, float *ms);

/* ---- atmospheric haze: a distance and height fog pass over the terrain ------------------------------
 * A setting of the handle, off by default.  With haze enabled vf_terrain_render draws the frame as before, with the visibility store
 * on, then -- behind the shadow, ambient and drape passes and the three tints, in front of the resolve of a supersampled handle and
 * of the overlays, which are composited on top and are not hazed -- blends the haze colour over every covered pixel (every sample of
 * a supersampled handle) with the opacity
 *     a = min(1 - exp(-density l g), max_opacity) alpha8 / 255,     l = max(d - start, 0),
 * d the view depth of the surface point (the geometry buffers' depth, clip w) and g the height factor: 1 with falloff == 0 (uniform
 * haze); with falloff > 0 the air's density at world height y is density exp(-(y - base) / falloff) and g is the mean of that
 * exponential along the straight line from the eye's height to the point's.  The blend is the viewshed tint's, on linear values with
 * the exact sRGB encoder; a pixel whose a is not > 0 keeps the frame's bytes.  background != 0: pixels without terrain are blended
 * too, with a = max_opacity alpha8 / 255, the limit of a surface infinitely far away, and keep their alpha byte; 0: they are never
 * touched.  The arithmetic is fixed bit for bit and does not follow vf_terrain_set_shade_precision (which also states
 * the exponential).  The colour is {r, g, b, a} bytes.
 *
 * vf_terrain_set_haze: stores every parameter, also with enable == 0 (the opacity calls below use them).  VF_ERR_INVALID, with a
 * message that says why and nothing changed: density, start or falloff negative or not finite; base not finite; max_opacity outside
 * [0, 1]; rgba == NULL.  Whole-frame handles only: enabling on a band- or tile-sharded handle, sharding a handle with haze enabled,
 * and vf_terrain_render_batch / _batch_host on a handle with haze enabled are VF_ERR_INVALID and change nothing.  The setting survives
 * height uploads, new uniforms, the drape and the vertex fields; it holds no cached field: per frame only the eye's height is formed
 * again, on the host.  A handle that never enables haze allocates and launches nothing for it.
 * vf_terrain_clear_haze: off, the defaults are back, the opacity plane is freed.
 * vf_terrain_haze_info: the settings as stored and, once uniforms are set (has_eye), eye_y of the live uniforms: y of -R^T t of the
 * view matrix.
 * vf_terrain_read_haze_opacity: a of every pixel (0 where the pass leaves the pixel) for the frame rendered last and the stored
 * settings, enabled or not, into host memory: (H, W) float32 of the raster size -- the sample size on a supersampled handle.
 * Produced as the geometry buffers are, only when asked: the frame is drawn again into scratch buffers with its visibility.
 * vf_terrain_haze_opacity_device: the same into device memory on `stream` (NULL: the context's stream); later calls on the handle
 * are ordered behind it by the library.
 * vf_terrain_debug_haze_stage: diagnostics -- the average time (HIP events, ms) of `repeats` launches of the haze pass alone with the
 * stored settings on the frame rendered last (drawn again into scratch buffers), after one warm-up launch. */
#define VF_HAZE_RGBA 0xFFEBD7C8u   /* (200, 215, 235, 255) as r | g << 8 | b << 16 | a << 24 */
typedef struct vf_haze_info {
    int32_t enabled, background;
    float density, start, falloff /* 0: uniform */, base, max_opacity;
    uint8_t rgba[4];
    int32_t has_eye;          /* uniforms are set: eye_y is valid */
    float eye_y;
} vf_haze_info;
int vf_terrain_set_haze(vf_terrain *t, int enable, float density, const uint8_t rgba[4], float start, float falloff /* 0: uniform */, float base,
                        float max_opacity, int background);
int vf_terrain_clear_haze(vf_terrain *t);
int vf_terrain_haze_info(vf_terrain *t, vf_haze_info *out);
int vf_terrain_read_haze_opacity(vf_terrain *t, float *dst);
int vf_terrain_haze_opacity_device(vf_terrain *t, float *dev, void *stream);
int vf_terrain_debug_haze_stage(vf_terrain *t, uint32_t repeats, float *ms);

/* ---- flood analysis: what is under water at a level and reachable from its sources, and a water tint --
 * The flood field is one float32 per grid vertex, (grid, grid) row-major (row j = z index, column i = x index): depth = level - h where
 * the vertex is flooded, 0 elsewhere.  h is the displaced height of the vertex as the renderer draws it, and `level` is in units of h
 * before exaggeration, exactly as contour levels are: vf_terrain_add_contours with the same level draws the shoreline.  A vertex is
 * wet-able when h is finite and h < level; a non-finite vertex is never wet and blocks water.  A vertex is flooded when it is wet-able
 * and 4-connected to a source through wet-able vertices: grid edges connect, diagonals do not, so a dike one vertex wide holds also
 * where it runs diagonally.  The sources, by `mode`: VF_FLOOD_EVERYWHERE -- every wet-able vertex is flooded (the plain bathtub);
 * VF_FLOOD_EDGES -- every wet-able vertex on the border of the grid; VF_FLOOD_SEEDS -- seeds_xz = count pairs (x, z) in the overlays'
 * world frame, each snapped to a grid vertex as vf_terrain_set_viewshed snaps its observer; duplicates are allowed and a seed on a
 * vertex that is not wet-able is no source.  The flooded set is the least fixpoint, so the field is fixed bit for bit whatever the
 * order of evaluation.  It is computed by the first tinted frame or field call that needs it and again only after the
 * heights, the level, the mode or the seeds' vertices have changed -- not for the colours, depth_full, the camera, the sun or the
 * exaggeration; the spacing counts only through where the seeds snap.
 *
 * vf_terrain_set_flood: enable != 0 -- vf_terrain_render draws the frame as before, with the visibility store on, then (behind the
 * shadow, ambient and drape passes, under the sun-exposure and viewshed tints, the haze, the resolve of a supersampled handle and the
 * overlays) paints the water: for a covered pixel of a primitive with a flooded vertex and three finite wd = level - h, d = wd
 * interpolated at the pixel centre; where d > 0, s = min(d / depth_full, 1) and shallow_rgba is blended over the pixel with coverage
 * 1 - s, then deep_rgba with coverage s, as vf_terrain_set_viewshed blends its colours.  The waterline follows the level inside the
 * shoreline triangles; the tint is flat (not lit, not shadowed); water can show in a triangle whose only flooded vertex is diagonal to
 * an unflooded wet-able one.  Geometry buffers and the diagnostics frames are unaffected.  VF_ERR_INVALID, nothing changed: level not
 * finite; depth_full not > 0 or not finite; an unknown mode; with VF_FLOOD_SEEDS count outside 1 <= count <= 65535, seeds_xz == NULL or
 * a seed that is not finite (seeds_xz and count are ignored in the other modes).  Whole-frame handles only: enabling on a band- or
 * tile-sharded handle, sharding a handle with a flood enabled, and vf_terrain_render_batch / _batch_host on such a handle are
 * VF_ERR_INVALID and change nothing.  The parameters are stored also with enable == 0 (the field calls below use them).  The setting
 * survives height uploads.  A handle that never calls any of these allocates and launches nothing for them.
 * vf_terrain_clear_flood: off, the defaults are back and everything made for the flood is freed.
 * vf_terrain_read_flood_field: the field for the current heights, uniforms, level and sources into host memory (grid * grid floats),
 * whether or not the flood is enabled for drawing; VF_ERR_INVALID before a flood is set.
 * vf_terrain_flood_field_device: the same into device memory, copied asynchronously on `stream` (NULL: the context's stream); later
 * calls on the handle are ordered behind the copy by the library.
 * vf_terrain_flood_info: the setting and, of the last computation of the field (0 before it), the flooded and the wet-able vertices,
 * the launches of the propagation kernel up to and including the first that changed nothing (0 in mode EVERYWHERE), how many times the
 * field was computed, and the passes queued per read-back.
 * vf_terrain_read_flood_seeds: the seeds' vertices (i, j) for the current uniforms, count pairs of uint32. */
#define VF_FLOOD_EVERYWHERE 0
#define VF_FLOOD_EDGES 1
#define VF_FLOOD_SEEDS 2
#define VF_FLOOD_MAX_SEEDS 65535u
#define VF_FLOOD_SHALLOW_RGBA 0x80E0B060u   /* (96, 176, 224, 128) as r | g << 8 | b << 16 | a << 24 */
#define VF_FLOOD_DEEP_RGBA 0xE0A04010u      /* (16, 64, 160, 224) */
#define VF_FLOOD_DEPTH_FULL 0.1f
typedef struct vf_flood_info {
    int32_t enabled, has_flood;
    int32_t mode;
    uint32_t count;           /* seeds; 0 in the other modes */
    float level, depth_full;
    uint8_t shallow_rgba[4], deep_rgba[4];
    uint32_t flooded_vertices, wettable_vertices, passes, scans, group;
} vf_flood_info;
int vf_terrain_set_flood(vf_terrain *t, int enable, float level, int mode, const float *seeds_xz /* count x 2 */, uint32_t count,
                         const uint8_t shallow_rgba[4], const uint8_t deep_rgba[4], float depth_full);
int vf_terrain_clear_flood(vf_terrain *t);
int vf_terrain_read_flood_field(vf_terrain *t, float *depth);
int vf_terrain_flood_field_device(vf_terrain *t, float *dev_depth, void *stream);
int vf_terrain_flood_info(vf_terrain *t, vf_flood_info *out);
int vf_terrain_read_flood_seeds(vf_terrain *t, uint32_t *vertices /* count x 2 */);
/* diagnostics: how many times the handle has computed its field so far; and the number of propagation passes queued per read-back of
 * their `changed` words (0: the default; at most 64; the next call computes the field again); and the average time (HIP events,
 * ms) of `repeats` computations of the field (ms[0]: every launch and every read-back of the host's loop) and of `repeats` launches of
 * the tint pass (ms[1]) on the frame rendered last, drawn again into scratch buffers, each after one warm-up; it needs the flood
 * enabled. */
int vf_terrain_debug_flood_scans(vf_terrain *t, uint32_t *count);
int vf_terrain_debug_flood_group(vf_terrain *t, uint32_t group);
int vf_terrain_debug_flood_stage(vf_terrain *t, uint32_t repeats, float ms[2]);

/* ---- spill analysis: the level the water must reach at its sources before a vertex gets wet, and a sink tint --
 * The spill field is one float32 per grid vertex, (grid, grid) row-major (row j = z index, column i = x index): the minimum, over
 * 4-connected paths of passable vertices from a source to the vertex, of the maximum h on the path, both ends counted; +inf where no
 * path arrives and where the vertex is not passable.  h is the displaced height of the vertex as the renderer draws it, in the units
 * of contour and flood levels.  A vertex is passable when h is finite; a non-finite vertex is never reached and blocks water.  All
 * comparisons take the total order of key(x) = bits ^ (sign ? 0xFFFFFFFF : 0x80000000): the float order on finite values, -0 below
 * +0.  The sources, by `mode`: VF_SPILL_EDGES -- every passable vertex on the border of the grid: the field is the depression-filled
 * surface; VF_SPILL_SEEDS -- seeds_xz = count pairs (x, z) in the overlays' world frame, each snapped to a grid vertex as
 * vf_terrain_set_flood snaps its seeds; duplicates are allowed and a seed on a vertex that is not passable is no source: the set
 * spill < L is what vf_terrain_set_flood floods at level L from the same seeds.  The field is the greatest fixpoint of a relaxation
 * of min and max of input heights, so it is fixed bit for bit whatever the order of evaluation.  The sink depth is
 * sd = spill - h where that is finite, 0 elsewhere: the depth of the closed basins.  The field is computed by the first tinted frame
 * or field call that needs it and again only after the heights, the mode or the seeds' vertices have changed -- not for the colours,
 * depth_full, the camera, the sun or the exaggeration; the spacing counts only through where the seeds snap.
 *
 * vf_terrain_set_spill: enable != 0 -- vf_terrain_render draws the frame as before, with the visibility store on, then (directly
 * behind the flood's water, under the sun-exposure and viewshed tints, the haze, the resolve of a supersampled handle and the overlays)
 * paints the sinks: for a covered pixel of a primitive with three finite sd that are not all 0, d = sd interpolated at the pixel
 * centre; where d > 0, s = min(d / depth_full, 1) and shallow_rgba is blended over the pixel with coverage 1 - s, then deep_rgba with
 * coverage s, as vf_terrain_set_flood blends its colours.  Geometry buffers and the diagnostics frames are unaffected.
 * VF_ERR_INVALID, nothing changed: depth_full not > 0 or not finite; an unknown mode; with VF_SPILL_SEEDS count outside
 * 1 <= count <= 65535, seeds_xz == NULL or a seed that is not finite (seeds_xz and count are ignored with VF_SPILL_EDGES).
 * Whole-frame handles only: enabling on a band- or tile-sharded handle, sharding a handle with the spill enabled, and
 * vf_terrain_render_batch / _batch_host on such a handle are VF_ERR_INVALID and change nothing.  The parameters are stored also with enable == 0 (the field
 * calls below use them).  The setting survives height uploads.  A handle that never calls any of these allocates and launches nothing
 * for them.
 * vf_terrain_clear_spill: off, the defaults are back and everything made for the spill is freed.
 * vf_terrain_read_spill_field: the spill field for the current heights, uniforms and sources into host memory (grid * grid floats),
 * whether or not the spill is enabled for drawing; VF_ERR_INVALID before vf_terrain_set_spill.
 * vf_terrain_spill_field_device: the same into device memory, copied asynchronously on `stream` (NULL: the context's stream); later
 * calls on the handle are ordered behind the copy by the library.
 * vf_terrain_read_sink_depth: the sink depth into host memory (grid * grid floats); VF_ERR_INVALID before vf_terrain_set_spill.
 * vf_terrain_spill_info: the setting and, of the last computation of the field (0 before it), the vertices a path reaches, the
 * vertices with a finite sd > 0, the launches of the relaxation kernel up to and including the first that changed nothing, the tiles
 * that did not leave such a launch at once (their activity word was set), how many times the field was computed, and the passes
 * queued per read-back.
 * vf_terrain_read_spill_seeds: the seeds' vertices (i, j) for the current uniforms, count pairs of uint32. */
#define VF_SPILL_EDGES 1
#define VF_SPILL_SEEDS 2
#define VF_SPILL_MAX_SEEDS 65535u
#define VF_SPILL_SHALLOW_RGBA 0x80E0B060u   /* (96, 176, 224, 128) as r | g << 8 | b << 16 | a << 24 */
#define VF_SPILL_DEEP_RGBA 0xE0A04010u      /* (16, 64, 160, 224) */
#define VF_SPILL_DEPTH_FULL 0.1f
#define VF_SPILL_GROUP_NO_FLAGS 0x80000000u /* vf_terrain_debug_spill_group: or-ed into `group`, every tile runs in every pass */
typedef struct vf_spill_info {
    int32_t enabled, has_spill;
    int32_t mode;
    uint32_t count;           /* seeds; 0 with VF_SPILL_EDGES */
    float depth_full;
    uint8_t shallow_rgba[4], deep_rgba[4];
    uint32_t reached_vertices, sink_vertices, passes, scans, group, tile_runs;
} vf_spill_info;
int vf_terrain_set_spill(vf_terrain *t, int enable, int mode, const float *seeds_xz /* count x 2 */, uint32_t count,
                         const uint8_t shallow_rgba[4], const uint8_t deep_rgba[4], float depth_full);
int vf_terrain_clear_spill(vf_terrain *t);
int vf_terrain_read_spill_field(vf_terrain *t, float *spill);
int vf_terrain_spill_field_device(vf_terrain *t, float *dev_spill, void *stream);
int vf_terrain_read_sink_depth(vf_terrain *t, float *depth);
int vf_terrain_spill_info(vf_terrain *t, vf_spill_info *out);
int vf_terrain_read_spill_seeds(vf_terrain *t, uint32_t *vertices /* count x 2 */);
/* diagnostics: how many times the handle has computed its field so far; and the number of relaxation passes queued per read-back of
 * their `changed` words (0: the default; at most 64; VF_SPILL_GROUP_NO_FLAGS or-ed in: the activity flags are ignored; the next call
 * computes the field again); and the average time (HIP events, ms) of `repeats` computations of the field (ms[0]: every launch and
 * every read-back of the host's loop) and of `repeats` launches of the tint pass (ms[1]) on the frame rendered last, drawn again into
 * scratch buffers, each after one warm-up; it needs the spill enabled. */
int vf_terrain_debug_spill_scans(vf_terrain *t, uint32_t *count);
int vf_terrain_debug_spill_group(vf_terrain *t, uint32_t group);
int vf_terrain_debug_spill_stage(vf_terrain *t, uint32_t repeats, float ms[2]);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_H */

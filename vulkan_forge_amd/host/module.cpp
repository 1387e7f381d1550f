// module.cpp -- CPython extension `_vulkan_forge`: the C++ host side above the C-ABI (include/vf_hip.h).
//
// Mirrors the Python-visible surface the reference registers in src/lib.rs:961-976 (names, signatures,
// return types, exception classes and messages) for the terrain-raster hot path:
//   classes   Renderer (triangle path), TerrainSpike, Scene
//   functions enumerate_adapters, device_probe, grid_generate, colormap_supported,
//             camera_look_at, camera_perspective, camera_view_proj
// All rendering goes through libvf_hip.so; there is no CPU fallback -- without a HIP device every
// object that needs the GPU raises RuntimeError("No suitable GPU adapter") like the reference.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include <sys/mman.h>

#include "../../include/vf_hip.h"
#include "../data/colormaps_rgba8.h"
#include "camera.hpp"
#include "png_writer.hpp"

namespace py = pybind11;
using namespace vfh;

namespace {

// ---- colormap registry: src/colormap/mod.rs --------------------------------------------------
const char *const kSupported[3] = { "viridis", "magma", "terrain" };   // :7 (case-sensitive)

std::string unknown_colormap(const std::string &name)
{
    return "Unknown colormap '" + name + "'. Supported: viridis, magma, terrain";   // :16,:32,:39
}
const uint8_t *resolve_lut(const std::string &name)
{
    if (name == "viridis") return VF_LUT_VIRIDIS;
    if (name == "magma") return VF_LUT_MAGMA;
    if (name == "terrain") return VF_LUT_TERRAIN;
    throw std::runtime_error(unknown_colormap(name));
}
// to_linear_u8_rgba, src/colormap/mod.rs:59-79 (the Rgba8Unorm fallback bytes)
void to_linear_u8_rgba(const uint8_t *src, uint8_t *dst)
{
    for (int i = 0; i < 256; ++i) {
        for (int ch = 0; ch < 3; ++ch) {
            float s = (float)src[4 * i + ch] / 255.0f;
            float l = s <= 0.04045f ? s / 12.92f : std::pow((s + 0.055f) / 1.055f, 2.4f);
            l = l < 0.0f ? 0.0f : (l > 1.0f ? 1.0f : l);
            dst[4 * i + ch] = (uint8_t)(l * 255.0f + 0.5f);
        }
        dst[4 * i + 3] = src[4 * i + 3];
    }
}

// ---- HIP context: one per process and device, like the reference's OnceCell (src/lib.rs:23-61) ----
[[noreturn]] void raise_vf(int rc)
{
    if (rc == VF_ERR_NO_DEVICE) throw std::runtime_error("No suitable GPU adapter");
    throw std::runtime_error(std::string(vf_last_error()));
}
void check(int rc) { if (rc != VF_OK) raise_vf(rc); }

int device_ordinal()
{
    const char *e = std::getenv("VF_HIP_DEVICE");
    return e ? std::atoi(e) : 0;
}

struct Ctx {
    vf_ctx *c = nullptr;
    ~Ctx() { /* process lifetime: the HIP runtime may already be torn down at exit */ }
};
vf_ctx *global_ctx()
{
    static std::mutex mu;
    static Ctx ctx;
    std::lock_guard<std::mutex> lk(mu);
    if (!ctx.c) check(vf_ctx_create(device_ordinal(), &ctx.c));
    return ctx.c;
}

// ---- frame-sized read-back buffers in page-locked host memory (round 5) ---------------------------------------------------------
// render_rgba returns a NumPy array OVER such a buffer instead of copying the frame into fresh pageable memory: the device writes it
// with one DMA transfer (C4: 64 MiB in 1.2 ms) where the staged copy into untouched pages was page-fault bound (2-5 ms; the
// reference maps a fresh buffer per call, src/terrain/mod.rs:446-451).  The array owns its buffer through a capsule; when the array
// dies the buffer goes back to the pool, so a render loop alternates between two buffers and never allocates again.  A buffer is
// 2 MiB-aligned huge-page memory registered with the runtime (vf_host_alloc): 2.6 ms to make for a C4 frame, where hipHostMalloc took 9.
class PinnedPool {
public:
    static PinnedPool &get() { static PinnedPool *p = new PinnedPool; return *p; }   // (process lifetime: never destroyed, like the context)
    void *take(size_t bytes)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t k = 0; k < idle.size(); ++k)
                if (idle[k].second == bytes) { void *p = idle[k].first; idle.erase(idle.begin() + (long)k); return p; }
        }
        void *p = nullptr;
        check(vf_host_alloc(bytes, &p));
        { std::lock_guard<std::mutex> lk(mu); made_bytes += bytes; }
        return p;
    }
    // ... for a caller that can do without: nullptr once `max_out` bytes of page-locked memory are out with arrays the caller keeps.
    // render_rgba allows three frames (round 6): a loop that DROPS its frames alternates between two pooled buffers for good, a loop
    // that KEEPS them gets ordinary arrays from the fourth on -- filled through the handle's ring of pinned chunks by four host threads,
    // 2.1 ms for a C4 frame, where a page-locked buffer of its own per frame costs 2.6 ms to make on top of the 1.3 ms transfer (round
    // 5: 4.9 ms per kept frame) and cannot be swapped.  render_batch allows kMaxOutBytes.
    void *take_or_null(size_t bytes, size_t max_out)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            bool have = false;
            size_t held = 0;
            for (auto &b : idle) { have |= b.second == bytes; held += b.second; }
            if (!have && (made_bytes - held) + bytes > max_out) return nullptr;
        }
        return take(bytes);
    }
    static constexpr size_t kMaxOutBytes = (size_t)1 << 30;
    void give(void *p, size_t bytes)
    {
        std::vector<void *> drop;
        {
            std::lock_guard<std::mutex> lk(mu);
            idle.emplace_back(p, bytes);
            size_t held = 0;
            for (auto &b : idle) held += b.second;
            while (idle.size() > kMaxIdle || held > kMaxIdleBytes) { held -= idle.front().second; made_bytes -= idle.front().second; drop.push_back(idle.front().first); idle.erase(idle.begin()); }
        }
        for (void *d : drop) vf_host_free(d);
    }
private:
    static constexpr size_t kMaxIdle = 4, kMaxIdleBytes = (size_t)1 << 30;
    size_t made_bytes = 0;                                      // page-locked and not freed: idle buffers + those out with arrays
    std::mutex mu;
    std::vector<std::pair<void *, size_t>> idle;
};
struct PinnedLease { void *p; size_t bytes; };
py::capsule pinned_owner(void *p, size_t bytes)
{
    return py::capsule(new PinnedLease{ p, bytes }, [](void *v) { auto *l = static_cast<PinnedLease *>(v); PinnedPool::get().give(l->p, l->bytes); delete l; });
}

// PyO3's `&mut self` borrow (Threading): a method entered while another thread is inside one of the same object
// raises RuntimeError("Already borrowed") instead of racing.  It matters here because render / read-back release the GIL:
// per-handle state (plan sets, pinned read-back buffers, frame counters) is not synchronised below the C-ABI ("calls on one
// handle are not re-entrant", include/vf_hip.h).
class Borrow {
public:
    explicit Borrow(std::atomic<bool> &flag, const char *what = "Already borrowed") : f(flag)
    {
        bool expected = false;
        if (!f.compare_exchange_strong(expected, true, std::memory_order_acquire)) throw std::runtime_error(what);
    }
    ~Borrow() { f.store(false, std::memory_order_release); }
    Borrow(const Borrow &) = delete;
    Borrow &operator=(const Borrow &) = delete;
private:
    std::atomic<bool> &f;
};

Vec3 v3(const std::tuple<float, float, float> &t) { return { std::get<0>(t), std::get<1>(t), std::get<2>(t) }; }

// The sun direction of an elevation and an azimuth in degrees (src/lib.rs:441-462): what set_sun stores and set_sun_exposure's angle
// form hands on, so one sun given by angles has the bits of the handle's own
Vec3 sun_from_angles(float elevation_deg, float azimuth_deg)
{
    const float k = 3.14159265358979323846f / 180.0f;
    const float el = elevation_deg * k, az = azimuth_deg * k;
    return normalize_or_zero({ std::cos(el) * std::cos(az), std::sin(el), std::cos(el) * std::sin(az) });
}

// mat4_to_numpy, src/camera.rs:94-112: (4,4) float32 C-contiguous in mathematical (row, col) indexing
py::array_t<float> mat4_to_numpy(const Mat4 &m)
{
    py::array_t<float> a({ 4, 4 });
    auto r = a.mutable_unchecked<2>();
    for (int row = 0; row < 4; ++row)
        for (int col = 0; col < 4; ++col) r(row, col) = m[4 * col + row];
    return a;
}

// ---- what the bound methods say more than once --------------------------------------------------------------------
// The callable `fn` of the rules in vulkan_forge_amd/<module>.py.  A call of it touches Python objects: never under a released GIL.  An
// `*_args` / `*_params` rule may refuse its arguments, so a method calls it BEFORE it borrows the object (the two that need a figure
// of the handle first, contour_args and mip_level, get it in a borrow of its own or say why not); the `*_info` rules only shape a result.
py::object rules(const char *module, const char *fn) { return py::module_::import((std::string("vulkan_forge_amd.") + module).c_str()).attr(fn); }
// a colour as the rules return it, a tuple of four ints, -> the bytes a C call takes; and four values of an info record -> a tuple
void rgba4(const py::object &colour, uint8_t out[4])
{
    py::tuple c = colour.cast<py::tuple>();
    for (int k = 0; k < 4; ++k) out[k] = c[k].cast<uint8_t>();
}
template <class T> py::tuple tuple4(const T *v) { return py::make_tuple(v[0], v[1], v[2], v[3]); }

// ---- TerrainSpike / Scene -----------------------------------------------------------------------
class TerrainObject {
public:
    // kind 0: TerrainSpike::new (src/terrain/mod.rs:259-407); kind 1: Scene::new (src/scene/mod.rs:60-206)
    // supersample: f x f samples per pixel, resolved on the GPU (argument rules: vulkan_forge_amd/_supersample.py)
    TerrainObject(int kind, uint32_t width, uint32_t height, py::object grid, py::object colormap, py::object supersample) : W(width), H(height)
    {
        ss = rules("_supersample", "supersample_args")(width, height, supersample).cast<uint32_t>();
        SW = ss * W; SH = ss * H;
        uint32_t g = grid.is_none() ? 128u : grid.cast<uint32_t>();
        n = g < 2 ? 2 : g;
        std::string cmap = colormap.is_none() ? "viridis" : colormap.cast<std::string>();
        bool known = false;
        for (const char *s : kSupported) known |= cmap == s;
        if (!known) throw std::runtime_error(unknown_colormap(cmap));
        const uint8_t *srgb_bytes = resolve_lut(cmap);
        // ColormapLUT::new format selection (src/terrain/mod.rs:45-60): sRGB sampling is always
        // available here, so only VF_FORCE_LUT_UNORM selects the CPU-linearised UNORM bytes.
        bool force_unorm = std::getenv("VF_FORCE_LUT_UNORM") != nullptr;
        uint8_t lin[1024];
        if (force_unorm) to_linear_u8_rgba(srgb_bytes, lin);
        lut_format = force_unorm ? "Rgba8Unorm" : "Rgba8UnormSrgb";

        check(vf_terrain_create_supersampled(global_ctx(), W, H, n, force_unorm ? lin : srgb_bytes, force_unorm ? 0 : 1, ss, &t));

        // build_view_matrices (src/terrain/mod.rs:681-691) / SceneGlobals::default (src/scene/mod.rs:17-23,119)
        view = look_at_rh({ 3.f, 2.f, 3.f }, { 0.f, 0.f, 0.f }, { 0.f, 1.f, 0.f });
        proj = perspective_wgpu(to_radians(45.0f), (float)W / (float)H, 0.1f, 100.0f);
        if (kind == 0) globals.sun_dir = normalize({ 0.5f, 1.0f, 0.3f });   // R4 override, src/terrain/mod.rs:325-327
        push_uniforms();
        if (kind == 1) {
            const float dummy[4] = { 0.00f, 0.25f, 0.50f, 0.75f };   // 2x2 gradient, src/scene/mod.rs:142-189
            check(vf_terrain_set_height(t, dummy, 2, 2));
        }
    }
    ~TerrainObject() { if (t) vf_terrain_destroy(t); }
    TerrainObject(const TerrainObject &) = delete;
    TerrainObject &operator=(const TerrainObject &) = delete;

    // src/terrain/mod.rs:498-535, src/scene/mod.rs:208-224
    void set_camera_look_at(std::tuple<float, float, float> eye, std::tuple<float, float, float> target,
                            std::tuple<float, float, float> up, float fovy_deg, float znear, float zfar)
    {
        Borrow b(busy);
        float aspect = (float)W / (float)H;
        validate_camera_params(v3(eye), v3(target), v3(up), fovy_deg, znear, zfar);
        view = look_at_rh(v3(eye), v3(target), v3(up));
        proj = perspective_wgpu(to_radians(fovy_deg), aspect, znear, zfar);
        push_uniforms();
    }

    // Scene::set_height_from_r32f, src/scene/mod.rs:226-276
    void set_height_from_r32f(py::object obj)
    {
        if (!py::isinstance<py::array>(obj)) throw py::type_error("argument 'height_r32f': expected a 2-D numpy.ndarray of float32");
        py::array arr = py::reinterpret_borrow<py::array>(obj);
        if (arr.ndim() != 2 || !arr.dtype().is(py::dtype::of<float>()))
            throw py::type_error("argument 'height_r32f': expected a 2-D numpy.ndarray of float32");
        if (!(arr.flags() & py::array::c_style)) throw std::runtime_error("height must be C-contiguous float32[H,W]");
        uint32_t h = (uint32_t)arr.shape(0), w = (uint32_t)arr.shape(1);
        Borrow b(busy);
        check(vf_terrain_set_height(t, static_cast<const float *>(arr.data()), w, h));
        frame_current = false;
    }

    void render_into(uint8_t *dst, uint32_t rows)          // caller holds the borrow
    {
        py::gil_scoped_release nogil;
        int rc = vf_terrain_render(t, nullptr);
        frame_current = rc == VF_OK;
        if (rc == VF_OK) rc = vf_terrain_read_rgba(t, dst, 0, rows);
        if (rc != VF_OK) { py::gil_scoped_acquire gil; raise_vf(rc); }
    }
    std::vector<uint8_t> render_pixels()                    // caller holds the borrow
    {
        uint32_t rows = 0;
        check(vf_terrain_local_rows(t, &rows));
        std::unique_ptr<uint8_t[]> raw(new uint8_t[(size_t)rows * W * 4]);     // not value-initialised: every byte is overwritten
        render_into(raw.get(), rows);
        return std::vector<uint8_t>(raw.get(), raw.get() + (size_t)rows * W * 4);
    }

    // render_png, src/terrain/mod.rs:409-491, src/scene/mod.rs:278-335
    void render_png(const std::string &path)
    {
        Borrow b(busy);
        uint32_t rows = 0;
        check(vf_terrain_local_rows(t, &rows));
        if (rows != H) {                                       // band-sharded handle: its rows only, filtered on the host
            std::vector<uint8_t> px = render_pixels();
            py::gil_scoped_release nogil;
            write_png_rgba8(path, px.data(), W, rows);
            return;
        }
        // whole frame: the GPU filters the scanlines into pinned host memory, the host deflates them in parallel
        py::gil_scoped_release nogil;
        const uint8_t *scan = nullptr;
        size_t nbytes = 0;
        int rc = vf_terrain_render(t, nullptr);
        frame_current = rc == VF_OK;
        if (rc == VF_OK) rc = vf_terrain_read_png_scanlines(t, &scan, &nbytes);
        if (rc != VF_OK) { py::gil_scoped_acquire gil; raise_vf(rc); }
        write_png_scanlines(path, scan, W, H);
    }

    // extension (not in the reference): the frame as (H, W, 4) uint8 without the PNG round trip
    py::array_t<uint8_t> render_rgba()
    {
        Borrow b(busy);
        uint32_t rows = 0;
        check(vf_terrain_local_rows(t, &rows));
        const size_t bytes = (size_t)rows * W * 4;
        // small frames: an ordinary array.  (Round 5 kept an object's FIRST frame-sized result in ordinary memory too, when page-locking
        // a C4 frame cost 9 ms; huge pages + registration make the buffer in 2.6 ms, less than the page faults of one copy into fresh
        // memory -- vf_host_alloc, tools/micro/pin_cost.hip.)
        if (bytes < ((size_t)4 << 20) || std::getenv("VF_RGBA_PAGEABLE")) {
            py::array_t<uint8_t> a({ (py::ssize_t)rows, (py::ssize_t)W, (py::ssize_t)4 });
            render_into(a.mutable_data(), rows);
            return a;
        }
        // frame-sized: the array lives in page-locked memory from the pool (above) -- one DMA transfer, no host copy
        void *p = PinnedPool::get().take_or_null(bytes, 3 * bytes);
        if (!p) {                                                // (the caller keeps its frames: ordinary arrays from here on)
            // ... in huge pages where the host has them: the copy out of the pinned ring into a fresh array is page-fault bound, and a
            // 2 MiB page takes one fault where 4 KiB pages take 512
            constexpr size_t kHuge = (size_t)2 << 20;
            void *q = nullptr;
            const size_t r = (bytes + kHuge - 1) & ~(kHuge - 1);
            if (posix_memalign(&q, kHuge, r) == 0) {
                (void)madvise(q, r, MADV_HUGEPAGE);
                py::capsule owner(q, [](void *v) { std::free(v); });
                render_into(static_cast<uint8_t *>(q), rows);
                return py::array_t<uint8_t>({ (py::ssize_t)rows, (py::ssize_t)W, (py::ssize_t)4 }, static_cast<uint8_t *>(q), owner);
            }
            py::array_t<uint8_t> a({ (py::ssize_t)rows, (py::ssize_t)W, (py::ssize_t)4 });
            render_into(a.mutable_data(), rows);
            return a;
        }
        py::capsule owner = pinned_owner(p, bytes);             // (returns the buffer if anything below throws)
        render_into(static_cast<uint8_t *>(p), rows);
        return py::array_t<uint8_t>({ (py::ssize_t)rows, (py::ssize_t)W, (py::ssize_t)4 }, static_cast<uint8_t *>(p), owner);
    }
    // extension (BASELINE config 5, "batch of camera look-ats over one terrain"): every pose is what set_camera_look_at + render
    // does per pose (src/scene/mod.rs:208-224, :278-335), queued back to back on the GPU; poses = sequence of
    // (eye, target, up, fovy_deg, znear, zfar).  Returns the frames as a list of (H, W, 4) uint8 arrays, or -- with `paths`, one per
    // pose -- writes PNG files and returns None.  The camera afterwards is the last pose's, as after the per-pose loop.
    py::object render_batch(py::sequence poses, py::object paths)
    {
        Borrow b(busy);
        uint32_t rows = 0;
        check(vf_terrain_local_rows(t, &rows));
        if (rows != H) throw std::runtime_error("render_batch needs the whole frame on one object (a band shard renders its rows with render_rgba)");
        const size_t n = (size_t)py::len(poses);
        std::vector<std::string> files;
        if (!paths.is_none()) {
            files = paths.cast<std::vector<std::string>>();
            if (files.size() != n) throw py::value_error("paths must hold one file name per pose");
        }
        const float aspect = (float)W / (float)H;
        std::vector<float> blocks(44 * n);
        Mat4 v{}, p{};
        for (size_t k = 0; k < n; ++k) {
            auto pose = poses[k].cast<std::tuple<std::tuple<float, float, float>, std::tuple<float, float, float>, std::tuple<float, float, float>, float, float, float>>();
            validate_camera_params(v3(std::get<0>(pose)), v3(std::get<1>(pose)), v3(std::get<2>(pose)), std::get<3>(pose), std::get<4>(pose), std::get<5>(pose));
            v = look_at_rh(v3(std::get<0>(pose)), v3(std::get<1>(pose)), v3(std::get<2>(pose)));
            p = perspective_wgpu(to_radians(std::get<3>(pose)), aspect, std::get<4>(pose), std::get<5>(pose));
            const Uniforms u = to_uniforms(globals, v, p);
            std::memcpy(blocks.data() + 44 * k, u.data(), 44 * sizeof(float));
        }
        if (n == 0) return files.empty() && paths.is_none() ? py::object(py::list()) : py::object(py::none());
        const size_t bytes = (size_t)H * W * 4;
        view = v; proj = p;                                     // the camera of the last pose stays, as after a loop of set_camera_look_at
        if (!files.empty()) {
            // PNG files: the poses go through in groups over a few pooled page-locked buffers -- every group one batch call, its frames
            // encoded before the next group is drawn -- so the page-locked footprint is kGroup frames whatever the number of poses
            // (advisor, round 5: n buffers up front were 4 GiB of unswappable memory and n registrations for 64 poses at 4096^2)
            constexpr size_t kGroup = 4;
            std::vector<py::capsule> owners;
            std::vector<uint8_t *> dst;
            for (size_t k = 0; k < std::min(n, kGroup); ++k) { void *q = PinnedPool::get().take(bytes); owners.push_back(pinned_owner(q, bytes)); dst.push_back(static_cast<uint8_t *>(q)); }
            {
                py::gil_scoped_release nogil;
                for (size_t k0 = 0; k0 < n; k0 += kGroup) {
                    const size_t m = std::min(kGroup, n - k0);
                    const int rc = vf_terrain_render_batch_host(t, blocks.data() + 44 * k0, (uint32_t)m, dst.data());
                    if (rc != VF_OK) { py::gil_scoped_acquire gil; raise_vf(rc); }
                    for (size_t k = 0; k < m; ++k) write_png_rgba8(files[k0 + k], dst[k], W, H);
                }
            }
            push_uniforms();
            return py::none();
        }
        // arrays: page-locked while the pool's allowance lasts (one DMA each, beside the next poses' kernels), ordinary memory beyond
        // (the runtime stages those copies: correct, slower)
        py::list frames;
        std::vector<uint8_t *> dst(n);
        for (size_t k = 0; k < n; ++k) {
            void *q = bytes >= ((size_t)4 << 20) ? PinnedPool::get().take_or_null(bytes, PinnedPool::kMaxOutBytes) : nullptr;
            if (q) {
                py::capsule owner = pinned_owner(q, bytes);
                frames.append(py::array_t<uint8_t>({ (py::ssize_t)H, (py::ssize_t)W, (py::ssize_t)4 }, static_cast<uint8_t *>(q), owner));
                dst[k] = static_cast<uint8_t *>(q);
            } else {
                py::array_t<uint8_t> a({ (py::ssize_t)H, (py::ssize_t)W, (py::ssize_t)4 });
                dst[k] = a.mutable_data();
                frames.append(a);
            }
        }
        {
            py::gil_scoped_release nogil;
            const int rc = vf_terrain_render_batch_host(t, blocks.data(), (uint32_t)n, dst.data());
            if (rc != VF_OK) { py::gil_scoped_acquire gil; raise_vf(rc); }
        }
        push_uniforms();
        return frames;
    }
    // extension: visible primitive id + 1 per pixel of the last render (0 = background)
    py::array_t<uint32_t> debug_visibility()
    {
        Borrow b(busy);
        uint32_t rows = 0;
        check(vf_terrain_local_rows(t, &rows));
        py::array_t<uint32_t> a({ (py::ssize_t)(ss > 1u ? SH : rows), (py::ssize_t)SW });   // (a supersampled object: the samples' ids)
        check(vf_terrain_read_visibility(t, a.mutable_data()));
        return a;
    }
    // extension: multi-GPU band ownership (DESIGN.md "Sharding")
    void set_shard(uint32_t rank, uint32_t nranks, uint32_t band_h) { Borrow b(busy); check(vf_terrain_set_shard(t, rank, nranks, band_h)); frame_current = false; }
    // extension: "reference" = fs_main as coded; "spec_t32" = the documented-only stage (forward-difference normals + Reinhard)
    void set_shade_mode(const std::string &mode)
    {
        Borrow b(busy);
        if (mode == "reference") check(vf_terrain_set_shade_mode(t, VF_SHADE_REFERENCE));
        else if (mode == "spec_t32") check(vf_terrain_set_shade_mode(t, VF_SHADE_SPEC_T32));
        else throw py::value_error("shade mode must be 'reference' or 'spec_t32'");
    }
    // extension: "fast" (default) = hardware rcp / rsq / sin / cos / log / exp in the fragment stage, within 1 LSB of "exact"
    // (IEEE binary32 in a fixed order, the CPU oracle bit for bit); visibility is identical
    void set_shade_precision(const std::string &precision)
    {
        Borrow b(busy);
        if (precision == "exact") check(vf_terrain_set_shade_precision(t, VF_PRECISION_EXACT));
        else if (precision == "fast") check(vf_terrain_set_shade_precision(t, VF_PRECISION_FAST));
        else throw py::value_error("shade precision must be 'exact' or 'fast'");
    }
    py::dict last_timings()
    {
        Borrow b(busy);
        vf_timings tm;
        check(vf_terrain_timings(t, &tm));
        py::dict d;
        d["ranges_ms"] = tm.ranges_ms; d["plan_ms"] = tm.plan_ms; d["tile_ms"] = tm.tile_ms; d["total_ms"] = tm.total_ms;
        d["blocks_rasterised"] = tm.blocks_rasterised; d["tiles"] = tm.tiles; d["frames"] = tm.frames; d["blocks_distinct"] = tm.blocks_distinct;
        return d;
    }
    void enable_timing(bool on) { Borrow b(busy); check(vf_terrain_enable_timing(t, on ? 1 : 0)); }

    // extension: overlays over the terrain frame (include/vf_hip.h; argument rules: vulkan_forge_amd/_overlays.py)
    uint32_t add_points(py::object xyz, py::object size_px, py::object rgba, py::object shape, bool drape, py::object occlude, py::object depth_bias,
                        py::object haze)
    {
        py::tuple a = rules("_overlays", "point_args")(xyz, size_px, rgba, shape);
        const LayerTail tail(occlude, depth_bias, haze);
        py::array pts = a[0].cast<py::array>(), dcol = a[3].cast<py::array>();
        const float dsize = a[1].cast<float>();
        py::object sizes = a[2], cols = a[4];
        const int shp = a[5].cast<int>();
        const float *sz = sizes.is_none() ? nullptr : static_cast<const float *>(sizes.cast<py::array>().data());
        const uint8_t *cl = cols.is_none() ? nullptr : static_cast<const uint8_t *>(cols.cast<py::array>().data());
        Borrow b(busy);
        tail.refuse_early(ss);
        uint32_t id = 0;
        check(vf_terrain_add_points(t, static_cast<const float *>(pts.data()), (uint32_t)pts.shape(0), sz, cl, dsize,
                                    static_cast<const uint8_t *>(dcol.data()), shp, drape ? 1 : 0, &id));
        tail.apply(t, id, true);
        return id;
    }
    uint32_t add_lines(py::object paths, py::object width_px, py::object rgba, py::object cap, bool drape, py::object occlude, py::object depth_bias,
                       py::object haze)
    {
        py::tuple a = rules("_overlays", "line_args")(paths, width_px, rgba, cap);
        const LayerTail tail(occlude, depth_bias, haze);
        py::array coords = a[0].cast<py::array>(), offsets = a[1].cast<py::array>(), col = a[3].cast<py::array>();
        const float width = a[2].cast<float>();
        const int cp = a[4].cast<int>();
        Borrow b(busy);
        tail.refuse_early(ss);
        uint32_t id = 0;
        check(vf_terrain_add_lines(t, static_cast<const float *>(coords.data()), static_cast<const uint32_t *>(offsets.data()),
                                   (uint32_t)(offsets.shape(0) - 1), width, static_cast<const uint8_t *>(col.data()), cp, drape ? 1 : 0, &id));
        tail.apply(t, id, true);
        return id;
    }
    uint32_t add_polygons(py::object polygons, py::object fill_rgba, py::object line_rgba, py::object line_width_px, bool drape)
    {
        py::tuple a = rules("_overlays", "polygon_args")(polygons, fill_rgba, line_rgba, line_width_px);
        py::array coords = a[0].cast<py::array>(), rings = a[1].cast<py::array>(), feats = a[2].cast<py::array>();
        py::object dfill = a[3], fills = a[4], line = a[5];
        const float width = a[6].cast<float>();
        auto bytes = [](py::object o) { return o.is_none() ? nullptr : static_cast<const uint8_t *>(o.cast<py::array>().data()); };
        Borrow b(busy);
        uint32_t id = 0;
        check(vf_terrain_add_polygons(t, static_cast<const float *>(coords.data()), static_cast<const uint32_t *>(rings.data()),
                                      (uint32_t)(rings.shape(0) - 1), static_cast<const uint32_t *>(feats.data()), (uint32_t)(feats.shape(0) - 1),
                                      bytes(fills), bytes(dfill), bytes(line), width, drape ? 1 : 0, &id));
        return id;
    }
    // occlusion of a point / line layer by the terrain
    void set_layer_occlusion(uint32_t layer, py::object occlude, py::object depth_bias)
    {
        py::tuple oc = rules("_overlays", "occlusion_args")(occlude, depth_bias);
        Borrow b(busy);
        check(vf_terrain_set_layer_occlusion(t, layer, oc[0].cast<bool>() ? 1 : 0, oc[1].cast<float>()));
    }
    // a point / line / contour layer under the atmospheric haze
    void set_layer_haze(uint32_t layer, py::object on)
    {
        const bool hz = rules("_overlays", "haze_arg")(on, "on").cast<bool>();
        Borrow b(busy);
        check(vf_terrain_set_layer_haze(t, layer, hz ? 1 : 0));
    }
    bool layer_haze(uint32_t layer)
    {
        Borrow b(busy);
        int on = 0;
        check(vf_terrain_layer_haze(t, layer, &on));
        return on != 0;
    }
    // contour lines of the rendered surface, extracted on the device
    py::tuple height_bounds()
    {
        Borrow b(busy);
        float lo = 0.0f, hi = 0.0f;
        check(vf_terrain_height_bounds(t, &lo, &hi));
        return py::make_tuple(lo, hi);
    }
    uint32_t layer_primitive_count(uint32_t layer)
    {
        return counter([layer](vf_terrain *h, uint32_t *count) { return vf_terrain_layer_primitive_count(h, layer, count); });
    }
    uint32_t add_contours(py::object levels, py::object interval, py::object base, py::object width_px, py::object rgba, py::object lift,
                          py::object join, py::object occlude, py::object depth_bias, py::object haze)
    {
        const LayerTail tail(occlude, depth_bias, haze);
        py::object bounds = py::none();
        if (levels.is_none() && !interval.is_none()) bounds = height_bounds();
        py::tuple a = rules("_overlays", "contour_args")(levels, interval, base, width_px, rgba, lift, join, bounds);
        py::array lv = a[0].cast<py::array>(), col = a[2].cast<py::array>();
        Borrow b(busy);
        uint32_t id = 0;
        // (the library's call takes the occlusion itself, and refuses it on a supersampled handle before it makes the layer)
        check(vf_terrain_add_contours(t, static_cast<const float *>(lv.data()), (uint32_t)lv.shape(0), a[1].cast<float>(),
                                      static_cast<const uint8_t *>(col.data()), a[3].cast<float>(), a[4].cast<int>(), tail.occlude ? 1 : 0,
                                      tail.depth_bias, &id, nullptr));
        tail.apply(t, id, false);
        return id;
    }
    void clear_overlays() { clear(vf_terrain_clear_overlays, false); }   // (overlays composite behind the stored frame: it stays current)

    // extension: supersampling
    uint32_t supersample() const { return ss; }
    uint32_t samples() const { return ss * ss; }
    py::tuple sample_size() const { return py::make_tuple(SW, SH); }
    // the samples of the current frame before the resolve: terrain and passes, no overlays, (f H, f W, 4) uint8
    py::array_t<uint8_t> render_samples() { return frame_plane<uint8_t>({ (py::ssize_t)SH, (py::ssize_t)SW, 4 }, vf_terrain_read_samples); }

    // extension: geometry buffers -- per-pixel depth, world position, normal and primitive id (argument rules:
    // vulkan_forge_amd/_gbuffer.py).  Like render_rgba they describe the frame for the current uniforms: it is drawn first unless the
    // frame this object drew last already is that frame.
    py::dict render_gbuffer(py::object planes)
    {
        py::tuple names = rules("_gbuffer", "plane_args")(planes);
        Borrow b(busy);
        py::dict out;
        float *f[3] = { nullptr, nullptr, nullptr };
        uint32_t *prim = nullptr;
        for (py::handle h : names) {
            const std::string k = h.cast<std::string>();
            // (the planes describe what was drawn: the samples of a supersampled object, sample_size)
            if (k == "primitive") { py::array_t<uint32_t> a({ (py::ssize_t)SH, (py::ssize_t)SW }); prim = a.mutable_data(); out[h] = a; continue; }
            const int slot = k == "depth" ? 0 : (k == "position" ? 1 : 2);
            py::array_t<float> a = slot == 0 ? py::array_t<float>({ (py::ssize_t)SH, (py::ssize_t)SW })
                                             : py::array_t<float>({ (py::ssize_t)SH, (py::ssize_t)SW, (py::ssize_t)3 });
            f[slot] = a.mutable_data(); out[h] = a;
        }
        {
            py::gil_scoped_release nogil;
            int rc = draw_current();
            if (rc == VF_OK) rc = vf_terrain_read_gbuffer(t, f[0], f[1], f[2], prim);
            if (rc != VF_OK) { py::gil_scoped_acquire gil; raise_vf(rc); }
        }
        return out;
    }
    py::array_t<float> render_depth()
    {
        return frame_plane<float>({ (py::ssize_t)SH, (py::ssize_t)SW },
                                  [](vf_terrain *h, float *depth) { return vf_terrain_read_gbuffer(h, depth, nullptr, nullptr, nullptr); });
    }
    py::dict pick(py::object pixels)
    {
        py::array px = rules("_gbuffer", "pixel_args")(pixels, W, H).cast<py::array>();
        const uint32_t count = (uint32_t)px.shape(0);
        Borrow b(busy);
        py::array_t<uint32_t> words({ (py::ssize_t)count, (py::ssize_t)8 });
        {
            const int32_t *src = static_cast<const int32_t *>(px.data());
            float *dst = reinterpret_cast<float *>(words.mutable_data());
            py::gil_scoped_release nogil;
            int rc = draw_current();
            if (rc == VF_OK) rc = vf_terrain_pick(t, src, count, dst);
            if (rc != VF_OK) { py::gil_scoped_acquire gil; raise_vf(rc); }
        }
        return rules("_gbuffer", "pick_result")(words).cast<py::dict>();
    }

    // extension: cast sun shadows (argument rules: vulkan_forge_amd/_shadows.py)
    void set_shadows(bool enabled, float strength, float softness, float bias)
    {
        py::tuple a = rules("_shadows", "shadow_args")(enabled, strength, softness, bias);
        Borrow b(busy);
        check(vf_terrain_set_shadows(t, a[0].cast<int>(), a[1].cast<float>(), a[2].cast<float>(), a[3].cast<float>()));
        frame_current = false;
    }
    py::array_t<float> shadow_field() { return vertex_field(vf_terrain_read_shadow_field); }
    uint32_t debug_shadow_scans() { return counter(vf_terrain_debug_shadow_scans); }
    // extension: ambient occlusion from a sky-view scan (argument rules: vulkan_forge_amd/_ambient.py)
    void set_ambient_occlusion(bool enabled, float strength, float reach, py::object directions)
    {
        py::tuple a = rules("_ambient", "ambient_args")(enabled, strength, reach, directions);
        py::array dirs = a[4].cast<py::array>();             // (D, 2) float32, contiguous
        Borrow b(busy);
        check(vf_terrain_set_ambient(t, a[0].cast<int>(), a[1].cast<float>(), a[2].cast<float>(), a[3].cast<uint32_t>(), static_cast<const float *>(dirs.data())));
        frame_current = false;
    }
    py::array_t<float> sky_view_field() { return vertex_field(vf_terrain_read_sky_view_field); }
    uint32_t debug_ambient_scans() { return counter(vf_terrain_debug_ambient_scans); }
    // extension: a draped image layer (argument rules: vulkan_forge_amd/_drape.py)
    void set_drape(py::object image, py::object extent, py::object opacity, py::object filter)
    {
        py::tuple a = rules("_drape", "drape_args")(image, extent, opacity, filter);
        py::array img = a[0].cast<py::array>();              // (ih, iw, channels) uint8, contiguous
        py::array ext = a[4].cast<py::array>();              // (4,) float32
        const uint32_t iw = a[1].cast<uint32_t>(), ih = a[2].cast<uint32_t>(), channels = a[3].cast<uint32_t>();
        const float op = a[5].cast<float>();
        const int code = a[6].cast<int>();
        Borrow b(busy);
        const uint8_t *src = static_cast<const uint8_t *>(img.data());
        const float *e = static_cast<const float *>(ext.data());
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = vf_terrain_set_drape(t, src, iw, ih, channels, e, op, code);
        }
        check(rc);
        frame_current = false;
    }
    void clear_drape() { clear(vf_terrain_clear_drape); }
    py::object drape_info()
    {
        Borrow b(busy);
        uint32_t iw = 0, ih = 0;
        float ext[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, op = 0.0f;
        int code = 0;
        check(vf_terrain_drape_info(t, &iw, &ih, ext, &op, &code));
        return rules("_drape", "drape_info")(iw, ih, tuple4(ext), op, code);
    }
    // extension: a mip pyramid under the draped image (argument rules: vulkan_forge_amd/_drape.py)
    void set_drape_mipmaps(py::object enabled, py::object bias)
    {
        py::tuple a = rules("_drape", "mip_params")(enabled, bias);
        Borrow b(busy);
        check(vf_terrain_set_drape_mips(t, a[0].cast<int>(), a[1].cast<float>()));
        frame_current = false;
    }
    py::object drape_mip_info()
    {
        Borrow b(busy);
        int enabled = 0;
        uint32_t levels = 0, builds = 0, iw = 0, ih = 0;
        float bias = 0.0f;
        uint64_t bytes = 0;
        check(vf_terrain_drape_mip_info(t, &enabled, &levels, &bias, &bytes, &builds));
        check(vf_terrain_drape_info(t, &iw, &ih, nullptr, nullptr, nullptr));
        return rules("_drape", "mip_info")(enabled != 0, levels, bias, bytes, builds, iw, ih);
    }
    py::array read_drape_level(py::object level)
    {
        Borrow b(busy);
        uint32_t levels = 0, w = 0, h = 0;
        check(vf_terrain_drape_mip_info(t, nullptr, &levels, nullptr, nullptr, nullptr));
        const uint32_t k = rules("_drape", "mip_level")(level, levels).cast<uint32_t>();   // (needs the handle's level count: inside the borrow)
        check(vf_terrain_read_drape_level(t, k, nullptr, &w, &h));
        py::array out(py::dtype("float16"), std::vector<py::ssize_t>{ (py::ssize_t)h, (py::ssize_t)w, 4 });
        uint16_t *dst = static_cast<uint16_t *>(out.mutable_data());
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = vf_terrain_read_drape_level(t, k, dst, nullptr, nullptr);
        }
        check(rc);
        return out;
    }
    // extension: anisotropic filtering of the mip sampling (argument rules: vulkan_forge_amd/_drape.py)
    void set_drape_anisotropy(py::object max_anisotropy)
    {
        const uint32_t a = rules("_drape", "aniso_params")(max_anisotropy).cast<uint32_t>();
        Borrow b(busy);
        check(vf_terrain_set_drape_anisotropy(t, a));
        frame_current = false;
    }
    uint32_t drape_anisotropy() { return counter(vf_terrain_drape_anisotropy); }
    // extension: viewshed analysis (argument rules: vulkan_forge_amd/_viewshed.py)
    void set_viewshed(py::object observer, py::object enabled, py::object eye_height, py::object target_height, py::object radius,
                      py::object visible_rgba, py::object hidden_rgba, py::object softness, py::object bias)
    {
        py::tuple a = rules("_viewshed", "viewshed_args")(observer, enabled, eye_height, target_height, radius, visible_rgba, hidden_rgba, softness, bias);
        const float xz[2] = { a[1].cast<float>(), a[2].cast<float>() };
        uint8_t vis[4], hid[4];
        rgba4(a[6], vis); rgba4(a[7], hid);
        Borrow b(busy);
        check(vf_terrain_set_viewshed(t, a[0].cast<int>(), xz, a[3].cast<float>(), a[4].cast<float>(), a[5].cast<float>(), vis, hid,
                                      a[8].cast<float>(), a[9].cast<float>()));
        frame_current = false;
    }
    void clear_viewshed()
    {
        Borrow b(busy);
        check(vf_terrain_set_viewshed(t, 0, nullptr, 0.0f, 0.0f, 0.0f, nullptr, nullptr, 1.0f, 0.0f));
        frame_current = false;
    }
    py::array_t<float> viewshed_field() { return vertex_field(vf_terrain_read_viewshed_field); }
    py::object viewshed_info()
    {
        Borrow b(busy);
        vf_viewshed_info v;
        check(vf_terrain_viewshed_info(t, &v));
        return rules("_viewshed", "viewshed_info")(
            v.enabled, v.has_observer, py::make_tuple(v.vertex[0], v.vertex[1]), py::make_tuple(v.observer_xyz[0], v.observer_xyz[1], v.observer_xyz[2]),
            v.eye_y, v.eye_height, v.target_height, v.radius, v.softness, v.bias, tuple4(v.visible_rgba), tuple4(v.hidden_rgba));
    }
    uint32_t debug_viewshed_scans() { return counter(vf_terrain_debug_viewshed_scans); }
    // extension: cumulative viewsheds (argument rules: vulkan_forge_amd/_cumulative_viewshed.py)
    void set_cumulative_viewshed(py::object observers, py::object enabled, py::object eye_height, py::object target_height, py::object radius,
                                 py::object high_rgba, py::object low_rgba, py::object softness, py::object bias)
    {
        py::tuple a = rules("_cumulative_viewshed", "cumulative_viewshed_args")(observers, enabled, eye_height, target_height, radius, high_rgba, low_rgba,
                                                                                softness, bias);
        auto obs = a[1].cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
        uint8_t high[4], low[4];
        rgba4(a[5], high); rgba4(a[6], low);
        Borrow b(busy);
        check(vf_terrain_set_cumulative_viewshed(t, a[0].cast<int>(), obs.data(), (uint32_t)obs.shape(0), a[2].cast<float>(), a[3].cast<float>(),
                                                 a[4].cast<float>(), high, low, a[7].cast<float>(), a[8].cast<float>()));
        frame_current = false;
    }
    void clear_cumulative_viewshed()
    {
        Borrow b(busy);
        check(vf_terrain_set_cumulative_viewshed(t, 0, nullptr, 0, 0.0f, 0.0f, 0.0f, nullptr, nullptr, 1.0f, 0.0f));
        frame_current = false;
    }
    py::array_t<float> cumulative_viewshed_field() { return vertex_field(vf_terrain_read_cumulative_viewshed_field); }
    py::object cumulative_viewshed_info()
    {
        Borrow b(busy);
        vf_cumulative_viewshed_info v;
        check(vf_terrain_cumulative_viewshed_info(t, &v));
        return rules("_cumulative_viewshed", "cumulative_viewshed_info")(
            v.enabled, v.count, v.batch, listed_vertices(v.count, vf_terrain_read_cumulative_viewshed_vertices), v.eye_height, v.target_height, v.radius,
            v.softness, v.bias, tuple4(v.high_rgba), tuple4(v.low_rgba));
    }
    void debug_cumulative_viewshed_batch(uint32_t batch) { Borrow b(busy); check(vf_terrain_debug_cumulative_viewshed_batch(t, batch)); }
    uint32_t debug_cumulative_viewshed_scans() { return counter(vf_terrain_debug_cumulative_viewshed_scans); }
    // extension: sun exposure (argument rules: vulkan_forge_amd/_sun_exposure.py)
    void set_sun_exposure(py::object suns, py::object weights, py::object incidence, py::object enabled, py::object softness, py::object bias,
                          py::object high_rgba, py::object low_rgba)
    {
        py::tuple a = rules("_sun_exposure", "sun_exposure_args")(suns, weights, incidence, enabled, softness, bias, high_rgba, low_rgba);
        auto given = a[1].cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
        auto w = a[2].cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
        const size_t count = (size_t)given.shape(0);
        std::vector<float> xyz(3u * count);
        const float *g = given.data();
        if (given.shape(1) == 2) {                              // angles: the vectors set_sun would store
            for (size_t o = 0; o < count; ++o) {
                const Vec3 v = sun_from_angles(g[2u * o], g[2u * o + 1u]);
                xyz[3u * o] = v.x; xyz[3u * o + 1u] = v.y; xyz[3u * o + 2u] = v.z;
            }
        }
        else std::copy(g, g + 3u * count, xyz.begin());
        uint8_t high[4], low[4];
        rgba4(a[6], high); rgba4(a[7], low);
        Borrow b(busy);
        check(vf_terrain_set_sun_exposure(t, a[0].cast<int>(), xyz.data(), w.data(), (uint32_t)count, a[3].cast<int>(), a[4].cast<float>(),
                                          a[5].cast<float>(), high, low));
        frame_current = false;
    }
    void clear_sun_exposure() { clear(vf_terrain_clear_sun_exposure); }
    py::array_t<float> sun_exposure_field() { return vertex_field(vf_terrain_read_sun_exposure_field); }
    py::object sun_exposure_info()
    {
        Borrow b(busy);
        vf_sun_exposure_info v;
        check(vf_terrain_sun_exposure_info(t, &v));
        return rules("_sun_exposure", "sun_exposure_info")(v.enabled, v.count, v.counted, v.weight_total, v.incidence, v.batch, v.softness, v.bias,
                                                           tuple4(v.high_rgba), tuple4(v.low_rgba));
    }
    void debug_sun_exposure_batch(uint32_t batch) { Borrow b(busy); check(vf_terrain_debug_sun_exposure_batch(t, batch)); }
    uint32_t debug_sun_exposure_scans() { return counter(vf_terrain_debug_sun_exposure_scans); }
    // extension: atmospheric haze (argument rules: vulkan_forge_amd/_haze.py)
    void set_haze(py::object density, py::object rgba, py::object start, py::object falloff, py::object base, py::object max_opacity,
                  py::object background, py::object enabled)
    {
        py::tuple a = rules("_haze", "haze_args")(density, rgba, start, falloff, base, max_opacity, background, enabled);
        uint8_t col[4];
        rgba4(a[2], col);
        Borrow b(busy);
        check(vf_terrain_set_haze(t, a[0].cast<int>(), a[1].cast<float>(), col, a[3].cast<float>(), a[4].cast<float>(), a[5].cast<float>(),
                                  a[6].cast<float>(), a[7].cast<int>()));
        frame_current = false;
    }
    void clear_haze() { clear(vf_terrain_clear_haze); }
    py::object haze_info()
    {
        Borrow b(busy);
        vf_haze_info v;
        check(vf_terrain_haze_info(t, &v));
        return rules("_haze", "haze_info")(v.enabled, v.background, v.density, v.start, v.falloff, v.base, v.max_opacity, tuple4(v.rgba), v.has_eye, v.eye_y);
    }
    // like render_depth it describes the frame for the current uniforms: drawn first unless the frame drawn last already is that frame
    py::array_t<float> haze_opacity() { return frame_plane<float>({ (py::ssize_t)SH, (py::ssize_t)SW }, vf_terrain_read_haze_opacity); }
    // what flood_args / spill_args return about the sources, as the C calls take it: a[i] the seeds ((N, 2) float32 or None), a[i + 1]
    // and a[i + 2] the shallow and the deep colour
    struct FillArgs {
        py::array_t<float, py::array::c_style | py::array::forcecast> arr;     // (holds what xz points to)
        const float *xz = nullptr;
        uint32_t count = 0;
        uint8_t sh[4], dp[4];
        FillArgs(const py::tuple &a, size_t i)
        {
            if (!a[i].is_none()) {
                arr = a[i].cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
                xz = arr.data(); count = (uint32_t)arr.shape(0);
            }
            rgba4(a[i + 1], sh); rgba4(a[i + 2], dp);
        }
    };
    // the vertices of `count` listed points -- the seeds of a fill, the observers of the cumulative viewshed -- as (count, 2) uint32, or
    // None: nothing listed, or no uniforms set yet (`read` refuses).  The caller holds the borrow.
    py::object listed_vertices(uint32_t count, int (*read)(vf_terrain *, uint32_t *))
    {
        if (!count) return py::none();
        py::array_t<uint32_t> a({ (py::ssize_t)count, (py::ssize_t)2 });
        if (read(t, a.mutable_data()) != VF_OK) return py::none();
        return a;
    }
    // extension: flood analysis (argument rules: vulkan_forge_amd/_flood.py)
    void set_flood(py::object level, py::object seeds, py::object enabled, py::object shallow_rgba, py::object deep_rgba, py::object depth_full)
    {
        py::tuple a = rules("_flood", "flood_args")(level, seeds, enabled, shallow_rgba, deep_rgba, depth_full);
        const FillArgs f(a, 3);
        Borrow b(busy);
        check(vf_terrain_set_flood(t, a[0].cast<int>(), a[1].cast<float>(), a[2].cast<int>(), f.xz, f.count, f.sh, f.dp, a[6].cast<float>()));
        frame_current = false;
    }
    void clear_flood() { clear(vf_terrain_clear_flood); }
    py::array_t<float> flood_field() { return vertex_field(vf_terrain_read_flood_field); }
    py::object flood_info()
    {
        Borrow b(busy);
        vf_flood_info v;
        check(vf_terrain_flood_info(t, &v));
        return rules("_flood", "flood_info")(
            v.enabled, v.has_flood, v.mode, v.count, listed_vertices(v.count, vf_terrain_read_flood_seeds), v.level, v.depth_full,
            tuple4(v.shallow_rgba), tuple4(v.deep_rgba), v.flooded_vertices, v.wettable_vertices, v.passes, v.scans, v.group);
    }
    void debug_flood_group(uint32_t group) { Borrow b(busy); check(vf_terrain_debug_flood_group(t, group)); }
    uint32_t debug_flood_scans() { return counter(vf_terrain_debug_flood_scans); }
    // extension: spill analysis (argument rules: vulkan_forge_amd/_spill.py)
    void set_spill(py::object seeds, py::object enabled, py::object shallow_rgba, py::object deep_rgba, py::object depth_full)
    {
        py::tuple a = rules("_spill", "spill_args")(seeds, enabled, shallow_rgba, deep_rgba, depth_full);
        const FillArgs f(a, 2);
        Borrow b(busy);
        check(vf_terrain_set_spill(t, a[0].cast<int>(), a[1].cast<int>(), f.xz, f.count, f.sh, f.dp, a[5].cast<float>()));
        frame_current = false;
    }
    void clear_spill() { clear(vf_terrain_clear_spill); }
    py::array_t<float> spill_field() { return vertex_field(vf_terrain_read_spill_field); }
    py::array_t<float> sink_depth_field() { return vertex_field(vf_terrain_read_sink_depth); }
    py::object spill_info()
    {
        Borrow b(busy);
        vf_spill_info v;
        check(vf_terrain_spill_info(t, &v));
        return rules("_spill", "spill_info")(
            v.enabled, v.has_spill, v.mode, v.count, listed_vertices(v.count, vf_terrain_read_spill_seeds), v.depth_full,
            tuple4(v.shallow_rgba), tuple4(v.deep_rgba), v.reached_vertices, v.sink_vertices, v.passes, v.scans, v.group, v.tile_runs);
    }
    void debug_spill_group(uint32_t group) { Borrow b(busy); check(vf_terrain_debug_spill_group(t, group)); }
    uint32_t debug_spill_scans() { return counter(vf_terrain_debug_spill_scans); }
    // extension: Renderer's sun and exposure setters (src/lib.rs:441-473) on the terrain objects; neither changes a default
    void set_sun(float elevation_deg, float azimuth_deg)
    {
        if (!std::isfinite(elevation_deg) || !std::isfinite(azimuth_deg)) throw py::value_error("angles must be finite");
        Borrow b(busy);
        globals.sun_dir = sun_from_angles(elevation_deg, azimuth_deg);
        push_uniforms();
    }
    void set_exposure(float exposure)
    {
        if (!std::isfinite(exposure) || exposure <= 0.0f) throw py::value_error("exposure must be > 0");
        Borrow b(busy);
        globals.exposure = exposure;
        push_uniforms();
    }

    // src/terrain/mod.rs:537-546
    py::array_t<float> debug_uniforms_f32() const
    {
        if (busy.load(std::memory_order_acquire)) throw std::runtime_error("Already mutably borrowed");   // a `&self` method, PyO3-style
        py::array_t<float> a(44);
        std::memcpy(a.mutable_data(), last.data(), 44 * sizeof(float));
        return a;
    }
    std::string debug_lut_format() const { return lut_format; }   // src/terrain/mod.rs:493-496

private:
    // ---- the call shapes the methods above share; each keeps, in one place, what a copy could get wrong ----
    // A per-vertex field as (n, n) float32.  The GIL is released around `read` alone: it computes a stale field on the device and touches no
    // Python object.  It is held again before a refusal is raised, and the borrow goes back on either way out.
    py::array_t<float> vertex_field(int (*read)(vf_terrain *, float *))
    {
        Borrow b(busy);
        py::array_t<float> a({ (py::ssize_t)n, (py::ssize_t)n });
        float *dst = a.mutable_data();
        py::gil_scoped_release nogil;
        const int rc = read(t, dst);
        if (rc != VF_OK) { py::gil_scoped_acquire gil; raise_vf(rc); }
        return a;
    }
    // A plane of the frame for the current uniforms, heights and settings: the same, with the frame drawn first unless the frame drawn last
    // already is that frame (draw_current).  Only render_samples, render_depth, haze_opacity, render_gbuffer and pick draw before they read.
    template <class T, class Read>
    py::array_t<T> frame_plane(std::vector<py::ssize_t> shape, Read read)
    {
        Borrow b(busy);
        py::array_t<T> a(std::move(shape));
        T *dst = a.mutable_data();
        py::gil_scoped_release nogil;
        int rc = draw_current();
        if (rc == VF_OK) rc = read(t, dst);
        if (rc != VF_OK) { py::gil_scoped_acquire gil; raise_vf(rc); }
        return a;
    }
    // One uint32 the handle keeps on the host -- a scan counter, a layer's primitive count, a setting: no device work, the GIL stays held.
    template <class Get>
    uint32_t counter(Get get)
    {
        Borrow b(busy);
        uint32_t v = 0;
        check(get(t, &v));
        return v;
    }
    // A vf_terrain_clear_* call.  What it drops was part of the frame, so the frame is stale -- except for overlays (redraw = false),
    // which are composited behind the stored frame.  clear_viewshed and clear_cumulative_viewshed are not here: the library clears those
    // through their set call, and so do they.
    void clear(int (*fn)(vf_terrain *), bool redraw = true)
    {
        Borrow b(busy);
        check(fn(t));
        if (redraw) frame_current = false;
    }
    // What add_points, add_lines and add_contours take behind their own arguments: occlude, depth_bias, haze.  The rules read them in the
    // constructor, before the object is borrowed.  add_points / add_lines make the layer first and set its occlusion afterwards: on a
    // supersampled object the library would refuse the second step with the layer already there, so refuse_early raises the library's
    // refusal, in its words, before the first is taken.  apply: the caller holds the borrow and the layer exists.
    struct LayerTail {
        bool occlude = false, haze = false;
        float depth_bias = 0.0f;
        LayerTail(const py::object &occlude_, const py::object &depth_bias_, const py::object &haze_)
        {
            haze = rules("_overlays", "haze_arg")(haze_).cast<bool>();
            py::tuple oc = rules("_overlays", "occlusion_args")(occlude_, depth_bias_);
            occlude = oc[0].cast<bool>(); depth_bias = oc[1].cast<float>();
        }
        void refuse_early(uint32_t supersampling) const
        {
            if (occlude && supersampling > 1u) throw std::runtime_error("the handle is supersampled: occluding overlay layers are not supported (their depth test reads the frame's visibility per output pixel)");
        }
        void apply(vf_terrain *h, uint32_t layer, bool occlusion_too) const
        {
            if (occlusion_too && occlude) check(vf_terrain_set_layer_occlusion(h, layer, 1, depth_bias));
            if (haze) check(vf_terrain_set_layer_haze(h, layer, 1));
        }
    };
    void push_uniforms()
    {
        last = to_uniforms(globals, view, proj);
        check(vf_terrain_set_uniforms(t, last.data()));
        frame_current = false;
    }
    int draw_current()                                      // caller holds the borrow
    {
        if (frame_current) return VF_OK;
        const int rc = vf_terrain_render(t, nullptr);
        frame_current = rc == VF_OK;
        return rc;
    }
    bool frame_current = false;                             // the frame vf_terrain_render drew last was drawn from the current uniforms and heights
    uint32_t W, H, n = 128;
    uint32_t ss = 1, SW = 0, SH = 0;                        // supersampling factor and the sample size (ss W, ss H)
    vf_terrain *t = nullptr;
    Globals globals;
    Mat4 view{}, proj{};
    Uniforms last{};
    std::string lut_format;
    mutable std::atomic<bool> busy{false};
};

class TerrainSpike : public TerrainObject {
public:
    TerrainSpike(uint32_t w, uint32_t h, py::object grid, py::object colormap, py::object supersample) : TerrainObject(0, w, h, grid, colormap, supersample) {}
};
class Scene : public TerrainObject {
public:
    Scene(uint32_t w, uint32_t h, py::object grid, py::object colormap, py::object supersample) : TerrainObject(1, w, h, grid, colormap, supersample) {}
};

// ---- Renderer: the triangle smoke path (src/lib.rs:245-334, 685-721) + the DEM path (:336-682) ---------------------
class Renderer {
public:
    Renderer(uint32_t w, uint32_t h) : W(w), H(h) { global_ctx(); }
    ~Renderer() { if (dem) vf_dem_destroy(dem); }
    Renderer(const Renderer &) = delete;
    Renderer &operator=(const Renderer &) = delete;
    std::string info() const { return "Renderer " + std::to_string(W) + "x" + std::to_string(H) + ", format=Rgba8UnormSrgb"; }
    py::array_t<uint8_t> render_triangle_rgba()
    {
        py::array_t<uint8_t> a({ (py::ssize_t)H, (py::ssize_t)W, (py::ssize_t)4 });
        check(vf_triangle_render(global_ctx(), W, H, a.mutable_data()));
        return a;
    }
    void render_triangle_png(const std::string &path)
    {
        std::vector<uint8_t> px((size_t)W * H * 4);
        check(vf_triangle_render(global_ctx(), W, H, px.data()));
        write_png_rgba8(path, px.data(), W, H);
    }

    // add_terrain, src/lib.rs:336-421
    void add_terrain(py::object heightmap, std::tuple<float, float> spacing, float exaggeration, const std::string &colormap)
    {
        if (std::get<0>(spacing) <= 0.0f || std::get<1>(spacing) <= 0.0f) throw std::runtime_error("spacing components must be > 0");
        if (exaggeration <= 0.0f) throw std::runtime_error("exaggeration must be > 0");
        const char *kind = "heightmap must be a 2-D NumPy array of dtype float32 or float64";
        if (!py::isinstance<py::array>(heightmap)) throw std::runtime_error(kind);
        py::array arr = py::reinterpret_borrow<py::array>(heightmap);
        const bool f32 = arr.dtype().is(py::dtype::of<float>()), f64 = arr.dtype().is(py::dtype::of<double>());
        if (arr.ndim() != 2 || !(f32 || f64)) throw std::runtime_error(kind);
        // a non-contiguous float32 array fails the reference's f32 attempt and then its f64 downcast: the dtype message
        // (src/lib.rs:351-372); only a non-contiguous float64 array reports the layout (:374-376)
        if (!(arr.flags() & py::array::c_style)) throw std::runtime_error(f32 ? kind : "heightmap must be C-contiguous (row-major)");
        const uint32_t h = (uint32_t)arr.shape(0), w = (uint32_t)arr.shape(1);
        if (w == 0 || h == 0) throw std::runtime_error("heightmap cannot be empty");
        // staged: the uploaded terrain replaces the current one only when the whole call succeeds (src/lib.rs:409-416 assigns
        // self.terrain last); the height range alone is stored before the colormap check, as in the reference (:394)
        struct Staged {
            vf_dem *d = nullptr;
            ~Staged() { if (d) vf_dem_destroy(d); }
        } fresh;
        check(vf_dem_create(global_ctx(), &fresh.d));
        if (f32) check(vf_dem_set_heights_f32(fresh.d, static_cast<const float *>(arr.data()), w, h, exaggeration));
        else check(vf_dem_set_heights_f64(fresh.d, static_cast<const double *>(arr.data()), w, h, exaggeration));
        // TerrainMeta::compute_and_store_h_range (src/renderer.rs:26-30): 1-99 percentile clamp
        float p1 = 0, p99 = 1;
        check(vf_dem_percentile_range(fresh.d, &p1, &p99));
        h_min = p1; h_max = std::fmax(p99, p1 + 1e-5f);
        bool known = false;
        for (const char *s : kSupported) known |= colormap == s;
        if (!known) throw std::runtime_error(unknown_colormap(colormap));    // after the range, like the reference (:398-407)
        std::swap(dem, fresh.d);                                             // (the previous terrain, if any, is released by `fresh`)
        has_terrain = true;
        terrain_colormap = colormap;
    }
    void need_terrain() const { if (!has_terrain) throw std::runtime_error("no terrain uploaded; call add_terrain() first"); }
    std::tuple<float, float, float, float> terrain_stats()                  // src/lib.rs:423-429
    {
        need_terrain();
        float st[4];
        check(vf_dem_stats(dem, st));
        return { st[0], st[1], st[2], st[3] };
    }
    void set_height_range(float mn, float mx)                               // src/renderer.rs:32-42
    {
        if (!std::isfinite(mn) || !std::isfinite(mx)) throw py::value_error("min/max must be finite floats");
        if (mn >= mx) throw py::value_error("min must be < max");
        h_min = mn; h_max = mx;
    }
    void set_sun(float elevation_deg, float azimuth_deg)                    // src/lib.rs:441-462
    {
        if (!std::isfinite(elevation_deg) || !std::isfinite(azimuth_deg)) throw py::value_error("angles must be finite");
        globals.sun_dir = sun_from_angles(elevation_deg, azimuth_deg);
    }
    void set_exposure(float exposure)                                       // src/lib.rs:464-473
    {
        if (!std::isfinite(exposure) || exposure <= 0.0f) throw py::value_error("exposure must be > 0");
        globals.exposure = exposure;
    }
    void normalize_terrain(const std::string &mode, py::object range, py::object eps)   // src/lib.rs:476-493
    {
        need_terrain();
        std::string m = mode;
        for (auto &c : m) c = (char)std::tolower((unsigned char)c);
        int code = m == "minmax" ? 0 : (m == "zscore" ? 1 : -1);
        if (code < 0) throw std::runtime_error("mode must be 'minmax' or 'zscore'");
        float e = eps.is_none() ? 1e-8f : eps.cast<float>();
        std::tuple<float, float> r = range.is_none() ? std::make_tuple(0.0f, 1.0f) : range.cast<std::tuple<float, float>>();
        check(vf_dem_normalize(dem, code, std::get<0>(r), std::get<1>(r), e));
    }
    void upload_height_r32f() { need_terrain(); check(vf_dem_upload_height(dem)); }     // src/lib.rs:495-571
    py::array_t<float> debug_read_height_patch(uint32_t x, uint32_t y, uint32_t w, uint32_t h)   // :573-666
    {
        if (w == 0 || h == 0) throw std::runtime_error("patch dimensions must be > 0");
        py::array_t<float> out({ (py::ssize_t)h, (py::ssize_t)w });
        uint32_t tw = 0, th = 0;
        if (dem) check(vf_dem_texture_size(dem, &tw, &th));
        if (tw == 0) { std::memset(out.mutable_data(), 0, (size_t)w * h * sizeof(float)); return out; }   // no texture yet: zeros (:580-588)
        check(vf_dem_read_patch(dem, x, y, w, h, out.mutable_data()));
        return out;
    }
    py::array_t<float> read_full_height_texture()                          // src/lib.rs:668-681
    {
        need_terrain();
        uint32_t tw = 0, th = 0;
        check(vf_dem_texture_size(dem, &tw, &th));
        if (tw == 0) throw std::runtime_error("no height texture uploaded; call upload_height_r32f() first");
        return debug_read_height_patch(0, 0, tw, th);
    }
private:
    uint32_t W, H;
    vf_dem *dem = nullptr;
    bool has_terrain = false;
    float h_min = 0.0f, h_max = 1.0f;          // TerrainMeta (src/renderer.rs:7-22)
    Globals globals;
    std::string terrain_colormap;
};

// ---- module functions ------------------------------------------------------------------------------
// grid_generate, src/terrain/mesh.rs:149-203 (validation strings :161-173 raised as ValueError)
py::tuple grid_generate(uint32_t nx, uint32_t nz, std::tuple<float, float> spacing, py::object origin)
{
    if (nx < 2 || nz < 2) throw py::value_error("nx and nz must be >= 2");
    float dx = std::get<0>(spacing), dy = std::get<1>(spacing);
    if (!std::isfinite(dx) || !std::isfinite(dy) || dx <= 0.0f || dy <= 0.0f) throw py::value_error("spacing components must be finite and > 0");
    std::string o = origin.is_none() ? "center" : origin.cast<std::string>();
    if (o != "center") throw py::value_error("origin must be 'center'");
    py::ssize_t nv = (py::ssize_t)nx * nz, ni = 6 * (py::ssize_t)(nx - 1) * (nz - 1);
    py::array_t<float> xy({ nv, (py::ssize_t)2 }), uv({ nv, (py::ssize_t)2 });
    py::array_t<uint32_t> idx(ni);
    check(vf_grid_generate(global_ctx(), nx, nz, dx, dy, xy.mutable_data(), uv.mutable_data(), idx.mutable_data()));
    return py::make_tuple(xy, uv, idx);
}

std::vector<std::string> colormap_supported() { return { "viridis", "magma", "terrain" }; }   // src/colormap/mod.rs:44-47
// extension: the 256 x 1 RGBA8 texels the registry resolves a name to (src/colormap/mod.rs:50-56), for callers that drive the
// C-ABI themselves (vf_terrain_create takes the bytes)
py::array_t<uint8_t> colormap_rgba8(const std::string &name)
{
    const uint8_t *lut = resolve_lut(name);
    py::array_t<uint8_t> a({ (py::ssize_t)256, (py::ssize_t)4 });
    std::memcpy(a.mutable_data(), lut, 1024);
    return a;
}

py::array_t<float> camera_look_at(std::tuple<float, float, float> eye, std::tuple<float, float, float> target,
                                  std::tuple<float, float, float> up)
{
    validate_vectors(v3(eye), v3(target), v3(up));
    return mat4_to_numpy(look_at_rh(v3(eye), v3(target), v3(up)));
}
py::array_t<float> camera_perspective(float fovy_deg, float aspect, float znear, float zfar, py::object clip_space)
{
    std::string clip = clip_space.is_none() ? "wgpu" : clip_space.cast<std::string>();
    validate_fovy(fovy_deg); validate_aspect(aspect); validate_near(znear); validate_far(zfar, znear);
    bool gl = clip_is_gl(clip);
    Mat4 p = gl ? perspective_rh_gl(to_radians(fovy_deg), aspect, znear, zfar) : perspective_wgpu(to_radians(fovy_deg), aspect, znear, zfar);
    return mat4_to_numpy(p);
}
py::array_t<float> camera_view_proj(std::tuple<float, float, float> eye, std::tuple<float, float, float> target,
                                    std::tuple<float, float, float> up, float fovy_deg, float aspect, float znear, float zfar,
                                    py::object clip_space)
{
    std::string clip = clip_space.is_none() ? "wgpu" : clip_space.cast<std::string>();
    validate_vectors(v3(eye), v3(target), v3(up));
    validate_fovy(fovy_deg); validate_aspect(aspect); validate_near(znear); validate_far(zfar, znear);
    bool gl = clip_is_gl(clip);
    Mat4 v = look_at_rh(v3(eye), v3(target), v3(up));
    Mat4 p = gl ? perspective_rh_gl(to_radians(fovy_deg), aspect, znear, zfar) : perspective_wgpu(to_radians(fovy_deg), aspect, znear, zfar);
    return mat4_to_numpy(mat_mul(p, v));
}

// enumerate_adapters / device_probe (src/lib.rs:744-845) reported from hipGetDeviceProperties
py::dict adapter_dict(const vf_device_info &di)
{
    py::dict d;
    d["name"] = std::string(di.name);
    d["backend"] = "HIP";
    d["device_type"] = "DiscreteGpu";
    d["vendor_id"] = 0x1002u;
    d["device_id"] = (uint32_t)di.pci_device_id;
    d["features"] = std::string("arch=") + di.arch + " wavefront=" + std::to_string(di.wavefront_size);
    d["limits"] = "compute_units=" + std::to_string(di.compute_units) + " total_mem_bytes=" + std::to_string(di.total_mem_bytes) +
                  " lds_bytes_per_cu=" + std::to_string(di.lds_bytes_per_cu);
    return d;
}
py::list enumerate_adapters()
{
    py::list out;
    int n = 0;
    if (vf_device_count(&n) != VF_OK) return out;
    for (int i = 0; i < n; ++i) {
        vf_device_info di;
        if (vf_device_query(i, &di) == VF_OK) out.append(adapter_dict(di));
    }
    return out;
}
py::dict device_probe(py::object backend)
{
    std::string b = backend.is_none() ? "AUTO" : backend.cast<std::string>();
    for (auto &ch : b) ch = (char)std::toupper((unsigned char)ch);
    py::dict d;
    d["backend_request"] = b;
    auto t0 = std::chrono::steady_clock::now();
    auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    if (b != "AUTO" && b != "HIP") {   // only one backend exists in this build
        d["status"] = "unsupported"; d["message"] = "No suitable GPU adapter"; d["millis"] = ms();
        return d;
    }
    vf_device_info di;
    int rc = vf_device_query(device_ordinal(), &di);
    if (rc != VF_OK) {
        d["status"] = "unsupported"; d["message"] = "No suitable GPU adapter"; d["millis"] = ms();
        return d;
    }
    py::dict a = adapter_dict(di);
    d["adapter_name"] = a["name"];
    for (const char *k : { "backend", "device_type", "vendor_id", "device_id", "features", "limits" }) d[k] = a[k];
    vf_ctx *c = nullptr;
    rc = vf_ctx_create(device_ordinal(), &c);
    if (rc != VF_OK) {
        d["status"] = "error"; d["message"] = std::string("request_device failed: ") + vf_last_error(); d["millis"] = ms();
        return d;
    }
    vf_ctx_destroy(c);
    d["status"] = "ok"; d["millis"] = ms();
    return d;
}

// testing hook: the PNG encoder behind render_png / render_triangle_png, without touching the GPU
py::bytes py_encode_png(py::array_t<uint8_t, py::array::c_style | py::array::forcecast> img)
{
    if (img.ndim() != 3 || img.shape(2) != 4) throw py::value_error("expected (H, W, 4) uint8");
    std::vector<uint8_t> png = vfh::encode_png_rgba8(img.data(), (uint32_t)img.shape(1), (uint32_t)img.shape(0));
    return py::bytes(reinterpret_cast<const char *>(png.data()), png.size());
}

template <class T>
py::class_<T> bind_terrain(py::module_ &m, const char *name)
{
    return py::class_<T>(m, name)
        .def(py::init<uint32_t, uint32_t, py::object, py::object, py::object>(), py::arg("width"), py::arg("height"), py::arg("grid") = 128,
             py::arg("colormap") = "viridis", py::kw_only(), py::arg("supersample") = 1)
        .def_property_readonly("supersample", &T::supersample, "The supersampling factor f per axis (1: none).")
        .def_property_readonly("samples", &T::samples, "Samples per pixel, f * f.")
        .def_property_readonly("sample_size", &T::sample_size, "(f * width, f * height): the size the terrain is drawn at.")
        .def("render_samples", &T::render_samples,
             "The samples of the current frame before the resolve, (f * height, f * width, 4) uint8: terrain and passes, no overlays.")
        .def("render_png", &T::render_png, py::arg("path"))
        .def("render_rgba", &T::render_rgba)
        .def("render_batch", &T::render_batch, py::arg("poses"), py::arg("paths") = py::none())
        .def("set_camera_look_at", &T::set_camera_look_at, py::arg("eye"), py::arg("target"), py::arg("up"), py::arg("fovy_deg"),
             py::arg("znear"), py::arg("zfar"))
        .def("debug_uniforms_f32", &T::debug_uniforms_f32)
        .def("debug_lut_format", &T::debug_lut_format)
        .def("debug_visibility", &T::debug_visibility)
        .def("set_shard", &T::set_shard, py::arg("rank"), py::arg("nranks"), py::arg("band_h") = 64)
        .def("set_shade_mode", &T::set_shade_mode, py::arg("mode"))
        .def("set_shade_precision", &T::set_shade_precision, py::arg("precision"))
        .def("enable_timing", &T::enable_timing, py::arg("on") = true)
        .def("last_timings", &T::last_timings)
        .def("add_points", &T::add_points, py::arg("xyz"), py::kw_only(), py::arg("size_px") = 5.0f,
             py::arg("rgba") = py::make_tuple(255, 255, 255, 255), py::arg("shape") = "circle", py::arg("drape") = false,
             py::arg("occlude") = false, py::arg("depth_bias") = VF_OCCLUSION_DEPTH_BIAS, py::arg("haze") = false)
        .def("add_lines", &T::add_lines, py::arg("paths"), py::kw_only(), py::arg("width_px") = 2.0f,
             py::arg("rgba") = py::make_tuple(255, 255, 255, 255), py::arg("cap") = "round", py::arg("drape") = false,
             py::arg("occlude") = false, py::arg("depth_bias") = VF_OCCLUSION_DEPTH_BIAS, py::arg("haze") = false)
        .def("set_layer_occlusion", &T::set_layer_occlusion, py::arg("layer"), py::arg("occlude"),
             py::arg("depth_bias") = VF_OCCLUSION_DEPTH_BIAS)
        .def("set_layer_haze", &T::set_layer_haze, py::arg("layer"), py::arg("on") = true,
             "A point, line or contour layer takes the handle's atmospheric haze (set_haze), or stops taking it (DESIGN.md 4r).  The flag\n"
             "rests with the layer until clear_overlays() and does nothing while haze is disabled or has density 0.")
        .def("layer_haze", &T::layer_haze, py::arg("layer"))
        .def("add_polygons", &T::add_polygons, py::arg("polygons"), py::kw_only(), py::arg("fill_rgba") = py::make_tuple(255, 255, 255, 255),
             py::arg("line_rgba") = py::none(), py::arg("line_width_px") = 1.0f, py::arg("drape") = false)
        .def("add_contours", &T::add_contours, py::arg("levels") = py::none(), py::kw_only(), py::arg("interval") = py::none(),
             py::arg("base") = 0.0, py::arg("width_px") = 1.0f, py::arg("rgba") = py::make_tuple(0, 0, 0, 255), py::arg("lift") = 0.0f,
             py::arg("join") = "round", py::arg("occlude") = false, py::arg("depth_bias") = VF_OCCLUSION_DEPTH_BIAS,
             py::arg("haze") = false)
        .def("height_bounds", &T::height_bounds)
        .def("layer_primitive_count", &T::layer_primitive_count, py::arg("layer"))
        .def("clear_overlays", &T::clear_overlays)
        .def("render_gbuffer", &T::render_gbuffer, py::arg("planes") = py::make_tuple("depth", "position", "normal", "primitive"))
        .def("render_depth", &T::render_depth)
        .def("pick", &T::pick, py::arg("pixels"))
        .def("set_shadows", &T::set_shadows, py::arg("enabled") = true, py::kw_only(), py::arg("strength") = VF_SHADOW_STRENGTH,
             py::arg("softness") = VF_SHADOW_SOFTNESS, py::arg("bias") = VF_SHADOW_BIAS,
             "Cast sun shadows on the terrain (DESIGN.md 4g).  The three parameters are stored by every call, also one that disables, and\n"
             "steer shadow_field() too: set_shadows(False) without them puts the defaults back.")
        .def("shadow_field", &T::shadow_field)
        .def("debug_shadow_scans", &T::debug_shadow_scans)
        .def("set_ambient_occlusion", &T::set_ambient_occlusion, py::arg("enabled") = true, py::kw_only(), py::arg("strength") = VF_AMBIENT_STRENGTH,
             py::arg("reach") = VF_AMBIENT_REACH, py::arg("directions") = VF_AMBIENT_DIRECTIONS,
             "Ambient occlusion from a sky-view scan of the height field (DESIGN.md 4i).  directions: how many of the default set, or a\n"
             "(D, 2) array of (ux, uz).  The parameters are stored by every call, also one that disables, and steer sky_view_field() too:\n"
             "set_ambient_occlusion(False) without them puts the defaults back.")
        .def("sky_view_field", &T::sky_view_field)
        .def("debug_ambient_scans", &T::debug_ambient_scans)
        .def("set_drape", &T::set_drape, py::arg("image"), py::kw_only(), py::arg("extent") = py::none(), py::arg("opacity") = 1.0,
             py::arg("filter") = "linear",
             "Drape an image on the terrain as its albedo (DESIGN.md 4j).  image: (ih, iw, 4) or (ih, iw, 3) uint8, sRGB bytes with\n"
             "straight alpha; row 0 lies at the extent's z0 and column 0 at its x0, as in the height array.  extent: (x0, z0, x1, z1)\n"
             "in the world plane of the grid (vertices at -1.5 ... 1.5), None: the whole grid.  The handle keeps a copy made at the\n"
             "call; a second call replaces it.  The image is lit and shadowed as the surface is; overlays composite on top.")
        .def("clear_drape", &T::clear_drape, "Drop the draped image and free its copy: the handle draws as before.")
        .def("drape_info", &T::drape_info, "None, or dict(width, height, extent, opacity, filter) of the drape as set.")
        .def("set_drape_mipmaps", &T::set_drape_mipmaps, py::arg("enabled") = true, py::kw_only(), py::arg("bias") = 0.0,
             "Sample the draped image through a mip pyramid at the level of detail of each pixel's footprint (DESIGN.md 4k): an image\n"
             "denser than the frame no longer aliases.  bias is added to the level, a finite number in [-16, 16].  A setting of the\n"
             "handle, off by default, that survives set_drape and clear_drape; the pyramid (a third of the image's texels at 8 bytes)\n"
             "exists while a drape is held and mipmaps are on.  Where the image is magnified the frame is the unmipped one.")
        .def("drape_mip_info", &T::drape_mip_info,
             "None while mipmaps are off, else dict(levels, sizes=[(w, h), ...], bias, bytes, builds); levels 0 without a drape.")
        .def("read_drape_level", &T::read_drape_level, py::arg("level"),
             "Level 1 <= level < levels of the pyramid as (h, w, 4) float16: premultiplied linear (r, g, b, a).  Builds it if stale.")
        .def("set_drape_anisotropy", &T::set_drape_anisotropy, py::arg("max_anisotropy") = 1,
             "Anisotropic filtering of the mip sampling (DESIGN.md 4p): a pixel whose footprint on the image is longer than wide takes\n"
             "up to max_anisotropy (1, 2, 4, 8 or 16) samples along the longer axis at the level of detail of the shorter, so oblique\n"
             "ground keeps its detail.  A setting of the handle, 1 by default, that survives set_drape, clear_drape and mipmaps off / on;\n"
             "it has no effect while mipmaps are off and never rebuilds the pyramid.")
        .def("drape_anisotropy", &T::drape_anisotropy, "The largest anisotropy as set (1: off).")
        .def("set_viewshed", &T::set_viewshed, py::arg("observer"), py::kw_only(), py::arg("enabled") = true, py::arg("eye_height") = VF_VIEWSHED_EYE_HEIGHT,
             py::arg("target_height") = VF_VIEWSHED_TARGET_HEIGHT, py::arg("radius") = py::none(), py::arg("visible_rgba") = py::make_tuple(64, 255, 96, 96),
             py::arg("hidden_rgba") = py::make_tuple(0, 0, 0, 0), py::arg("softness") = VF_VIEWSHED_SOFTNESS, py::arg("bias") = VF_VIEWSHED_BIAS,
             "Viewshed analysis (DESIGN.md 4l): tint the frame by what an observer sees.  observer = (x, z) in the overlays' world frame\n"
             "(the one add_points takes), snapped to the nearest grid vertex; eye_height and target_height are in the units of\n"
             "y = h * exag; radius (world units) limits the tint to a disc around the observer, None: everywhere.  The tint is flat:\n"
             "hidden_rgba over hidden ground, visible_rgba over seen ground, each with its alpha.  Every parameter is stored by every\n"
             "call, also one that disables, and steers viewshed_field() too.")
        .def("clear_viewshed", &T::clear_viewshed, "Forget the observer: the viewshed is off, its parameters are the defaults again, its buffers are freed.")
        .def("viewshed_field", &T::viewshed_field, "(grid, grid) float32, row j = z index, column i = x index: 1 = seen from the observer, 0 = hidden.")
        .def("viewshed_info", &T::viewshed_info,
             "dict(enabled, vertex (i, j), observer_xyz (world), eye_y, eye_height, target_height, radius, visible_rgba, hidden_rgba,\n"
             "softness, bias); vertex, observer_xyz and eye_y are None before an observer is set.")
        .def("debug_viewshed_scans", &T::debug_viewshed_scans)
        .def("set_cumulative_viewshed", &T::set_cumulative_viewshed, py::arg("observers"), py::kw_only(), py::arg("enabled") = true,
             py::arg("eye_height") = VF_VIEWSHED_EYE_HEIGHT, py::arg("target_height") = VF_VIEWSHED_TARGET_HEIGHT, py::arg("radius") = py::none(),
             py::arg("high_rgba") = py::make_tuple(64, 255, 96, 160), py::arg("low_rgba") = py::make_tuple(0, 0, 0, 0),
             py::arg("softness") = VF_VIEWSHED_SOFTNESS, py::arg("bias") = VF_VIEWSHED_BIAS,
             "Cumulative viewshed (DESIGN.md 4m): tint the frame by how many of N observers see the ground.  observers = (N, 2) points\n"
             "(x, z) in the overlays' world frame, 1 <= N <= 65535, each snapped to the nearest grid vertex; eye_height, target_height,\n"
             "softness and bias are shared by all of them and mean what they mean for set_viewshed; radius (world units): an observer\n"
             "counts only for the ground within it, None: everywhere.  The tint is flat: low_rgba where nobody sees the ground, high_rgba\n"
             "where everybody does, blended by count / N in between.  Every parameter is stored by every call, also one that disables,\n"
             "and steers cumulative_viewshed_field() too.")
        .def("clear_cumulative_viewshed", &T::clear_cumulative_viewshed,
             "Forget the observers: the cumulative viewshed is off, its parameters are the defaults again, its buffers are freed.")
        .def("cumulative_viewshed_field", &T::cumulative_viewshed_field,
             "(grid, grid) float32, row j = z index, column i = x index: the sum of the observers' seen values, in [0, N].")
        .def("cumulative_viewshed_info", &T::cumulative_viewshed_info,
             "dict(enabled, observers (N), batch, vertices ((N, 2) uint32 (i, j)), eye_height, target_height, radius, high_rgba, low_rgba,\n"
             "softness, bias); vertices is None before observers are set.")
        .def("debug_cumulative_viewshed_batch", &T::debug_cumulative_viewshed_batch, py::arg("batch") = 0)
        .def("debug_cumulative_viewshed_scans", &T::debug_cumulative_viewshed_scans)
        .def("set_sun_exposure", &T::set_sun_exposure, py::arg("suns"), py::kw_only(), py::arg("weights") = py::none(), py::arg("incidence") = false,
             py::arg("enabled") = true, py::arg("softness") = VF_SHADOW_SOFTNESS, py::arg("bias") = VF_SHADOW_BIAS,
             py::arg("high_rgba") = py::make_tuple(255, 208, 64, 160), py::arg("low_rgba") = py::make_tuple(0, 0, 0, 0),
             "Sun exposure (DESIGN.md 4n): tint the frame by how much direct sun the ground gets from N suns.  suns = (N, 2) angles\n"
             "(elevation_deg, azimuth_deg) as set_sun takes them, or (N, 3) direction vectors, 1 <= N <= 65535; a sun on or below the\n"
             "horizon is not counted.  weights = (N,) numbers in [0, 1] (None: all 1).  Each sun's shadow field (strength 1, the call's\n"
             "softness and bias) times its weight -- with incidence=True also times the cosine between the sun and the surface normal --\n"
             "is added up; the tint is low_rgba where the sum is 0, high_rgba where it equals the sum of the counted weights, blended in\n"
             "between.  Every parameter is stored by every call, also one that disables, and steers sun_exposure_field() too.")
        .def("clear_sun_exposure", &T::clear_sun_exposure, "Forget the suns: sun exposure is off, its parameters are the defaults again, its buffers are freed.")
        .def("sun_exposure_field", &T::sun_exposure_field,
             "(grid, grid) float32, row j = z index, column i = x index: the weighted sum of the suns' lit values, in [0, sum of weights].")
        .def("sun_exposure_info", &T::sun_exposure_info,
             "dict(enabled, suns (N), counted, weight_total, incidence, batch, softness, bias, high_rgba, low_rgba).")
        .def("debug_sun_exposure_batch", &T::debug_sun_exposure_batch, py::arg("batch") = 0)
        .def("debug_sun_exposure_scans", &T::debug_sun_exposure_scans)
        .def("set_haze", &T::set_haze, py::arg("density"), py::kw_only(), py::arg("rgba") = py::make_tuple(200, 215, 235, 255), py::arg("start") = 0.0f,
             py::arg("falloff") = py::none(), py::arg("base") = 0.0f, py::arg("max_opacity") = 1.0f, py::arg("background") = false,
             py::arg("enabled") = true,
             "Atmospheric haze (DESIGN.md 4q): blend `rgba` over the terrain with opacity 1 - exp(-density * path), the path being the\n"
             "view depth beyond `start`.  falloff (world units of y): the density falls off exponentially with height above `base`;\n"
             "None: uniform haze.  max_opacity caps the opacity; background: pixels without terrain take max_opacity, so the far edge of\n"
             "the terrain fades into the sky.  Haze covers shadows, the drape and the tints; overlays are composited on top and are not\n"
             "hazed.  Every parameter is stored by every call, also one that disables, and steers haze_opacity() too.")
        .def("clear_haze", &T::clear_haze, "Haze off, its parameters the defaults again, its opacity plane freed.")
        .def("haze_info", &T::haze_info, "dict: the haze settings as stored (falloff None: uniform) and eye_y, the eye's height for the current camera.")
        .def("haze_opacity", &T::haze_opacity,
             "(height, width) float32 (the sample size on a supersampled object): the haze opacity of every pixel of the current frame for\n"
             "the stored settings, enabled or not; 0 where the pass leaves the pixel.")
        .def("set_flood", &T::set_flood, py::arg("level"), py::arg("seeds") = py::none(), py::kw_only(), py::arg("enabled") = true,
             py::arg("shallow_rgba") = py::make_tuple(96, 176, 224, 128), py::arg("deep_rgba") = py::make_tuple(16, 64, 160, 224),
             py::arg("depth_full") = VF_FLOOD_DEPTH_FULL,
             "Flood analysis (DESIGN.md 4s): paint the ground that lies below `level` and that water can reach.  level is in units of the\n"
             "height before exaggeration, as contour levels are: add_contours([level]) draws the shoreline.  seeds=None: every vertex below\n"
             "the level (the plain bathtub); seeds=\"edges\": water comes in over the border of the grid; seeds=(N, 2) points (x, z) in the\n"
             "overlays' world frame, 1 <= N <= 65535, each snapped to the nearest grid vertex: water spreads from them through 4-connected\n"
             "vertices below the level, so ground behind a dike stays dry.  The tint is flat: shallow_rgba at the waterline, deep_rgba where\n"
             "the water is depth_full deep or more, blended in between.  Every parameter is stored by every call, also one that disables,\n"
             "and steers flood_field() too.")
        .def("clear_flood", &T::clear_flood, "The flood is off, its parameters are the defaults again, its buffers are freed.")
        .def("flood_field", &T::flood_field,
             "(grid, grid) float32, row j = z index, column i = x index: the water depth level - h where the vertex is flooded, else 0.")
        .def("flood_info", &T::flood_info,
             "dict(enabled, level, mode, seeds (N), vertices ((N, 2) uint32 (i, j)), shallow_rgba, deep_rgba, depth_full, flooded_vertices,\n"
             "wettable_vertices, passes, scans, group); the counts and passes are those of the last computation of the field.")
        .def("debug_flood_group", &T::debug_flood_group, py::arg("group") = 0)
        .def("debug_flood_scans", &T::debug_flood_scans)
        .def("set_spill", &T::set_spill, py::arg("seeds") = "edges", py::kw_only(), py::arg("enabled") = true,
             py::arg("shallow_rgba") = py::make_tuple(96, 176, 224, 128), py::arg("deep_rgba") = py::make_tuple(16, 64, 160, 224),
             py::arg("depth_full") = VF_SPILL_DEPTH_FULL,
             "Spill analysis (DESIGN.md 4t): the lowest level the water must reach at the sources before a vertex gets wet (the minimax\n"
             "path height over 4-connected paths of finite vertices), and a tint of the closed basins by their depth spill - h.\n"
             "seeds=\"edges\": the border of the grid is the source, the field is the depression-filled surface; seeds=(N, 2) points (x, z)\n"
             "in the overlays' world frame, 1 <= N <= 65535, each snapped to the nearest grid vertex: spill_field() < L is what\n"
             "set_flood(L, seeds) floods.  The tint is flat: shallow_rgba at the rim, deep_rgba where the basin is depth_full deep or more,\n"
             "blended in between.  Every parameter is stored by every call, also one that disables, and steers the field calls too.")
        .def("clear_spill", &T::clear_spill, "The spill is off, its parameters are the defaults again, its buffers are freed.")
        .def("spill_field", &T::spill_field,
             "(grid, grid) float32, row j = z index, column i = x index: the spill level of the vertex, +inf where no path arrives.")
        .def("sink_depth_field", &T::sink_depth_field, "(grid, grid) float32: spill - h where that is finite, 0 elsewhere.")
        .def("spill_info", &T::spill_info,
             "dict(enabled, mode, seeds (N), vertices ((N, 2) uint32 (i, j)), shallow_rgba, deep_rgba, depth_full, reached_vertices,\n"
             "sink_vertices, passes, scans, group, tile_runs); the counts, passes and tile_runs are those of the last computation.")
        .def("debug_spill_group", &T::debug_spill_group, py::arg("group") = 0)
        .def("debug_spill_scans", &T::debug_spill_scans)
        .def("set_sun", &T::set_sun, py::arg("elevation_deg"), py::arg("azimuth_deg"))
        .def("set_exposure", &T::set_exposure, py::arg("exposure"));
}

} // namespace

PYBIND11_MODULE(_vulkan_forge, m)
{
    m.doc() = "MI355X-native drop-in for vulkan-forge's _vulkan_forge extension (terrain raster hot path)";
    py::class_<Renderer>(m, "Renderer")
        .def(py::init<uint32_t, uint32_t>(), py::arg("width"), py::arg("height"))
        .def("info", &Renderer::info)
        .def("render_triangle_rgba", &Renderer::render_triangle_rgba)
        .def("render_triangle_png", &Renderer::render_triangle_png, py::arg("path"))
        .def("add_terrain", &Renderer::add_terrain, py::arg("heightmap"), py::arg("spacing"), py::arg("exaggeration") = 1.0f,
             py::arg("colormap") = "viridis")
        .def("terrain_stats", &Renderer::terrain_stats)
        .def("set_height_range", &Renderer::set_height_range, py::arg("min"), py::arg("max"))
        .def("set_sun", &Renderer::set_sun, py::arg("elevation_deg"), py::arg("azimuth_deg"))
        .def("set_exposure", &Renderer::set_exposure, py::arg("exposure"))
        .def("normalize_terrain", &Renderer::normalize_terrain, py::arg("mode"), py::arg("range") = py::none(), py::arg("eps") = py::none())
        .def("upload_height_r32f", &Renderer::upload_height_r32f)
        .def("debug_read_height_patch", &Renderer::debug_read_height_patch, py::arg("x"), py::arg("y"), py::arg("w"), py::arg("h"))
        .def("read_full_height_texture", &Renderer::read_full_height_texture);
    bind_terrain<TerrainSpike>(m, "TerrainSpike");
    bind_terrain<Scene>(m, "Scene").def("set_height_from_r32f", &Scene::set_height_from_r32f, py::arg("height_r32f"));
    m.def("enumerate_adapters", &enumerate_adapters);
    m.def("device_probe", &device_probe, py::arg("backend") = py::none());
    m.def("grid_generate", &grid_generate, py::arg("nx"), py::arg("nz"), py::arg("spacing") = std::make_tuple(1.0f, 1.0f),
          py::arg("origin") = "center");
    m.def("colormap_supported", &colormap_supported);
    m.def("colormap_rgba8", &colormap_rgba8, py::arg("name"));
    m.def("_encode_png_rgba8", &py_encode_png, py::arg("rgba"));
    m.def("camera_look_at", &camera_look_at, py::arg("eye"), py::arg("target"), py::arg("up"));
    m.def("camera_perspective", &camera_perspective, py::arg("fovy_deg"), py::arg("aspect"), py::arg("znear"), py::arg("zfar"),
          py::arg("clip_space") = "wgpu");
    m.def("camera_view_proj", &camera_view_proj, py::arg("eye"), py::arg("target"), py::arg("up"), py::arg("fovy_deg"),
          py::arg("aspect"), py::arg("znear"), py::arg("zfar"), py::arg("clip_space") = "wgpu");
}

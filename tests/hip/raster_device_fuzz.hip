// raster_device_fuzz.hip -- the span solver (vulkan_forge_amd/csrc/vf_raster.h) and the line loop that walks it (raster_fast,
// vf_kernels.h) run AS DEVICE CODE against the brute-force int64 coverage rule of tests/cpp/raster_cases.h.  The host harness
// (tests/cpp/raster_fuzz.cpp) checks the host build of the header; on the GPU rs_rcp is v_rcp_f32, rs_floor_i the inline
// v_cvt_flr_i32_f32, rs_med3 v_med3_f32, span_exact device FP64 division and FMA, all of it under the library's -O3 / -mllvm
// switches -- and raster_fast exists as device code only.  Built (with __graft_entry__.HIPCC_FLAGS) and run by
// tests/test_gpu_raster_device.py:
//     raster_device_fuzz <draws> <seed> <soup cases> [target extent]      (0 soup cases: part 1 alone)
//
// Part 1, spans: the case stream of raster_cases.h, one thread per accepted case.  The kernel calls span_setup, span_group for every
// run of four lines, span_line / span_confirm / span_exact for every line and stores what they return; the host makes the four
// checks of raster_fuzz.cpp on those numbers and prints the same summary; a fifth holds the error margin the solver applies against
// the bound its header derives (a margin that is too thin, yet wider than the errors that occur, changes no result).  Nothing the
// kernel computes is an address: where a result is stored comes from the host's prefix sums and the loop bounds from the case, so
// it stays in bounds whatever the solver returns.
//
// Part 2, triangle soup: one wave per case calls raster_fast<GROUPS> on a TileCtx built in LDS the way k_tile builds it: the case's
// triangle and window from the same stream, nsub cooperating lanes from lane `first`, a final-pixel set (empty / sparse / dense /
// whole lines / everything) given as column AND row masks, four-line masks that are the exact AND or lag behind it, and a
// visibility tile pre-filled with ids below and above the triangle's.  The wave's other lane groups walk OTHER triangles of the
// stream (moved by whole pixels onto the same box corner) with word 0 -- an atomic max with 0 paints nothing -- so the ballots that
// carry the group verdicts see foreign lanes, as they do in k_tile.  The whole 64 x 64 tile comes back and must equal
// max(prior, word) where the pixel centre is covered, inside the window and not final, and prior everywhere else.
// raster_fast's paint offset is masked into the tile by construction (line * 256 + (... & 252) with line and bit index < 64:
// below 16 KB, the size of the LDS tile), and its mask loads are indexed by the line number inside the window, so a wrong span
// cannot touch memory outside the kernel's LDS arrays.
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>
#include "../cpp/raster_cases.h"
#include "../../vulkan_forge_amd/csrc/vf_kernels.h"

using namespace vf;
using raster_cases::covered;

#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) { printf("HIP error %s at %s:%d: %s\n", hipGetErrorName(e_), __FILE__, __LINE__, #expr); fflush(stdout); exit(2); } \
    } while (0)

static constexpr int kHostThreads = 8;

template <typename F>
static void parallel_chunks(size_t n, F &&fn)              // fn(thread, begin, end)
{
    std::vector<std::thread> pool;
    const size_t per = (n + kHostThreads - 1) / kHostThreads;
    for (int t = 0; t < kHostThreads; ++t) {
        const size_t a = std::min(n, per * t), b = std::min(n, per * (t + 1));
        pool.emplace_back([&fn, t, a, b] { fn(t, a, b); });
    }
    for (auto &th : pool) th.join();
}

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---------------------------------------------------------------------------------------------
// part 1: the span solver
// ---------------------------------------------------------------------------------------------
struct SpanCase { int32_t U[3], V[3], u0c, v0c, n_outer, n_inner, swapped; uint32_t line0, group0; };
struct LineOut { int32_t lo, hi, elo, ehi, F[3], confirm; };
struct GroupOut { int32_t lo, hi; };
struct SetupOut { int32_t regular; float eps2[3]; };

__global__ __launch_bounds__(256) void k_spans(const SpanCase *__restrict__ cases, uint32_t n, LineOut *__restrict__ lines, GroupOut *__restrict__ groups,
                                               SetupOut *__restrict__ setups)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const SpanCase c = cases[i];
    SpanSetup S;
    span_setup(c.U, c.V, c.swapped != 0, c.u0c, c.v0c, c.n_outer, S);
    SetupOut so;
    so.regular = S.regular ? 1 : 0;
    for (int k = 0; k < 3; ++k) so.eps2[k] = S.eps2[k];
    setups[i] = so;
    uint32_t g = c.group0;
    for (int32_t oa = 0; oa <= c.n_outer; oa += 4, ++g) {
        GroupOut go;
        span_group(S, oa, min(oa + 3, c.n_outer), c.n_inner, go.lo, go.hi);
        groups[g] = go;
    }
    for (int32_t o = 0; o <= c.n_outer; ++o) {
        LineOut lo;
        span_line(S, o, c.n_inner, lo.F, lo.lo, lo.hi);
        lo.confirm = span_confirm(S, o, c.n_inner, lo.F) ? 1 : 0;
        span_exact(c.U, c.V, c.swapped != 0, c.u0c, c.v0c, o, c.n_inner, lo.elo, lo.ehi);
        lines[c.line0 + (uint32_t)o] = lo;
    }
}

static long check_spans(const std::vector<raster_cases::Case> &cs)
{
    const size_t n = cs.size();
    std::vector<SpanCase> h_cases(n);
    uint32_t nlines = 0, ngroups = 0;
    for (size_t i = 0; i < n; ++i) {
        const raster_cases::SolverArgs a = raster_cases::solver_args(cs[i]);
        SpanCase &s = h_cases[i];
        for (int k = 0; k < 3; ++k) { s.U[k] = a.U[k]; s.V[k] = a.V[k]; }
        s.u0c = a.u0c; s.v0c = a.v0c; s.n_outer = a.n_outer; s.n_inner = a.n_inner; s.swapped = a.cols ? 0 : 1;
        s.line0 = nlines; s.group0 = ngroups;
        nlines += (uint32_t)a.n_outer + 1u; ngroups += (uint32_t)a.n_outer / 4u + 1u;
    }
    SpanCase *d_cases; LineOut *d_lines; GroupOut *d_groups; SetupOut *d_regular;
    HIP_TRY(hipMalloc(&d_cases, n * sizeof(SpanCase)));
    HIP_TRY(hipMalloc(&d_lines, (size_t)nlines * sizeof(LineOut)));
    HIP_TRY(hipMalloc(&d_groups, (size_t)ngroups * sizeof(GroupOut)));
    HIP_TRY(hipMalloc(&d_regular, n * sizeof(SetupOut)));
    HIP_TRY(hipMemcpy(d_cases, h_cases.data(), n * sizeof(SpanCase), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_lines, 0xFF, (size_t)nlines * sizeof(LineOut)));
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0));
    k_spans<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(d_cases, (uint32_t)n, d_lines, d_groups, d_regular);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e1));
    HIP_TRY(hipDeviceSynchronize());
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    std::vector<LineOut> lines(nlines);
    std::vector<GroupOut> groups(ngroups);
    std::vector<SetupOut> regular(n);
    HIP_TRY(hipMemcpy(lines.data(), d_lines, (size_t)nlines * sizeof(LineOut), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(groups.data(), d_groups, (size_t)ngroups * sizeof(GroupOut), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(regular.data(), d_regular, n * sizeof(SetupOut), hipMemcpyDeviceToHost));
    HIP_TRY(hipFree(d_cases)); HIP_TRY(hipFree(d_lines)); HIP_TRY(hipFree(d_groups)); HIP_TRY(hipFree(d_regular));

    struct Counts { long lines = 0, nonempty = 0, fallback = 0, irregular = 0, bad = 0, thin = 0, edges = 0, group_lines = 0, group_slack = 0, f_differs = 0, reg_differs = 0;
                    long k_tris[10] = {0}, k_irr[10] = {0}, k_lines[10] = {0}, k_fb[10] = {0}; };
    std::vector<Counts> per(kHostThreads);
    std::atomic<long> printed{0};
    std::mutex mu;
    const double t0 = now_s();
    parallel_chunks(n, [&](int t, size_t begin, size_t end) {
        Counts &C = per[t];
        auto fail = [&](const char *what, size_t c, int32_t o, int32_t lo, int32_t hi, int32_t tlo, int32_t thi, int ncov) {
            ++C.bad;
            if (printed.fetch_add(1) < 10) {
                std::lock_guard<std::mutex> lk(mu);
                printf("%s: accepted case %zu (kind %d) line %d: [%d,%d] vs true [%d,%d] (ncov %d)\n", what, c, cs[c].kind, o, lo, hi, tlo, thi, ncov);
            }
        };
        for (size_t c = begin; c < end; ++c) {
            const raster_cases::Case &rc = cs[c];
            const raster_cases::SolverArgs a = raster_cases::solver_args(rc);
            const SpanCase &s = h_cases[c];
            const int kind = rc.kind;
            const bool reg = regular[c].regular != 0;
            C.irregular += reg ? 0 : 1; C.k_tris[kind]++; C.k_irr[kind] += reg ? 0 : 1;
            SpanSetup HS;                                  // the host build of the same header (this translation unit's host pass): for information
            span_setup(a.U, a.V, !a.cols, a.u0c, a.v0c, a.n_outer, HS);
            C.reg_differs += HS.regular != reg ? 1 : 0;
            // the margin: results cannot show an eps that is smaller than the one vf_raster.h derives as long as it still exceeds the
            // rounding error that actually occurs (the derivation rounds every constant up), so the applied eps is held against the
            // derived bound itself, evaluated in FP64 from the integers:
            //     eps_i >= (((2 |gg| + span) |s| + |cc|) 2^-21 + |rc| 2^-8 + 2^-16) (1 - 2^-19)
            // (1 - 2^-19: the FP32 evaluation carries the 1-ulp reciprocal (2^-23) into rc and s and rounds gg, cc, the product that forms
            // s and four fused operations by 2^-24 each; every term is positive, so the relative errors do not amplify: under 2^-21
            // in all.)  An edge parallel to the lines has no crossing and no eps.
            for (int i = 0; i < 3; ++i) {
                const int ea = i == 0 ? 1 : (i == 1 ? 2 : 0), eb = i == 0 ? 2 : (i == 1 ? 0 : 1);
                const double dU = (double)a.U[eb] - a.U[ea], dV = (double)a.V[eb] - a.V[ea];
                if (dU == 0.0) continue;
                const double gg = fabs(((double)a.u0c - a.U[ea]) / 256.0), cc = fabs(((double)a.V[ea] - a.v0c) / 256.0), sl = fabs(dV / dU);
                const double bound = ((2.0 * gg + (double)(a.n_outer + 1)) * sl + cc) * 0x1.0p-21 + fabs(1.0 / dU) * 0x1.0p-8 + 0x1.0p-16;
                ++C.edges;
                if (!((double)regular[c].eps2[i] >= 2.0 * bound * (1.0 - 0x1.0p-19))) {
                    ++C.thin;
                    if (printed.fetch_add(1) < 10) {
                        std::lock_guard<std::mutex> lk(mu);
                        printf("eps below the derived bound: accepted case %zu (kind %d) edge %d: eps %.9g, bound %.9g\n", c, kind, i, 0.5 * (double)regular[c].eps2[i], bound);
                    }
                }
            }
            if (reg)                                       // stage 0: the bound of lines oa .. oa + 3 holds every one of their stage-1 spans
                for (int32_t oa = 0; oa <= a.n_outer; oa += 4) {
                    const int32_t ob = std::min(oa + 3, a.n_outer);
                    const GroupOut &G = groups[s.group0 + (uint32_t)oa / 4u];
                    for (int32_t o = oa; o <= ob; ++o) {
                        const LineOut &L = lines[s.line0 + (uint32_t)o];
                        ++C.group_lines;
                        if (L.lo <= L.hi && (G.lo > L.lo || G.hi < L.hi)) { fail("group bound cuts a line", c, o, L.lo, L.hi, G.lo, G.hi, -1); break; }
                        C.group_slack += (L.lo <= L.hi) ? (L.lo - G.lo) + (G.hi - L.hi) : 0;
                    }
                }
            for (int32_t o = 0; o <= a.n_outer; ++o) {
                ++C.lines; C.k_lines[kind]++;
                int32_t tlo = a.n_inner + 1, thi = -1;     // brute force: first / last covered offset (coverage along a line is an interval)
                int ncov = 0;
                for (int32_t r = 0; r <= a.n_inner; ++r) {
                    const int32_t px = a.cols ? rc.px0 + o : rc.px0 + r, py = a.cols ? rc.py0 + r : rc.py0 + o;
                    if (covered(rc.X, rc.Y, px, py)) { tlo = std::min(tlo, r); thi = std::max(thi, r); ++ncov; }
                }
                if (ncov && ncov != thi - tlo + 1) { fail("NOT AN INTERVAL?!", c, o, 0, 0, tlo, thi, ncov); continue; }
                C.nonempty += ncov ? 1 : 0;
                const LineOut &L = lines[s.line0 + (uint32_t)o];
                {
                    int32_t HF[3], hlo, hhi;
                    span_line(HS, o, a.n_inner, HF, hlo, hhi);
                    C.f_differs += (HF[0] != L.F[0] || HF[1] != L.F[1] || HF[2] != L.F[2]) ? 1 : 0;
                }
                if (reg) {
                    if (ncov && (L.lo > tlo || L.hi < thi || L.lo > L.hi)) { fail("stage 1 cuts the span", c, o, L.lo, L.hi, tlo, thi, ncov); continue; }
                    if (L.lo <= L.hi) {
                        if (L.confirm) {
                            const bool same = ncov ? (L.lo == tlo && L.hi == thi) : false;
                            if (!same) { fail("stage 2 accepts a wrong span", c, o, L.lo, L.hi, tlo, thi, ncov); continue; }
                        } else { ++C.fallback; C.k_fb[kind]++; }
                    }
                }
                const int32_t elo = std::max(L.elo, 0), ehi = std::min(L.ehi, a.n_inner);
                const bool eok = ncov ? (elo == tlo && ehi == thi) : (elo > ehi);
                if (!eok) { fail("span_exact wrong", c, o, elo, ehi, tlo, thi, ncov); continue; }
            }
        }
    });
    const double t1 = now_s();
    Counts T;
    for (const Counts &C : per) {
        T.lines += C.lines; T.nonempty += C.nonempty; T.fallback += C.fallback; T.irregular += C.irregular; T.bad += C.bad + C.thin; T.thin += C.thin; T.edges += C.edges;
        T.group_lines += C.group_lines; T.group_slack += C.group_slack; T.f_differs += C.f_differs; T.reg_differs += C.reg_differs;
        for (int k = 0; k < 10; ++k) { T.k_tris[k] += C.k_tris[k]; T.k_irr[k] += C.k_irr[k]; T.k_lines[k] += C.k_lines[k]; T.k_fb[k] += C.k_fb[k]; }
    }
    const long tris = (long)n;
    printf("triangles %ld (irregular %ld = %.3f %%)  lines %ld  non-empty %ld  stage-2 fallbacks %ld (%.4f %% of lines)  failures %ld\n",
           tris, T.irregular, 100.0 * T.irregular / (tris ? tris : 1), T.lines, T.nonempty, T.fallback, 100.0 * T.fallback / (T.lines ? T.lines : 1), T.bad);
    printf("group bounds: %ld lines checked, mean slack %.2f pixels per non-empty line\n", T.group_lines, (double)T.group_slack / (T.group_lines ? T.group_lines : 1));
    for (int k = 0; k < 10; ++k) printf("  kind %d: triangles %ld irregular %.3f %%  lines %ld fallback %.4f %%\n", k, T.k_tris[k], 100.0 * T.k_irr[k] / (T.k_tris[k] ? T.k_tris[k] : 1), T.k_lines[k], 100.0 * T.k_fb[k] / (T.k_lines[k] ? T.k_lines[k] : 1));
    printf("error margin: eps below the derived bound on %ld of %ld edges\n", T.thin, T.edges);
    printf("device vs host build (information): F[] differs on %ld of %ld lines, `regular` on %ld of %ld triangles\n", T.f_differs, T.lines, T.reg_differs, tris);
    printf("spans timing: kernel %.3f ms, host checks %.3f s\n", ms, t1 - t0);
    return T.bad;
}

// ---------------------------------------------------------------------------------------------
// part 2: raster_fast on triangle soup
// ---------------------------------------------------------------------------------------------
struct SoupCase { uint32_t tri; int32_t px_lo, py_lo, px_hi, py_hi; uint32_t nsub, first, word; };
constexpr uint32_t kFinWords = 2u * (kTileW + kTileH) + 2u * (kTileW / 4 + kTileH / 4);     // colfin, rowfin, colfin4, rowfin4 of one case

// The tile before the triangle: nothing, an id below `word`, or an id above it (k: the word's index in the LDS tile)
__host__ __device__ static inline uint32_t prior_word(uint32_t c, uint32_t k, uint32_t word)
{
    uint32_t h = c * 4096u + k;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    const uint32_t sel = h % 3u, v = h >> 8;
    return sel == 0u ? 0u : (sel == 1u ? 1u + v % (word - 1u) : word + 1u + (v & 0xFFFFu));      // word >= 2
}

__device__ __forceinline__ int32_t first_centre(int32_t a, int32_t b, int32_t c) { return (min(a, min(b, c)) + 127) >> 8; }

template <bool GROUPS>
__global__ __launch_bounds__(64) void k_soup(const int32_t *__restrict__ tris, uint32_t ntri, const SoupCase *__restrict__ cases, uint32_t case0,
                                             const uint32_t *__restrict__ fin, uint32_t *__restrict__ out)
{
    __shared__ uint32_t s_vis[kTileW * kTileH];
    __shared__ uint32_t s_fin[kFinWords];
    __shared__ int2 s_xy[192];
    const uint32_t lane = threadIdx.x, c = case0 + blockIdx.x;
    const SoupCase sc = cases[c];
    for (uint32_t k = lane; k < (uint32_t)(kTileW * kTileH); k += 64u) s_vis[k] = prior_word(c, k, sc.word);
    for (uint32_t k = lane; k < kFinWords; k += 64u) s_fin[k] = fin[(size_t)c * kFinWords + k];
    // the lane groups' triangles: the case's own for the group that starts at `first`, other triangles of the stream for the rest,
    // moved by whole pixels so that their boxes begin at the same pixel centre (they meet the window, and paint nothing: word 0)
    const uint32_t ngroups = 64u / sc.nsub, own = sc.first / sc.nsub;
    if (lane < ngroups) {
        const int32_t *q = tris + 6u * sc.tri;
        int32_t dx = 0, dy = 0;
        if (lane != own) {
            const int32_t *d = tris + 6u * ((sc.tri + 1u + (lane * 7919u + c) % (ntri - 1u)) % ntri);
            dx = (first_centre(q[0], q[2], q[4]) - first_centre(d[0], d[2], d[4])) * 256;
            dy = (first_centre(q[1], q[3], q[5]) - first_centre(d[1], d[3], d[5])) * 256;
            q = d;
        }
        for (uint32_t k = 0; k < 3u; ++k) s_xy[3u * lane + k] = make_int2(q[2u * k] + dx, q[2u * k + 1u] + dy);
    }
    __syncthreads();
    TileCtx T;
    T.vis = s_vis; T.colfin = s_fin; T.rowfin = s_fin + 2 * kTileW; T.colfin4 = s_fin + 2 * (kTileW + kTileH); T.rowfin4 = T.colfin4 + 2 * (kTileW / 4);
    T.px_lo = sc.px_lo; T.px_hi = sc.px_hi; T.py_lo = sc.py_lo; T.py_hi = sc.py_hi;
    const uint32_t gi = lane / sc.nsub, sub = lane - gi * sc.nsub;
    raster_fast<GROUPS>(T, gi == own ? sc.word : 0u, s_xy, (3u * gi) | ((3u * gi + 1u) << 8) | ((3u * gi + 2u) << 16), (int32_t)sub, (int32_t)sc.nsub, gi * sc.nsub);
    __syncthreads();
    for (uint32_t k = lane; k < (uint32_t)(kTileW * kTileH); k += 64u) out[(size_t)blockIdx.x * (kTileW * kTileH) + k] = s_vis[k];
}

static inline uint32_t host_vis_index(int32_t lx, int32_t ly) { return (uint32_t)ly * 64u + (uint32_t)((lx + ly) & 63); }   // vis_index of vf_kernels.h, restated

static long check_soup(const std::vector<raster_cases::Case> &all, size_t nsoup, uint64_t seed)
{
    const size_t n = std::min(nsoup, all.size()), ntri = all.size();
    std::mt19937_64 rng(seed ^ 0x9E3779B97F4A7C15ull);
    auto uni = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    std::vector<int32_t> h_tris(6 * ntri);
    for (size_t i = 0; i < ntri; ++i) for (int k = 0; k < 3; ++k) { h_tris[6 * i + 2 * k] = all[i].X[k]; h_tris[6 * i + 2 * k + 1] = all[i].Y[k]; }
    std::vector<SoupCase> h_cases(n);
    std::vector<uint64_t> rowfin(64 * n);                  // the final-pixel set the expected tile is formed from: bit x of row y
    std::vector<uint32_t> h_fin((size_t)kFinWords * n);
    long n_nsub[7] = {0}, n_kind[10] = {0}, n_mode[5] = {0}, n_lag = 0, n_res[4] = {0};
    for (size_t c = 0; c < n; ++c) {
        const raster_cases::Case &rc = all[c];
        SoupCase &sc = h_cases[c];
        const int e = (int)uni(0, 6);
        sc.tri = (uint32_t)c; sc.px_lo = rc.tx_lo; sc.px_hi = rc.tx_hi; sc.py_lo = rc.ty_lo; sc.py_hi = rc.ty_hi;
        sc.nsub = 1u << e; sc.first = sc.nsub * (uint32_t)uni(0, 64u / sc.nsub - 1u); sc.word = (uint32_t)uni(2, 1u << 25);
        ++n_nsub[e]; ++n_kind[rc.kind];
        ++n_res[(((rc.px1 - rc.px0) <= (rc.py1 - rc.py0)) ? rc.px0 - rc.tx_lo : rc.py0 - rc.ty_lo) & 3];
        static const int modes[13] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4};
        const int mode = modes[uni(0, 12)];
        ++n_mode[mode];
        uint64_t *rf = &rowfin[64 * c];
        uint64_t colsel = rng() & rng(), cf[64];
        for (int y = 0; y < 64; ++y) {
            const uint64_t a = rng(), b = rng(), d = rng(), f = rng();
            rf[y] = mode == 0 ? 0ull : mode == 1 ? (a & b & d & f) : mode == 2 ? (a | b | d | f) : mode == 3 ? ((a & 1ull) ? ~0ull : colsel) : ~0ull;
        }
        for (int x = 0; x < 64; ++x) { cf[x] = 0; for (int y = 0; y < 64; ++y) cf[x] |= ((rf[y] >> x) & 1ull) << y; }
        uint32_t *w = &h_fin[(size_t)kFinWords * c];
        for (int k = 0; k < 64; ++k) { w[2 * k] = (uint32_t)cf[k]; w[2 * k + 1] = (uint32_t)(cf[k] >> 32); w[128 + 2 * k] = (uint32_t)rf[k]; w[128 + 2 * k + 1] = (uint32_t)(rf[k] >> 32); }
        const int lag = (int)uni(0, 3);                    // 0, 1: the exact AND; 2: a random subset of it; 3: never refreshed
        n_lag += lag >= 2;
        for (int g = 0; g < 16; ++g) {
            uint64_t c4 = cf[4 * g] & cf[4 * g + 1] & cf[4 * g + 2] & cf[4 * g + 3], r4 = rf[4 * g] & rf[4 * g + 1] & rf[4 * g + 2] & rf[4 * g + 3];
            if (lag == 2) { c4 &= rng() | rng(); r4 &= rng() | rng(); }
            if (lag == 3) { c4 = 0; r4 = 0; }
            w[256 + 2 * g] = (uint32_t)c4; w[256 + 2 * g + 1] = (uint32_t)(c4 >> 32); w[288 + 2 * g] = (uint32_t)r4; w[288 + 2 * g + 1] = (uint32_t)(r4 >> 32);
        }
    }
    int32_t *d_tris; SoupCase *d_cases; uint32_t *d_fin, *d_out;
    constexpr size_t kBatch = 8192, kTileWords = (size_t)kTileW * kTileH;
    HIP_TRY(hipMalloc(&d_tris, h_tris.size() * sizeof(int32_t)));
    HIP_TRY(hipMalloc(&d_cases, n * sizeof(SoupCase)));
    HIP_TRY(hipMalloc(&d_fin, h_fin.size() * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&d_out, kBatch * kTileWords * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(d_tris, h_tris.data(), h_tris.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_cases, h_cases.data(), n * sizeof(SoupCase), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_fin, h_fin.data(), h_fin.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    std::vector<uint32_t> out(kBatch * kTileWords);
    std::atomic<long> printed{0};
    std::mutex mu;
    long bad_cases[2] = {0, 0}, bad_pixels[2] = {0, 0}, painted = 0, bad_by_nsub[2][7] = {{0}};
    float ms_total = 0.0f;
    const double t0 = now_s();
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    for (int groups = 0; groups < 2; ++groups)
        for (size_t base = 0; base < n; base += kBatch) {
            const size_t nb = std::min(kBatch, n - base);
            HIP_TRY(hipMemset(d_out, 0xEE, nb * kTileWords * sizeof(uint32_t)));
            HIP_TRY(hipEventRecord(e0));
            if (groups) k_soup<true><<<dim3((unsigned)nb), dim3(64)>>>(d_tris, (uint32_t)ntri, d_cases, (uint32_t)base, d_fin, d_out);
            else k_soup<false><<<dim3((unsigned)nb), dim3(64)>>>(d_tris, (uint32_t)ntri, d_cases, (uint32_t)base, d_fin, d_out);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(e1));
            HIP_TRY(hipDeviceSynchronize());
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
            ms_total += ms;
            HIP_TRY(hipMemcpy(out.data(), d_out, nb * kTileWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
            std::vector<long> t_cases(kHostThreads, 0), t_pixels(kHostThreads, 0), t_painted(kHostThreads, 0);
            std::vector<long> t_nsub(kHostThreads * 7, 0);
            parallel_chunks(nb, [&](int t, size_t begin, size_t end) {
                for (size_t i = begin; i < end; ++i) {
                    const size_t c = base + i;
                    const raster_cases::Case &rc = all[c];
                    const SoupCase &sc = h_cases[c];
                    const uint32_t *tile = &out[i * kTileWords];
                    const uint64_t *rf = &rowfin[64 * c];
                    long wrong = 0;
                    int32_t fx = -1, fy = -1; uint32_t fgot = 0, fexp = 0;
                    for (int32_t ly = 0; ly < 64; ++ly)
                        for (int32_t lx = 0; lx < 64; ++lx) {
                            const uint32_t k = host_vis_index(lx, ly), prior = prior_word((uint32_t)c, k, sc.word);
                            const int32_t px = sc.px_lo + lx, py = sc.py_lo + ly;
                            const bool in = px >= rc.px0 && px <= rc.px1 && py >= rc.py0 && py <= rc.py1;     // window and box
                            const bool paint = in && !((rf[ly] >> lx) & 1ull) && covered(rc.X, rc.Y, px, py);
                            const uint32_t expect = paint ? std::max(prior, sc.word) : prior;
                            t_painted[t] += paint ? 1 : 0;
                            if (tile[k] != expect) { if (!wrong) { fx = lx; fy = ly; fgot = tile[k]; fexp = expect; } ++wrong; }
                        }
                    if (wrong) {
                        ++t_cases[t]; t_pixels[t] += wrong; ++t_nsub[t * 7 + __builtin_ctz(sc.nsub)];
                        if (printed.fetch_add(1) < 10) {
                            std::lock_guard<std::mutex> lk(mu);
                            printf("soup: GROUPS %d case %zu (kind %d) nsub %u first %u window x %d..%d y %d..%d box x %d..%d y %d..%d: %ld pixels differ, first at local (%d, %d): %u, expected %u (word %u)\n",
                                   groups, c, rc.kind, sc.nsub, sc.first, sc.px_lo, sc.px_hi, sc.py_lo, sc.py_hi, rc.px0, rc.px1, rc.py0, rc.py1, wrong, fx, fy, fgot, fexp, sc.word);
                        }
                    }
                }
            });
            for (int t = 0; t < kHostThreads; ++t) {
                bad_cases[groups] += t_cases[t]; bad_pixels[groups] += t_pixels[t]; painted += t_painted[t];
                for (int e = 0; e < 7; ++e) bad_by_nsub[groups][e] += t_nsub[t * 7 + e];
            }
        }
    const double t1 = now_s();
    HIP_TRY(hipFree(d_tris)); HIP_TRY(hipFree(d_cases)); HIP_TRY(hipFree(d_fin)); HIP_TRY(hipFree(d_out));
    for (int groups = 0; groups < 2; ++groups) {
        printf("soup GROUPS %d: cases %zu  failures %ld (%ld pixels)  per nsub", groups, n, bad_cases[groups], bad_pixels[groups]);
        for (int e = 0; e < 7; ++e) printf("  %d: %ld cases %ld failed", 1 << e, n_nsub[e], bad_by_nsub[groups][e]);
        printf("\n");
    }
    printf("soup kinds:");
    for (int k = 0; k < 10; ++k) printf(" %ld", n_kind[k]);
    printf("  final sets (empty sparse dense lines all): %ld %ld %ld %ld %ld  lagging four-line masks: %ld  first line mod 4: %ld %ld %ld %ld  pixels painted: %ld\n",
           n_mode[0], n_mode[1], n_mode[2], n_mode[3], n_mode[4], n_lag, n_res[0], n_res[1], n_res[2], n_res[3], painted / 2);
    printf("soup timing: kernels %.3f ms, all of part 2 %.3f s\n", ms_total, t1 - t0);
    return bad_cases[0] + bad_cases[1];
}

int main(int argc, char **argv)
{
    const long draws = argc > 1 ? atol(argv[1]) : 250000;
    const uint64_t seed = argc > 2 ? (uint64_t)atoll(argv[2]) : 1;
    const long nsoup = argc > 3 ? atol(argv[3]) : 24000;
    const long extent = argc > 4 ? atol(argv[4]) : 4096;      // the target the triangles lie around (raster_cases.h)
    const double t0 = now_s();
    raster_cases::Stream stream(seed, extent);
    std::vector<raster_cases::Case> cs;
    for (long c = 0; c < draws; ++c) {
        raster_cases::Case rc;
        if (stream.draw(rc)) cs.push_back(rc);
    }
    if (cs.size() < 2) { printf("no cases\n"); return 2; }
    const long bad_spans = check_spans(cs);
    const long bad_soup = nsoup > 0 ? check_soup(cs, (size_t)nsoup, seed) : 0;
    printf("total time %.3f s\n", now_s() - t0);
    return (bad_spans || bad_soup) ? 1 : 0;
}

/* spill_model.c -- CPU model of the spill analysis, the contract the gfx950 kernels of vulkan_forge_amd/csrc/vf_spill.h
 * (k_spill_init / _seed / _pass / _out / _tint) are held to bit for bit.  Written from the contract: the field is a priority flood (a
 * binary heap on the keys) from the sources, with no tiles and no relaxation; spm_tile_passes is the other thing, the emulation of the
 * kernels' launches with Jacobi halos; the tinted frame takes a frame and its visibility ids, interpolates sd = spill - h of the three
 * vertices of every covered pixel with the geometry-buffer model's weights (clip, fan, last covering piece) and blends the two colours
 * as the flood model does.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC spill_model.c -o libspmodel.so -lm     (spill_model.py does this)
 */
#include "../viewshed_model/viewshed_model.c"

enum { SPM_EDGES = 1, SPM_SEEDS = 2 };
#define SPM_INF 0xFF800000u                                    /* key(+inf) */

/* ---- the order (contract item 1) ---- */

uint32_t spm_key(float x)
{
    uint32_t b;
    memcpy(&b, &x, sizeof b);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
float spm_unkey(uint32_t k)
{
    const uint32_t b = (k >> 31) ? k ^ 0x80000000u : ~k;
    float x;
    memcpy(&x, &b, sizeof x);
    return x;
}
static uint32_t spm_hkey(float h) { return isfinite(h) ? spm_key(h) : SPM_INF; }   /* not passable: the key of +inf */

/* is vertex o a source?  (ij: count seed vertices, SPM_SEEDS only; checked by the callers) */
static void spm_sources(uint8_t *src, uint32_t n, int mode, const uint32_t *ij, uint32_t count)
{
    memset(src, 0, (size_t)n * n);
    if (mode == SPM_EDGES) {
        for (uint32_t a = 0; a < n; ++a) src[a] = src[(size_t)(n - 1u) * n + a] = src[(size_t)a * n] = src[(size_t)a * n + (n - 1u)] = 1;
    } else
        for (uint32_t k = 0; k < count; ++k) src[(size_t)ij[2u * k + 1u] * n + ij[2u * k]] = 1;
}
static int spm_bad(uint32_t n, int mode, const uint32_t *ij, uint32_t count)
{
    if (n < 2u || (mode != SPM_EDGES && mode != SPM_SEEDS)) return 1;
    if (mode == SPM_SEEDS)
        for (uint32_t k = 0; k < count; ++k)
            if (ij[2u * k] >= n || ij[2u * k + 1u] >= n) return 1;
    return 0;
}

/* spill, sd = spill - h and sink = (sd finite ? sd : 0) from the keys w */
static int64_t spm_finish(float *spill, float *sd, float *sink, const uint32_t *w, const float *h, size_t nv)
{
    int64_t reached = 0;
    for (size_t k = 0; k < nv; ++k) {
        spill[k] = spm_unkey(w[k]);
        sd[k] = spill[k] - h[k];
        sink[k] = isfinite(sd[k]) ? sd[k] : 0.0f;
        reached += w[k] != SPM_INF;
    }
    return reached;
}

/* ---- the field (contract items 1-5): the search ---- */

typedef struct { uint32_t key, v; } SpmItem;
static void spm_push(SpmItem *heap, size_t *len, SpmItem x)
{
    size_t c = (*len)++;
    while (c > 0) {
        const size_t p = (c - 1u) / 2u;
        if (heap[p].key <= x.key) break;
        heap[c] = heap[p];
        c = p;
    }
    heap[c] = x;
}
static SpmItem spm_pop(SpmItem *heap, size_t *len)
{
    const SpmItem top = heap[0], x = heap[--(*len)];
    size_t p = 0;
    for (;;) {
        size_t c = 2u * p + 1u;
        if (c >= *len) break;
        if (c + 1u < *len && heap[c + 1u].key < heap[c].key) ++c;
        if (x.key <= heap[c].key) break;
        heap[p] = heap[c];
        p = c;
    }
    heap[p] = x;
    return top;
}

/* h (n x n, row j = z index, column i = x index) and the sources -> spill, sd, sink (all n x n).  Returns the number of reached
 * vertices, -1 on a bad argument. */
int64_t spm_field(float *spill, float *sd, float *sink, const float *h, uint32_t n, int mode, const uint32_t *ij, uint32_t count)
{
    if (spm_bad(n, mode, ij, count)) return -1;
    const size_t nv = (size_t)n * n;
    uint32_t *w = (uint32_t *)malloc(nv * sizeof *w);
    uint8_t *state = (uint8_t *)malloc(nv);                    /* first the sources, then 2: final */
    SpmItem *heap = (SpmItem *)malloc((4u * nv + 4u) * sizeof *heap);   /* every vertex is pushed at most once per neighbour, or as a source */
    if (!w || !state || !heap) { free(w); free(state); free(heap); return -1; }
    spm_sources(state, n, mode, ij, count);
    size_t len = 0;
    for (size_t k = 0; k < nv; ++k) {
        const uint32_t hk = spm_hkey(h[k]);
        w[k] = SPM_INF;
        if (state[k] && hk != SPM_INF) { w[k] = hk; spm_push(heap, &len, (SpmItem){ hk, (uint32_t)k }); }
        state[k] = 0;
    }
    while (len) {
        const SpmItem it = spm_pop(heap, &len);
        if (state[it.v] == 2 || it.key != w[it.v]) continue;
        state[it.v] = 2;
        const uint32_t i = it.v % n, j = it.v / n;
        const size_t nb[4] = { (size_t)it.v - 1u, (size_t)it.v + 1u, (size_t)it.v - n, (size_t)it.v + n };
        const int ok[4] = { i > 0u, i + 1u < n, j > 0u, j + 1u < n };
        for (int d = 0; d < 4; ++d) {
            if (!ok[d] || state[nb[d]] == 2) continue;
            const uint32_t hk = spm_hkey(h[nb[d]]);
            if (hk == SPM_INF) continue;
            const uint32_t k = hk > it.key ? hk : it.key;
            if (k < w[nb[d]]) { w[nb[d]] = k; spm_push(heap, &len, (SpmItem){ k, (uint32_t)nb[d] }); }
        }
    }
    const int64_t reached = spm_finish(spill, sd, sink, w, h, nv);
    free(w); free(state); free(heap);
    return reached;
}

/* ---- the launches of k_spill_pass, emulated with Jacobi halos ---- */

#define SPM_RELAX(o_, x_) do { const uint32_t m_ = w[o_] < (x_) ? w[o_] : (x_), nv_ = hk[o_] > m_ ? hk[o_] : m_; \
                               if (nv_ != w[o_]) { w[o_] = nv_; moved = 1; } } while (0)

/* In every pass each tile takes the facing column and row its four neighbours held BEFORE the pass, then runs to its own fixpoint
 * (raster sweeps of the relaxation, forwards and backwards, until one changes nothing).  Returns the passes up to and including the
 * first that changed nothing; changed_tiles[p] (p < cap): the tiles pass p + 1 changed.  The kernels may see a neighbour's stores of
 * the same launch, so they never need more passes than this. */
int64_t spm_tile_passes(float *spill, float *sd, float *sink, const float *h, uint32_t n, int mode, const uint32_t *ij, uint32_t count, uint32_t tile,
                        uint32_t *changed_tiles, uint32_t cap)
{
    if (spm_bad(n, mode, ij, count) || tile < 1u) return -1;
    const size_t nv = (size_t)n * n;
    uint32_t *w = (uint32_t *)malloc(nv * sizeof *w), *hk = (uint32_t *)malloc(nv * sizeof *hk), *old = (uint32_t *)malloc(nv * sizeof *old);
    uint8_t *src = (uint8_t *)malloc(nv);
    if (!w || !hk || !old || !src) { free(w); free(hk); free(old); free(src); return -1; }
    spm_sources(src, n, mode, ij, count);
    for (size_t k = 0; k < nv; ++k) {
        hk[k] = spm_hkey(h[k]);
        w[k] = src[k] ? hk[k] : SPM_INF;
    }
    const uint32_t nt = (n + tile - 1u) / tile;
    int64_t passes = 0;
    for (;;) {
        memcpy(old, w, nv * sizeof *w);
        uint32_t changed = 0;
        for (uint32_t ty = 0; ty < nt; ++ty)
            for (uint32_t tx = 0; tx < nt; ++tx) {
                const uint32_t i0 = tx * tile, j0 = ty * tile, i1 = i0 + tile < n ? i0 + tile : n, j1 = j0 + tile < n ? j0 + tile : n;
                int moved = 0, fell = 0;
                for (uint32_t j = j0; j < j1; ++j) {
                    if (i0 > 0u) SPM_RELAX((size_t)j * n + i0, old[(size_t)j * n + i0 - 1u]);
                    if (i1 < n) SPM_RELAX((size_t)j * n + i1 - 1u, old[(size_t)j * n + i1]);
                }
                for (uint32_t i = i0; i < i1; ++i) {
                    if (j0 > 0u) SPM_RELAX((size_t)j0 * n + i, old[(size_t)(j0 - 1u) * n + i]);
                    if (j1 < n) SPM_RELAX((size_t)(j1 - 1u) * n + i, old[(size_t)j1 * n + i]);
                }
                fell = moved;
                do {
                    moved = 0;
                    for (uint32_t j = j0; j < j1; ++j)
                        for (uint32_t i = i0; i < i1; ++i) {
                            const size_t o = (size_t)j * n + i;
                            if (i > i0) SPM_RELAX(o, w[o - 1u]);
                            if (j > j0) SPM_RELAX(o, w[o - n]);
                        }
                    for (uint32_t j = j1; j-- > j0;)
                        for (uint32_t i = i1; i-- > i0;) {
                            const size_t o = (size_t)j * n + i;
                            if (i + 1u < i1) SPM_RELAX(o, w[o + 1u]);
                            if (j + 1u < j1) SPM_RELAX(o, w[o + n]);
                        }
                    fell |= moved;
                } while (moved);
                changed += fell != 0;
            }
        if ((uint64_t)passes < cap) changed_tiles[passes] = changed;
        ++passes;
        if (!changed) break;
    }
    spm_finish(spill, sd, sink, w, h, nv);
    free(w); free(hk); free(old); free(src);
    return passes;
}
#undef SPM_RELAX

/* ---- the tint pass (contract item 6) ---- */

/* rgba (H x W x 4, the frame without the tint) -> the frame with it, in place.  dval (H x W): the pixel's interpolated depth d where the
 * pass blends (d > 0), -1 where it leaves the pixel.  sd: n x n as spm_field gives it. */
int spm_frame(uint8_t *rgba, float *dval, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw, uint32_t th,
              uint32_t grid, const float *sd, uint32_t shallow_rgba, uint32_t deep_rgba, float depth_full)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const size_t o = (size_t)py * W + px;
            dval[o] = -1.0f;
            const uint32_t id = vis[o];
            if (id == 0u) continue;
            const uint32_t prim = id - 1u, cell = prim >> 1, odd = prim & 1u;
            const uint32_t j = cell / F.nm1, i = cell - j * F.nm1;
            const uint32_t vi[3] = { odd ? i + 1u : i, i, i + 1u }, vj[3] = { j, j + 1u, odd ? j + 1u : j };
            float l[3];
            int zero = 1, finite = 1;
            for (int k = 0; k < 3; ++k) {
                l[k] = sd[(size_t)vj[k] * F.n + vi[k]];
                zero &= l[k] == 0.0f;
                finite &= isfinite(l[k]) != 0;
            }
            if (!finite || zero) continue;
            AVert v[3], poly[8];
            for (int k = 0; k < 3; ++k) { v[k] = attr_vertex(&F, vi[k], vj[k]); v[k].a[0] = l[k]; }   /* sd in the place of h */
            const int np = clip_attr(v, poly);
            float d = 0.0f;
            for (int f = 1; f + 1 < np; ++f) {
                float q[3];
                if (!tri_weights(&F, &poly[0].c, &poly[f].c, &poly[f + 1].c, (int32_t)px, (int32_t)py, q)) continue;
                const float rQ = 1.0f / ((q[0] + q[1]) + q[2]);
                d = fmaf(q[2], poly[f + 1].a[0], fmaf(q[1], poly[f].a[0], q[0] * poly[0].a[0])) * rQ;
            }
            if (!(d > 0.0f)) continue;
            const float s = fminf(d / depth_full, 1.0f);
            float c[3];
            for (int k = 0; k < 3; ++k) c[k] = ovm_decode(rgba[4 * o + k]);
            const int sh = vsm_blend(c, shallow_rgba, 1.0f - s);
            const int dp = vsm_blend(c, deep_rgba, s);
            if (!sh && !dp) continue;
            dval[o] = d;
            for (int k = 0; k < 3; ++k) rgba[4 * o + k] = (uint8_t)ovm_encode(c[k]);
            rgba[4 * o + 3] = 255;
        }
    frame_free(&F);
    return 0;
}

/* flood_model.c -- CPU model of the flood analysis, the contract the gfx950 kernels of vulkan_forge_amd/csrc/vf_flood.h
 * (k_flood_wet / _seed / _pass / _depth / _tint) are held to bit for bit.  Written from the contract: the flooded set is a
 * breadth-first search over the 4-neighbourhood from the sources, with no tiles and no masks; the tinted frame takes a frame and its
 * visibility ids, interpolates wd = level - h of the three vertices of every covered pixel with the geometry-buffer model's weights
 * (clip, fan, last covering piece) and blends the two colours as the viewshed model blends its tints.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC flood_model.c -o libfdmodel.so -lm     (flood_model.py does this)
 */
#include "../viewshed_model/viewshed_model.c"

enum { FDM_EVERYWHERE = 0, FDM_EDGES = 1, FDM_SEEDS = 2 };

/* ---- the field (contract items 1-4) ---- */

/* h (n x n, row j = z index, column i = x index; before exaggeration), the level and the sources -> wet (1: wet-able), flooded
 * (1: flooded), wd = level - h and depth = flooded ? wd : 0, all n x n.  ij: count seed vertices (i, j), mode FDM_SEEDS only.
 * Returns the number of flooded vertices, -1 on a bad argument. */
int64_t fdm_field(uint8_t *wet, uint8_t *flooded, float *wd, float *depth, const float *h, uint32_t n, float level, int mode, const uint32_t *ij,
                  uint32_t count)
{
    if (n < 2u || mode < FDM_EVERYWHERE || mode > FDM_SEEDS) return -1;
    const size_t nv = (size_t)n * n;
    for (size_t k = 0; k < nv; ++k) {
        wet[k] = isfinite(h[k]) && h[k] < level;
        wd[k] = level - h[k];
        flooded[k] = 0;
    }
    uint32_t *queue = (uint32_t *)malloc(nv * sizeof *queue);
    if (!queue) return -1;
    size_t head = 0, tail = 0;
#define FDM_SOURCE(o) do { const size_t o_ = (o); if (wet[o_] && !flooded[o_]) { flooded[o_] = 1; queue[tail++] = (uint32_t)o_; } } while (0)
    if (mode == FDM_EVERYWHERE) {
        for (size_t k = 0; k < nv; ++k) FDM_SOURCE(k);
    } else if (mode == FDM_EDGES) {
        for (uint32_t a = 0; a < n; ++a) {
            FDM_SOURCE((size_t)a); FDM_SOURCE((size_t)(n - 1u) * n + a); FDM_SOURCE((size_t)a * n); FDM_SOURCE((size_t)a * n + (n - 1u));
        }
    } else {
        for (uint32_t k = 0; k < count; ++k) {
            if (ij[2u * k] >= n || ij[2u * k + 1u] >= n) { free(queue); return -1; }
            FDM_SOURCE((size_t)ij[2u * k + 1u] * n + ij[2u * k]);
        }
    }
    while (head < tail) {
        const uint32_t o = queue[head++], i = o % n, j = o / n;
        if (i > 0u) FDM_SOURCE((size_t)o - 1u);
        if (i + 1u < n) FDM_SOURCE((size_t)o + 1u);
        if (j > 0u) FDM_SOURCE((size_t)o - n);
        if (j + 1u < n) FDM_SOURCE((size_t)o + n);
    }
#undef FDM_SOURCE
    free(queue);
    for (size_t k = 0; k < nv; ++k) depth[k] = flooded[k] ? wd[k] : 0.0f;
    return (int64_t)tail;
}

/* the 4-connected components of `wet` inside tile x tile squares of the grid -> labels (n x n): 0 where not wet, else a number that
 * only the vertices of one component of one tile share.  What the emulation of the tile passes (flood_model.py) runs a tile to its
 * own fixpoint with.  Returns the number of components. */
int64_t fdm_label_tiles(int32_t *labels, const uint8_t *wet, uint32_t n, uint32_t tile)
{
    if (n < 1u || tile < 1u) return -1;
    const size_t nv = (size_t)n * n;
    memset(labels, 0, nv * sizeof *labels);
    uint32_t *queue = (uint32_t *)malloc(nv * sizeof *queue);
    if (!queue) return -1;
    int32_t next = 0;
    for (size_t s = 0; s < nv; ++s) {
        if (!wet[s] || labels[s]) continue;
        size_t head = 0, tail = 0;
        labels[s] = ++next;
        queue[tail++] = (uint32_t)s;
        while (head < tail) {
            const uint32_t o = queue[head++], i = o % n, j = o / n;
#define FDM_JOIN(o2) do { const size_t o_ = (o2); if (wet[o_] && !labels[o_]) { labels[o_] = next; queue[tail++] = (uint32_t)o_; } } while (0)
            if (i % tile) FDM_JOIN((size_t)o - 1u);
            if ((i + 1u) % tile && i + 1u < n) FDM_JOIN((size_t)o + 1u);
            if (j % tile) FDM_JOIN((size_t)o - n);
            if ((j + 1u) % tile && j + 1u < n) FDM_JOIN((size_t)o + n);
#undef FDM_JOIN
        }
    }
    free(queue);
    return next;
}

/* ---- the tint pass (contract item 5) ---- */

/* rgba (H x W x 4, the frame without water) -> the frame with it, in place.  dval (H x W): the pixel's interpolated depth d where the
 * pass blends (d > 0), -1 where it leaves the pixel.  flooded, wd: n x n as fdm_field gives them. */
int fdm_frame(uint8_t *rgba, float *dval, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw, uint32_t th,
              uint32_t grid, const uint8_t *flooded, const float *wd, uint32_t shallow_rgba, uint32_t deep_rgba, float depth_full)
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
            int any = 0, finite = 1;
            for (int k = 0; k < 3; ++k) {
                const size_t v = (size_t)vj[k] * F.n + vi[k];
                l[k] = wd[v];
                any |= flooded[v] != 0;
                finite &= isfinite(l[k]) != 0;
            }
            if (!any || !finite) continue;
            AVert v[3], poly[8];
            for (int k = 0; k < 3; ++k) { v[k] = attr_vertex(&F, vi[k], vj[k]); v[k].a[0] = l[k]; }   /* wd in the place of h */
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

/* polygon_model.c -- CPU model of the polygon fill pass, the contract the gfx950 kernels of
 * vulkan_forge_amd/csrc/vf_overlay.h (k_pg_*, and the fill walk of k_ov_composite) are held to bit for bit.  Written from the contract,
 * not from the kernels' structure: no bins, no backdrop masks -- a fill feature's parity at a pixel counts every crossing of its row
 * right of the pixel, and its distance is the minimum over every edge that can come within 0.5 px of it (beyond that the coverage
 * has saturated, as for the points of 4b).  Points and lines are the overlay model's own code (included below), so layers mix.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC polygon_model.c -o libpgmodel.so -lm     (polygon_model.py does this)
 */
#include "../overlay_model/overlay_model.c"

/* one screen edge of a fill: start, direction, 1 / |e|^2 (0 if zero), ex / ey (0 if horizontal), x and y range */
typedef struct { float x0, y0, ex, ey, il2, s, xmin, xmax, ymin, ymax; } PEdge;

static int frame_init(Frame *F, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw, uint32_t th, uint32_t grid)
{
    tables();
    memset(F, 0, sizeof *F);
    F->view = u; F->proj = u + 16;
    F->spacing = fmaxf(u[36], 1e-8f); F->exag = u[38];
    F->hw = 0.5f * (float)W; F->hh = 0.5f * (float)H;
    F->n = grid < 2 ? 2 : grid; F->nm1 = F->n - 1;
    F->step = (2.0f * 1.5f) / ((float)F->n - 1.0f);
    F->W = W; F->H = H; F->tw = tw; F->tex = tex;
    F->sinx = malloc(F->n * sizeof(float)); F->cosz = malloc(F->n * sizeof(float));
    F->txi = malloc(F->n * sizeof(int32_t)); F->tyj = malloc(F->n * sizeof(int32_t));
    if (!F->sinx || !F->cosz || !F->txi || !F->tyj) return -1;
    const float nm1f = (float)F->n - 1.0f;
    for (uint32_t i = 0; i < F->n; ++i) {
        const float x = -1.5f + (float)i * F->step, uvc = (float)i / nm1f;
        F->sinx[i] = det_sin(x * 1.3f);
        F->cosz[i] = det_cos(x * 1.1f);
        int tx = (int)floorf(uvc * (float)tw), ty = (int)floorf(uvc * (float)th);
        F->txi[i] = tx < 0 ? 0 : (tx > (int)tw - 1 ? (int)tw - 1 : tx);
        F->tyj[i] = ty < 0 ? 0 : (ty > (int)th - 1 ? (int)th - 1 : ty);
    }
    return 0;
}

static void frame_free(Frame *F) { free(F->sinx); free(F->cosz); free(F->txi); free(F->tyj); }

/* the near plane (z >= 0) crossing of clip-space segment in -> out (4b's formula) */
static void cross_near(const float in[4], const float out[4], float r[4])
{
    const float di = in[2], dou = out[2];
    const float t = di / (di - dou);
    for (int k = 0; k < 4; ++k) r[k] = fmaf(t, out[k] - in[k], in[k]);
}

static int to_screen(const Frame *F, const float c[4], float *sx, float *sy)
{
    if (!(c[3] > 0.0f)) return 0;
    const float rw = 1.0f / c[3];
    *sx = fmaf(c[0] * rw, F->hw, F->hw);
    *sy = fmaf(-(c[1] * rw), F->hh, F->hh);
    return isfinite(*sx) && isfinite(*sy);
}

static void add_edge(const Frame *F, const float a[4], const float b[4], PEdge *E, uint32_t *ne)
{
    float ax, ay, bx, by;
    if (!to_screen(F, a, &ax, &ay) || !to_screen(F, b, &bx, &by)) return;
    PEdge e;
    e.x0 = ax; e.y0 = ay; e.ex = bx - ax; e.ey = by - ay;
    const float l2 = e.ex * e.ex + e.ey * e.ey;
    e.il2 = l2 > 0.0f ? 1.0f / l2 : 0.0f;
    e.s = e.ey != 0.0f ? e.ex / e.ey : 0.0f;
    e.xmin = fminf(ax, bx); e.xmax = fmaxf(ax, bx); e.ymin = fminf(ay, by); e.ymax = fmaxf(ay, by);
    E[(*ne)++] = e;
}

/* one ring's screen edge set: drape, transform, Sutherland-Hodgman against z >= 0 (the kept part of every edge; for every exit point
 * a closing segment along the plane to the next entry point in ring order), viewport.  E has room for 2 nv edges. */
static int ring_edges(const Frame *F, const float *xyz, uint32_t nv, int drape, PEdge *E, uint32_t *ne)
{
    float (*c)[4] = malloc((size_t)nv * sizeof *c);
    if (!c) return -1;
    for (uint32_t v = 0; v < nv; ++v) to_clip(F, xyz + 3u * v, drape, c[v]);
    for (uint32_t e = 0; e < nv; ++e) {
        const float *a = c[e], *b = c[(e + 1u) % nv];
        const int ain = a[2] >= 0.0f, bin = b[2] >= 0.0f;
        float s0[4], s1[4];
        if (ain || bin) {
            memcpy(s0, a, sizeof s0); memcpy(s1, b, sizeof s1);
            if (!bin) cross_near(a, b, s1);
            else if (!ain) cross_near(b, a, s0);
            add_edge(F, s0, s1, E, ne);
        }
        if (ain && !bin) {
            cross_near(a, b, s0);
            for (uint32_t k = 2; k <= nv; ++k) {
                const uint32_t j = (e + k) % nv;
                if (c[j][2] >= 0.0f) { cross_near(c[j], c[(j + nv - 1u) % nv], s1); add_edge(F, s0, s1, E, ne); break; }
            }
        }
    }
    free(c);
    return 0;
}

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* the edge set of one fill feature (rings r0 .. r1 - 1): *E malloc'ed */
static int feature_edges(const Frame *F, const float *xyz, const uint32_t *ring_offsets, uint32_t r0, uint32_t r1, int drape,
                         PEdge **E, uint32_t *ne)
{
    size_t cap = 0;
    for (uint32_t r = r0; r < r1; ++r) cap += 2u * (size_t)(ring_offsets[r + 1] - ring_offsets[r]);
    *E = malloc((cap ? cap : 1) * sizeof(PEdge));
    *ne = 0;
    if (!*E) return -1;
    for (uint32_t r = r0; r < r1; ++r)
        if (ring_edges(F, xyz + 3u * (size_t)ring_offsets[r], ring_offsets[r + 1] - ring_offsets[r], drape, *E, ne)) return -1;
    return 0;
}

/* coverage of one fill feature: cov[o] for every pixel o of the feature box (written; listed once in list / listed) */
static int fill_cover(const Frame *F, const PEdge *E, uint32_t ne, float *cov, uint32_t *list, uint8_t *listed, uint32_t *nl)
{
    const int W = (int)F->W, H = (int)F->H;
    int fx0 = 1 << 30, fy0 = 1 << 30, fx1 = -(1 << 30), fy1 = -(1 << 30);
    for (uint32_t k = 0; k < ne; ++k) {                  /* the feature box: every edge's extent +-1 px, floored in [-2, n + 2] */
        const PEdge *e = &E[k];
        const int a = (int)floorf(fminf(fmaxf(e->xmin - 1.0f, -2.0f), (float)W + 2.0f));
        const int b = (int)floorf(fminf(fmaxf(e->xmax + 1.0f, -2.0f), (float)W + 2.0f));
        const int c = (int)floorf(fminf(fmaxf(e->ymin - 1.0f, -2.0f), (float)H + 2.0f));
        const int d = (int)floorf(fminf(fmaxf(e->ymax + 1.0f, -2.0f), (float)H + 2.0f));
        if (a < fx0) fx0 = a;
        if (b > fx1) fx1 = b;
        if (c < fy0) fy0 = c;
        if (d > fy1) fy1 = d;
    }
    fx0 = fx0 < 0 ? 0 : fx0; fy0 = fy0 < 0 ? 0 : fy0;
    fx1 = fx1 > W - 1 ? W - 1 : fx1; fy1 = fy1 > H - 1 ? H - 1 : fy1;
    if (fx0 > fx1 || fy0 > fy1) return 0;
    const int bw = fx1 - fx0 + 1, bh = fy1 - fy0 + 1;
    float *d2 = malloc((size_t)bw * bh * sizeof(float));
    uint8_t *flip = calloc((size_t)bw * bh, 1);
    if (!d2 || !flip) return -1;
    for (size_t o = 0; o < (size_t)bw * bh; ++o) d2[o] = INFINITY;
    for (uint32_t k = 0; k < ne; ++k) {
        const PEdge *e = &E[k];
        int px0, px1, py0, py1;
        span(e->xmin - 1.0f, e->xmax + 1.0f, F->W, &px0, &px1);
        span(e->ymin - 1.0f, e->ymax + 1.0f, F->H, &py0, &py1);
        for (int py = py0; py <= py1; ++py) {
            const float qy = (float)py + 0.5f;
            for (int px = px0; px <= px1; ++px) {            /* distance: the pixels within the edge's extent +-1 px */
                const float qx = (float)px + 0.5f;
                const float dx = qx - e->x0, dy = qy - e->y0;
                const float t = fminf(fmaxf((dx * e->ex + dy * e->ey) * e->il2, 0.0f), 1.0f);
                const float rx = dx - t * e->ex, ry = dy - t * e->ey;
                float *m = &d2[(size_t)(py - fy0) * bw + (px - fx0)];
                *m = fminf(*m, rx * rx + ry * ry);
            }
            if (!(e->ymin <= qy && qy < e->ymax)) continue;
            /* parity: the crossing flips every pixel of the row with qx < x_c -- px <= p, marked at p (suffix XOR below) */
            const float xc = fminf(fmaxf(fmaf(qy - e->y0, e->s, e->x0), e->xmin), e->xmax);
            if (!((float)fx0 + 0.5f < xc)) continue;
            int p = (int)floorf(fminf(xc, (float)fx1 + 2.0f));
            p = clampi(p, fx0, fx1);
            while (p < fx1 && (float)(p + 1) + 0.5f < xc) ++p;
            while (!((float)p + 0.5f < xc)) --p;
            flip[(size_t)(py - fy0) * bw + (p - fx0)] ^= 1u;
        }
    }
    for (int y = 0; y < bh; ++y) {
        uint32_t par = 0;
        for (int x = bw - 1; x >= 0; --x) {
            const size_t b = (size_t)y * bw + x;
            par ^= flip[b];
            const float d = sqrtf(d2[b]);
            const float sd = par ? -d : d;
            const size_t o = (size_t)(y + fy0) * F->W + (size_t)(x + fx0);
            cov[o] = fminf(fmaxf(0.5f - sd, 0.0f), 1.0f);
            if (!listed[o]) { listed[o] = 1; list[(*nl)++] = (uint32_t)o; }
        }
    }
    free(d2); free(flip);
    return 0;
}

/* The frame rgba (H x W x 4, sRGB8, composited in place): point / line primitives prims[nprims] (overlay model records, ascending
 * features) and nfill fill features -- feature fill_feature[k], colour fill_rgba[k], drape fill_drape[k], rings fill_rings[k] ..
 * fill_rings[k + 1] - 1 of ring_offsets / xyz -- composited in ascending feature order. */
int pgm_composite(uint8_t *rgba, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw, uint32_t th, uint32_t grid,
                  const OvIn *prims, uint32_t nprims, uint32_t nfill, const uint32_t *fill_feature, const uint32_t *fill_rgba,
                  const uint8_t *fill_drape, const uint32_t *fill_rings, const uint32_t *ring_offsets, const float *xyz)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    const size_t npx = (size_t)W * H;
    float *lin = malloc(npx * 3 * sizeof(float)), *cov = calloc(npx, sizeof(float));
    uint8_t *touched = calloc(npx, 1), *listed = calloc(npx, 1);
    uint32_t *list = malloc(npx * sizeof(uint32_t));
    if (!lin || !cov || !touched || !list || !listed) return -1;
    uint32_t k = 0, f = 0;
    while (k < nprims || f < nfill) {
        uint32_t nl = 0, rgba_f;
        if (f < nfill && (k >= nprims || fill_feature[f] < prims[k].feature)) {
            rgba_f = fill_rgba[f];
            PEdge *E;
            uint32_t ne;
            if (feature_edges(&F, xyz, ring_offsets, fill_rings[f], fill_rings[f + 1], fill_drape[f], &E, &ne)) return -1;
            if (fill_cover(&F, E, ne, cov, list, listed, &nl)) return -1;
            free(E);
            ++f;
        } else {
            const uint32_t feature = prims[k].feature;
            rgba_f = prims[k].rgba;
            for (; k < nprims && prims[k].feature == feature; ++k) {
                Prim p;
                setup(&F, &prims[k], &p);
                for (int py = p.py0; py <= p.py1; ++py)
                    for (int px = p.px0; px <= p.px1; ++px) {
                        const size_t o = (size_t)py * W + (size_t)px;
                        cov[o] = fmaxf(cov[o], cover(&p, (float)px + 0.5f, (float)py + 0.5f));
                        if (!listed[o]) { listed[o] = 1; list[nl++] = (uint32_t)o; }
                    }
            }
        }
        const float A = (float)(rgba_f >> 24) / 255.0f;
        for (uint32_t m = 0; m < nl; ++m) {
            const size_t o = list[m];
            listed[o] = 0;
            if (cov[o] > 0.0f) {
                if (!touched[o]) { for (int c = 0; c < 3; ++c) lin[3 * o + c] = g_dec[rgba[4 * o + c]]; touched[o] = 1; }
                const float a = cov[o] * A;
                for (int c = 0; c < 3; ++c) {
                    const float s = g_dec[(rgba_f >> (8 * c)) & 255u];
                    lin[3 * o + c] = s * a + lin[3 * o + c] * (1.0f - a);
                }
            }
            cov[o] = 0.0f;
        }
    }
    for (size_t o = 0; o < npx; ++o)
        if (touched[o]) {
            for (int c = 0; c < 3; ++c) rgba[4 * o + c] = (uint8_t)ovm_encode(lin[3 * o + c]);
            rgba[4 * o + 3] = 255;
        }
    frame_free(&F); free(lin); free(cov); free(touched); free(list); free(listed);
    return 0;
}

/* one fill feature's coverage (W x H floats, 0 outside its box) -- for the model's own tests */
int pgm_fill_coverage(float *cov, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw, uint32_t th, uint32_t grid,
                      uint32_t nrings, const uint32_t *ring_offsets, const float *xyz, int drape)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    const size_t npx = (size_t)W * H;
    uint32_t *list = malloc(npx * sizeof(uint32_t)), nl = 0, ne;
    uint8_t *listed = calloc(npx, 1);
    PEdge *E;
    memset(cov, 0, npx * sizeof(float));
    if (!list || !listed || feature_edges(&F, xyz, ring_offsets, 0, nrings, drape, &E, &ne)) return -1;
    const int rc = fill_cover(&F, E, ne, cov, list, listed, &nl);
    free(E); free(list); free(listed); frame_free(&F);
    return rc;
}

/* one ring's screen edge set, 10 floats per edge (x0, y0, ex, ey, 1/|e|^2, ex/ey, x min / max, y min / max); returns the count */
int pgm_ring_edges(float *out, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw, uint32_t th, uint32_t grid,
                   const float *xyz, uint32_t nv, int drape)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    uint32_t ne = 0;
    if (ring_edges(&F, xyz, nv, drape, (PEdge *)out, &ne)) return -1;
    frame_free(&F);
    return (int)ne;
}

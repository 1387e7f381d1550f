/* occlusion_model.c -- CPU model of overlay occlusion, the contract the gfx950 kernels of
 * vulkan_forge_amd/csrc/vf_overlay.h (k_ov_setup's depth values, k_ov_composite_occlude) and terrain_rw (vf_visible.h) are held to
 * bit for bit.  Written from the contract: the terrain's 1/w at every pixel comes from the visibility ids and a restatement of the
 * vertex stage (vertex_shader, snap_vertex), the clipper and the coverage rule; every primitive takes the generic path (clip, fan,
 * last covering piece), which for an unclipped primitive is the same arithmetic as the kernels' vertex-record path.  Points, lines
 * and polygon fills are the overlay and polygon models' own code (included below); only the occlusion test is new.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC occlusion_model.c -o libocmodel.so -lm     (occlusion_model.py does this)
 */
#include "../polygon_model/polygon_model.c"

enum { OCCLUDE = 32 };

/* ---- the terrain's vertex stage (vf_device.h vertex_shader, snap_vertex) ---- */
typedef struct { float x, y, z, w; } CVert;

static CVert terrain_vertex(const Frame *F, uint32_t i, uint32_t j)
{
    const float x = -1.5f + (float)i * F->step, z = -1.5f + (float)j * F->step;
    const float h = height_at(F, i, j);
    float vp[4], c[4];
    mat_vec(F->view, x * F->spacing, h * F->exag, z * F->spacing, 1.0f, vp);
    mat_vec(F->proj, vp[0], vp[1], vp[2], vp[3], c);
    CVert v = { c[0], c[1], c[2], c[3] };
    return v;
}

static int snap(const Frame *F, const CVert *v, int32_t *X, int32_t *Y, float *rw)
{
    if (!(v->w > 0.0f)) return 0;
    *rw = 1.0f / v->w;
    float xf = fmaf(v->x * *rw, F->hw, F->hw);
    float yf = fmaf(-(v->y * *rw), F->hh, F->hh);
    if (!isfinite(xf) || !isfinite(yf)) return 0;
    xf = fminf(fmaxf(xf, -4194304.0f), 4194304.0f);
    yf = fminf(fmaxf(yf, -4194304.0f), 4194304.0f);
    *X = (int32_t)rintf(xf * 256.0f);
    *Y = (int32_t)rintf(yf * 256.0f);
    return 1;
}

static float plane_d(const CVert *v, int plane) { return plane == 0 ? v->z : v->w - v->z; }

/* Sutherland-Hodgman against z >= 0 then z <= w, crossings from the inside vertex outwards */
static int clip_tri(const CVert v[3], CVert poly[8])
{
    for (int k = 0; k < 3; ++k)
        if (!(isfinite(v[k].x) && isfinite(v[k].y) && isfinite(v[k].z) && isfinite(v[k].w))) return 0;
    int out_near = 0, out_far = 0;
    for (int k = 0; k < 3; ++k) { out_near += v[k].z < 0.0f; out_far += v[k].z > v[k].w; }
    if (out_near == 3 || out_far == 3) return 0;
    for (int k = 0; k < 3; ++k) poly[k] = v[k];
    if (out_near == 0 && out_far == 0) return 3;
    CVert tmp[8];
    int n = 3;
    for (int plane = 0; plane < 2; ++plane) {
        int m = 0;
        for (int k = 0; k < n; ++k) {
            const CVert *cur = &poly[k], *nxt = &poly[(k + 1) % n];
            const float dc = plane_d(cur, plane), dn = plane_d(nxt, plane);
            const int cin = dc >= 0.0f, nin = dn >= 0.0f;
            if (cin) tmp[m++] = *cur;
            if (cin != nin) {
                const CVert *in = cin ? cur : nxt, *ou = cin ? nxt : cur;
                const float di = cin ? dc : dn, dou = cin ? dn : dc;
                const float t = di / (di - dou);
                CVert r = { fmaf(t, ou->x - in->x, in->x), fmaf(t, ou->y - in->y, in->y), fmaf(t, ou->z - in->z, in->z),
                            fmaf(t, ou->w - in->w, in->w) };
                tmp[m++] = r;
            }
        }
        n = m;
        for (int k = 0; k < n; ++k) poly[k] = tmp[k];
        if (n < 3) return 0;
    }
    return n;
}

/* Q of one (sub-)triangle at pixel (px, py): 1 and *Q if it is front-facing and covers the pixel centre (top-left rule) */
static int tri_q(const Frame *F, const CVert *a, const CVert *b, const CVert *c, int32_t px, int32_t py, float *Q)
{
    int32_t X[3], Y[3];
    float rw[3];
    const CVert *v[3] = { a, b, c };
    for (int k = 0; k < 3; ++k)
        if (!snap(F, v[k], &X[k], &Y[k], &rw[k])) return 0;
    const int64_t area2 = (int64_t)(X[1] - X[0]) * (Y[2] - Y[0]) - (int64_t)(Y[1] - Y[0]) * (X[2] - X[0]);
    if (area2 >= 0) return 0;
    const int64_t Px = (int64_t)px * 256 + 128, Py = (int64_t)py * 256 + 128;
    int64_t e[3];
    int tl[3];
    for (int k = 0; k < 3; ++k) {
        const int s = (k + 1) % 3, t = (k + 2) % 3;          /* edge s -> t, opposite vertex k */
        e[k] = -((int64_t)(X[t] - X[s]) * (Py - Y[s]) - (int64_t)(Y[t] - Y[s]) * (Px - X[s]));
        const int32_t ea = Y[t] - Y[s], eb = -(X[t] - X[s]);
        tl[k] = ea > 0 || (ea == 0 && eb > 0);
    }
    for (int k = 0; k < 3; ++k)
        if (!(e[k] > 0 || (e[k] == 0 && tl[k]))) return 0;
    const float fA = (float)(-area2);
    const float l0 = (float)e[0] / fA, l1 = (float)e[1] / fA, l2 = (float)e[2] / fA;
    const float q0 = l0 * rw[0], q1 = l1 * rw[1], q2 = l2 * rw[2];
    *Q = (q0 + q1) + q2;
    return 1;
}

/* the terrain's depth Q at pixel (px, py) with visibility id (0: background, hides nothing) */
static float terrain_q(const Frame *F, uint32_t id, int32_t px, int32_t py)
{
    if (id == 0u) return 0.0f;
    const uint32_t prim = id - 1u, cell = prim >> 1, odd = prim & 1u;
    const uint32_t j = cell / F->nm1, i = cell - j * F->nm1;
    /* indices [a,c,b, b,c,d]: even = (a, c, b), odd = (b, c, d) */
    CVert v[3] = { terrain_vertex(F, odd ? i + 1u : i, j), terrain_vertex(F, i, j + 1u), terrain_vertex(F, i + 1u, odd ? j + 1u : j) };
    CVert poly[8];
    const int np = clip_tri(v, poly);
    float Q = 0.0f, q;
    for (int f = 1; f + 1 < np; ++f)                            /* the last covering piece wins */
        if (tri_q(F, &poly[0], &poly[f], &poly[f + 1], px, py, &q)) Q = q;
    return Q;
}

/* the 1/w of a point's centre or a segment's two ends after clipping (0: the primitive is not drawn) */
static void prim_rw(const Frame *F, const OvIn *q, float *rwa, float *rwb)
{
    *rwa = *rwb = 0.0f;
    const int drape = (q->flags & DRAPE) != 0;
    float a[4], b[4];
    to_clip(F, q->p0, drape, a);
    if ((q->flags & KIND) != SEGMENT) {
        if (finite4(a) && a[3] > 0.0f && !(a[2] < 0.0f) && !(a[2] > a[3])) *rwa = *rwb = 1.0f / a[3];
        return;
    }
    to_clip(F, q->p1, drape, b);
    if (!finite4(a) || !finite4(b)) return;
    for (int plane = 0; plane < 2; ++plane) {
        const float da = plane == 0 ? a[2] : a[3] - a[2], db = plane == 0 ? b[2] : b[3] - b[2];
        const int ain = da >= 0.0f, bin = db >= 0.0f;
        if (!ain && !bin) return;
        if (ain && bin) continue;
        float *in = ain ? a : b, *ou = ain ? b : a;
        const float di = ain ? da : db, dou = ain ? db : da;
        const float t = di / (di - dou);
        float r[4];
        for (int k = 0; k < 4; ++k) r[k] = fmaf(t, ou[k] - in[k], in[k]);
        memcpy(ou, r, sizeof r);
    }
    if (!(a[3] > 0.0f && b[3] > 0.0f)) return;
    *rwa = 1.0f / a[3];
    *rwb = 1.0f / b[3];
}

/* pgm_composite with the visibility ids vis (H x W) and the occlusion test of DESIGN.md 4d; the same arguments otherwise */
int ocm_composite(uint8_t *rgba, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw, uint32_t th,
                  uint32_t grid, const OvIn *prims, uint32_t nprims, uint32_t nfill, const uint32_t *fill_feature, const uint32_t *fill_rgba,
                  const uint8_t *fill_drape, const uint32_t *fill_rings, const uint32_t *ring_offsets, const float *xyz)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    const size_t npx = (size_t)W * H;
    float *lin = malloc(npx * 3 * sizeof(float)), *cov = calloc(npx, sizeof(float)), *Q = malloc(npx * sizeof(float));
    uint8_t *touched = calloc(npx, 1), *listed = calloc(npx, 1);
    uint32_t *list = malloc(npx * sizeof(uint32_t));
    if (!lin || !cov || !Q || !touched || !list || !listed) return -1;
    int any = 0;
    for (uint32_t k = 0; k < nprims; ++k) any |= (prims[k].flags & OCCLUDE) != 0;
    for (uint32_t py = 0; py < H && any; ++py)
        for (uint32_t px = 0; px < W; ++px) Q[(size_t)py * W + px] = terrain_q(&F, vis[(size_t)py * W + px], (int32_t)px, (int32_t)py);
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
                const int occl = (prims[k].flags & OCCLUDE) != 0;
                float kb, rwa = 0.0f, rwb = 0.0f;
                memcpy(&kb, &prims[k].pad[0], sizeof kb);
                if (occl) prim_rw(&F, &prims[k], &rwa, &rwb);
                const float drw = rwb - rwa;
                for (int py = p.py0; py <= p.py1; ++py)
                    for (int px = p.px0; px <= p.px1; ++px) {
                        const size_t o = (size_t)py * W + (size_t)px;
                        const float qx = (float)px + 0.5f, qy = (float)py + 0.5f;
                        float c = cover(&p, qx, qy);
                        if (occl && c > 0.0f) {
                            float rw = rwa;
                            if (p.kind == SEGMENT) {
                                const float uu = (qx - p.g[0]) * p.g[2] + (qy - p.g[1]) * p.g[3];
                                rw = fmaf(fminf(fmaxf(uu / p.h[0], 0.0f), 1.0f), drw, rwa);
                            }
                            if (Q[o] > rw * kb) c = 0.0f;
                        }
                        cov[o] = fmaxf(cov[o], c);
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
    frame_free(&F); free(lin); free(cov); free(Q); free(touched); free(list); free(listed);
    return 0;
}

/* the terrain's depth Q of every pixel (H x W floats) from its visibility ids -- for the model's own tests, and for whether a pixel's
 * primitive needed clipping (*clipped, H x W bytes, may be NULL: 1 where the visible primitive has a vertex outside 0 <= z <= w) */
int ocm_terrain_q(float *Q, uint8_t *clipped, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw,
                  uint32_t th, uint32_t grid)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const size_t o = (size_t)py * W + px;
            Q[o] = terrain_q(&F, vis[o], (int32_t)px, (int32_t)py);
            if (!clipped) continue;
            clipped[o] = 0;
            if (!vis[o]) continue;
            const uint32_t prim = vis[o] - 1u, cell = prim >> 1, odd = prim & 1u;
            const uint32_t j = cell / F.nm1, i = cell - j * F.nm1;
            const CVert v[3] = { terrain_vertex(&F, odd ? i + 1u : i, j), terrain_vertex(&F, i, j + 1u), terrain_vertex(&F, i + 1u, odd ? j + 1u : j) };
            for (int m = 0; m < 3; ++m) clipped[o] |= v[m].z < 0.0f || v[m].z > v[m].w;
        }
    frame_free(&F);
    return 0;
}

/* overlay_haze_model.c -- CPU model of hazed overlay layers, the contract the gfx950 kernels of
 * vulkan_forge_amd/csrc/vf_overlay_haze.h (k_ov_haze_setup, k_ov_composite_haze) are held to bit for bit.  Written from the contract:
 * points, lines, polygon fills and the occlusion test are the overlay, polygon and occlusion models' own code (included below); new
 * are the depth and height of a hazed primitive at a pixel (item 1), the opacity (item 2: the haze contract's det_exp, g and alpha,
 * restated here because haze_model.c brings a frame set-up of its own that cannot share a translation unit with the occlusion model's;
 * tests/test_overlay_haze_model.py holds the restatement equal to haze_model's bit for bit), the primitive that speaks for a feature
 * (item 3) and the blend (item 4).
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC overlay_haze_model.c -o libohmodel.so -lm     (overlay_haze_model.py does this)
 *
 * Every float operation is a binary32 one in the order written (-ffp-contract=off; fmaf only where written). */
#include "../occlusion_model/occlusion_model.c"

enum { HAZE = 64 };

typedef struct { float density, start, falloff, base, max_opacity, eye_y; uint32_t rgba; } HazeP;

/* ---- DESIGN.md 4q items 8, 3, 1, 2, 5, restated ---- */
static float oh_det_exp(float x)
{
    const float n = rintf(x * 1.44269504088896341f);
    float r = fmaf(-n, 0.693359375f, x);
    r = fmaf(-n, -2.12194440e-4f, r);
    float p = fmaf(r, 1.9875691500e-4f, 1.3981999507e-3f);
    p = fmaf(r, p, 8.3334519073e-3f);
    p = fmaf(r, p, 4.1665795894e-2f);
    p = fmaf(r, p, 1.6666665459e-1f);
    p = fmaf(r, p, 5.0000001201e-1f);
    const float y = fmaf(r * r, p, r) + 1.0f;
    const uint32_t bits = (uint32_t)((int32_t)n + 127) << 23;
    float scale;
    memcpy(&scale, &bits, sizeof scale);
    return y * scale;
}

static float oh_clamp_k(float k) { return fminf(fmaxf(k, -16.0f), 64.0f); }

static float oh_g(const HazeP *Z, float y)
{
    if (!(Z->falloff > 0.0f)) return 1.0f;
    const float k_e = oh_clamp_k((Z->eye_y - Z->base) / Z->falloff), k_p = oh_clamp_k((y - Z->base) / Z->falloff);
    const float s = k_p - k_e;
    const float E_e = oh_det_exp(-k_e);
    if (fabsf(s) < 0.5f) {
        float t = fmaf(s, 2.7557319224e-6f, -2.4801587302e-5f);
        t = fmaf(s, t, 1.9841269841e-4f);
        t = fmaf(s, t, -1.3888888889e-3f);
        t = fmaf(s, t, 8.3333333333e-3f);
        t = fmaf(s, t, -4.1666666667e-2f);
        t = fmaf(s, t, 1.6666666667e-1f);
        t = fmaf(s, t, -0.5f);
        t = fmaf(s, t, 1.0f);
        return E_e * t;
    }
    return (E_e - oh_det_exp(-k_p)) / s;
}

static float oh_alpha(const HazeP *Z, float d, float y)
{
    if (!isfinite(d)) return 0.0f;
    const float l = fmaxf(d - Z->start, 0.0f);
    if (!(l > 0.0f)) return 0.0f;
    const float tau = (Z->density * l) * oh_g(Z, y);
    const float a0 = 1.0f - oh_det_exp(-fminf(tau, 87.0f));
    const float a = fminf(a0, Z->max_opacity) * ((float)(Z->rgba >> 24) / 255.0f);
    return a > 0.0f ? a : 0.0f;
}

static float oh_eye_y(const float *u) { return -fmaf(u[6], u[14], fmaf(u[5], u[13], u[4] * u[12])); }

/* the restated opacity of n (d, y) pairs, for the test that holds it equal to haze_model's */
void ohm_alpha_n(float *out, const float *d, const float *y, uint32_t n, float eye_y, float density, float start, float falloff, float base,
                 float max_opacity, uint32_t alpha8)
{
    const HazeP Z = { density, start, falloff, base, max_opacity, eye_y, alpha8 << 24 };
    for (uint32_t k = 0; k < n; ++k) out[k] = oh_alpha(&Z, d[k], y[k]);
}

/* ---- item 1: the world height that goes into the view matrix, and the side record of a primitive ---- */
static float world_y(const Frame *F, const float p[3], int drape)
{
    float y = p[1];
    if (drape) y = ovm_drape_h(F, p[0], p[2]) * F->exag + p[1];
    return y;
}

/* s = (rw_a, rw_b - rw_a, yq_a or y_c, yq_b - yq_a); all zero: the primitive is not drawn; ends (may be NULL):
 * (rw_a, rw_b, y_a, y_b) after clipping */
static void prim_side(const Frame *F, const OvIn *q, float s[4], float ends[4])
{
    s[0] = s[1] = s[2] = s[3] = 0.0f;
    if (ends) ends[0] = ends[1] = ends[2] = ends[3] = 0.0f;
    const int drape = (q->flags & DRAPE) != 0;
    float a[4], b[4];
    to_clip(F, q->p0, drape, a);
    float ya = world_y(F, q->p0, drape);
    if ((q->flags & KIND) != SEGMENT) {
        if (finite4(a) && a[3] > 0.0f && !(a[2] < 0.0f) && !(a[2] > a[3])) {
            s[0] = 1.0f / a[3]; s[2] = ya;
            if (ends) { ends[0] = ends[1] = s[0]; ends[2] = ends[3] = ya; }
        }
        return;
    }
    to_clip(F, q->p1, drape, b);
    float yb = world_y(F, q->p1, drape);
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
        if (ain) yb = fmaf(t, yb - ya, ya); else ya = fmaf(t, ya - yb, yb);       /* y_out towards y_in, the clipper's own t */
    }
    if (!(a[3] > 0.0f && b[3] > 0.0f)) return;
    const float rwa = 1.0f / a[3], rwb = 1.0f / b[3];
    const float yqa = ya * rwa, yqb = yb * rwb;
    s[0] = rwa; s[1] = rwb - rwa; s[2] = yqa; s[3] = yqb - yqa;
    if (ends) { ends[0] = rwa; ends[1] = rwb; ends[2] = ya; ends[3] = yb; }
}

/* items 1 and 2 at pixel centre (qx, qy): depth, height (dy, may be NULL: d, y, t) and the opacity */
static float prim_ah(const HazeP *Z, const Prim *p, const float s[4], float qx, float qy, float dy[3])
{
    if (dy) dy[0] = dy[1] = dy[2] = 0.0f;
    if (!(s[0] > 0.0f)) return 0.0f;
    float rw = s[0], y = s[2], t = 0.0f;
    if (p->kind == SEGMENT) {
        const float uu = (qx - p->g[0]) * p->g[2] + (qy - p->g[1]) * p->g[3];
        t = fminf(fmaxf(uu / p->h[0], 0.0f), 1.0f);
        rw = fmaf(t, s[1], s[0]);
        y = fmaf(t, s[3], s[2]) / rw;
    }
    const float d = 1.0f / rw;
    if (dy) { dy[0] = d; dy[1] = y; dy[2] = t; }
    return oh_alpha(Z, d, y);
}

/* ocm_composite under the haze (density, haze_rgba, start, falloff, base, max_opacity; eye_y from u): records with flag HAZE take it.
 * ah_plane (H x W, may be NULL): the S.ah of the last hazed feature that covers the pixel; touch (H x W bytes, may be NULL): 1 where a
 * hazed feature covers the pixel; counts (3 words, may be NULL): the (hazed feature, covered pixel) pairs, those of them with
 * 0 < S.ah < max_opacity, and those with S.ah == 0.  Without a flagged record, or with density 0, the frame is ocm_composite's. */
int ohm_composite(uint8_t *rgba, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw, uint32_t th,
                  uint32_t grid, const OvIn *prims, uint32_t nprims, uint32_t nfill, const uint32_t *fill_feature, const uint32_t *fill_rgba,
                  const uint8_t *fill_drape, const uint32_t *fill_rings, const uint32_t *ring_offsets, const float *xyz,
                  float density, uint32_t haze_rgba, float start, float falloff, float base, float max_opacity, float *ah_plane, uint8_t *touch,
                  uint64_t *counts)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    const HazeP Z = { density, start, falloff, base, max_opacity, oh_eye_y(u), haze_rgba };
    const size_t npx = (size_t)W * H;
    float *lin = malloc(npx * 3 * sizeof(float)), *cov = calloc(npx, sizeof(float)), *Q = malloc(npx * sizeof(float)), *ahp = calloc(npx, sizeof(float));
    uint8_t *touched = calloc(npx, 1), *listed = calloc(npx, 1);
    uint32_t *list = malloc(npx * sizeof(uint32_t));
    if (!lin || !cov || !Q || !ahp || !touched || !list || !listed) return -1;
    if (ah_plane) memset(ah_plane, 0, npx * sizeof(float));
    if (touch) memset(touch, 0, npx);
    if (counts) counts[0] = counts[1] = counts[2] = 0;
    int any = 0;
    for (uint32_t k = 0; k < nprims; ++k) any |= (prims[k].flags & OCCLUDE) != 0;
    for (uint32_t py = 0; py < H && any; ++py)
        for (uint32_t px = 0; px < W; ++px) Q[(size_t)py * W + px] = terrain_q(&F, vis[(size_t)py * W + px], (int32_t)px, (int32_t)py);
    float hzl[3];
    for (int c = 0; c < 3; ++c) hzl[c] = g_dec[(haze_rgba >> (8 * c)) & 255u];
    uint32_t k = 0, f = 0;
    while (k < nprims || f < nfill) {
        uint32_t nl = 0, rgba_f;
        int hazed_f = 0;
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
                const int occl = (prims[k].flags & OCCLUDE) != 0, hazed = (prims[k].flags & HAZE) != 0 && density > 0.0f;
                hazed_f |= hazed;
                float kb, rwa = 0.0f, rwb = 0.0f, side[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                memcpy(&kb, &prims[k].pad[0], sizeof kb);
                if (occl) prim_rw(&F, &prims[k], &rwa, &rwb);
                if (hazed) prim_side(&F, &prims[k], side, NULL);
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
                        if (c > cov[o]) {                                  /* item 3: the first primitive that reaches the maximum speaks */
                            cov[o] = c;
                            ahp[o] = hazed ? prim_ah(&Z, &p, side, qx, qy, NULL) : 0.0f;
                        }
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
                const float a = cov[o] * A, ah = ahp[o];
                for (int c = 0; c < 3; ++c) {
                    float s = g_dec[(rgba_f >> (8 * c)) & 255u];
                    if (ah > 0.0f) s = hzl[c] * ah + s * (1.0f - ah);       /* item 4 */
                    lin[3 * o + c] = s * a + lin[3 * o + c] * (1.0f - a);
                }
                if (hazed_f) {
                    if (ah_plane) ah_plane[o] = ah;
                    if (touch) touch[o] = 1;
                    if (counts) { counts[0]++; counts[1] += ah > 0.0f && ah < max_opacity; counts[2] += ah == 0.0f; }
                }
            }
            cov[o] = 0.0f;
            ahp[o] = 0.0f;
        }
    }
    for (size_t o = 0; o < npx; ++o)
        if (touched[o]) {
            for (int c = 0; c < 3; ++c) rgba[4 * o + c] = (uint8_t)ovm_encode(lin[3 * o + c]);
            rgba[4 * o + 3] = 255;
        }
    frame_free(&F); free(lin); free(cov); free(Q); free(ahp); free(touched); free(list); free(listed);
    return 0;
}

/* One record at one pixel, for the model's own tests: out = (coverage, d, y, t, ah, rw_a, rw_b, y_a, y_b) -- the ends after clipping */
int ohm_probe(float out[9], uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw, uint32_t th, uint32_t grid, const OvIn *q,
              int32_t px, int32_t py, float density, uint32_t haze_rgba, float start, float falloff, float base, float max_opacity)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    const HazeP Z = { density, start, falloff, base, max_opacity, oh_eye_y(u), haze_rgba };
    Prim p;
    setup(&F, q, &p);
    float side[4], dy[3];
    prim_side(&F, q, side, out + 5);
    const float qx = (float)px + 0.5f, qy = (float)py + 0.5f;
    const int inside = px >= p.px0 && px <= p.px1 && py >= p.py0 && py <= p.py1;
    out[0] = inside ? cover(&p, qx, qy) : 0.0f;
    out[4] = prim_ah(&Z, &p, side, qx, qy, dy);
    out[1] = dy[0]; out[2] = dy[1]; out[3] = dy[2];
    frame_free(&F);
    return 0;
}

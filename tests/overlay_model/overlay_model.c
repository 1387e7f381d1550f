/* overlay_model.c -- CPU model of the overlay pass (DESIGN.md "Overlays"), the contract the gfx950 kernels of
 * vulkan_forge_amd/csrc/vf_overlay.h are held to bit for bit.  Written from the contract, not from the kernels' structure: no bins,
 * no sorting -- features are composited one after the other, each over the pixels its primitives can reach.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC overlay_model.c -o libovmodel.so -lm     (overlay_model.py does this)
 *
 * Every float operation is a binary32 one in the order the contract states (-ffp-contract=off: no fused multiply-adds except the
 * explicit fmaf calls, which are exact-rounded by C99). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* the primitive records the library builds at add time (vf_overlay.h OvIn, 48 bytes) */
typedef struct {
    float p0[3], p1[3];
    float size;
    uint32_t flags, rgba, feature, pad[2];
} OvIn;

enum { CIRCLE = 0, SQUARE = 1, SEGMENT = 2, KIND = 3, DRAPE = 4, EXT0 = 8, EXT1 = 16 };

/* ---- the project's deterministic sin / cos (vf_device.h) ---- */
static float sin_poly(float r)
{
    float r2 = r * r;
    float p = fmaf(r2, -1.9515295891e-4f, 8.3321608736e-3f);
    p = fmaf(r2, p, -1.6666654611e-1f);
    return fmaf(r * r2, p, r);
}
static float cos_poly(float r)
{
    float r2 = r * r;
    float p = fmaf(r2, 2.443315711809948e-5f, -1.388731625493765e-3f);
    p = fmaf(r2, p, 4.166664568298827e-2f);
    return fmaf(r2 * r2, p, fmaf(-0.5f, r2, 1.0f));
}
static float reduce_pio2(float x, int *q)
{
    float k = rintf(x * 0.636619772f);
    float r = fmaf(-k, 1.5703125f, x);
    r = fmaf(-k, 4.837512969970703125e-4f, r);
    r = fmaf(-k, 7.54978995489188e-8f, r);
    *q = ((int)k) & 3;
    return r;
}
static float det_sin(float x)
{
    int q; float r = reduce_pio2(x, &q);
    float s = sin_poly(r), c = cos_poly(r);
    float v = (q & 1) ? c : s;
    return (q & 2) ? -v : v;
}
static float det_cos(float x)
{
    int q; float r = reduce_pio2(x, &q);
    float s = sin_poly(r), c = cos_poly(r);
    float v = (q & 1) ? -s : c;
    return (q & 2) ? -v : v;
}

/* ---- sRGB ---- */
static double eotf_d(double s) { return s <= 0.04045 ? s / 12.92 : pow((s + 0.055) / 1.055, 2.4); }
static float g_dec[256], g_thr[256];
static int g_tables = 0;
static void tables(void)
{
    if (g_tables) return;
    for (int k = 0; k < 256; ++k) {
        g_dec[k] = (float)eotf_d((double)k / 255.0);
        g_thr[k] = k == 0 ? -INFINITY : (float)eotf_d(((double)k - 0.5) / 255.0);
    }
    g_tables = 1;
}
float ovm_decode(uint32_t k) { tables(); return g_dec[k & 255u]; }
uint32_t ovm_encode(float c)
{
    tables();
    uint32_t k = 0;
    while (k < 255 && c >= g_thr[k + 1]) ++k;
    return k;
}

/* ---- frame ---- */
typedef struct {
    const float *view, *proj;
    float spacing, exag, hw, hh, step;
    uint32_t n, nm1, W, H, tw;
    const float *tex;
    float *sinx, *cosz;
    int32_t *txi, *tyj;
} Frame;

static float height_at(const Frame *F, uint32_t i, uint32_t j)
{
    float h_tex = F->tex[(size_t)F->tyj[j] * F->tw + F->txi[i]];
    float h_ana = F->sinx[i] * 0.25f + F->cosz[j] * 0.25f;
    return h_tex + h_ana;
}

float ovm_drape_h(const Frame *F, float x, float z)
{
    float mx = x / F->spacing, mz = z / F->spacing;
    mx = fminf(fmaxf(mx, -1.5f), 1.5f);
    mz = fminf(fmaxf(mz, -1.5f), 1.5f);
    const float gx = (mx + 1.5f) / F->step, gz = (mz + 1.5f) / F->step;
    int i = (int)floorf(gx), j = (int)floorf(gz);
    const int top = (int)F->nm1 - 1;
    i = i < 0 ? 0 : (i > top ? top : i);
    j = j < 0 ? 0 : (j > top ? top : j);
    const float fx = gx - (float)i, fz = gz - (float)j;
    const float hb = height_at(F, (uint32_t)i + 1u, (uint32_t)j), hc = height_at(F, (uint32_t)i, (uint32_t)j + 1u);
    if (fx + fz <= 1.0f) {
        const float ha = height_at(F, (uint32_t)i, (uint32_t)j);
        return (ha + fx * (hb - ha)) + fz * (hc - ha);
    }
    const float hd = height_at(F, (uint32_t)i + 1u, (uint32_t)j + 1u);
    return (hd + (1.0f - fx) * (hc - hd)) + (1.0f - fz) * (hb - hd);
}

static void mat_vec(const float *m, float x, float y, float z, float w, float r[4])
{
    for (int k = 0; k < 4; ++k) {
        float acc = m[k] * x;
        acc = fmaf(m[4 + k], y, acc);
        acc = fmaf(m[8 + k], z, acc);
        acc = fmaf(m[12 + k], w, acc);
        r[k] = acc;
    }
}

static void to_clip(const Frame *F, const float p[3], int drape, float c[4])
{
    float y = p[1];
    if (drape) y = ovm_drape_h(F, p[0], p[2]) * F->exag + p[1];
    float vp[4];
    mat_vec(F->view, p[0], y, p[2], 1.0f, vp);
    mat_vec(F->proj, vp[0], vp[1], vp[2], vp[3], c);
}

static int finite4(const float *v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]); }

typedef struct { uint32_t kind; float g[4], h[4]; int px0, px1, py0, py1; } Prim;

static void span(float a, float b, uint32_t n, int *lo, int *hi)
{
    const float lim = (float)n + 2.0f;
    int l = (int)floorf(fminf(fmaxf(a, -2.0f), lim)), h = (int)floorf(fminf(fmaxf(b, -2.0f), lim));
    *lo = l < 0 ? 0 : l;
    *hi = h > (int)n - 1 ? (int)n - 1 : h;
}

/* the screen-space primitive (contract: drape, transform, clip / cull, viewport) and the pixels it may cover */
static void setup(const Frame *F, const OvIn *q, Prim *o)
{
    memset(o, 0, sizeof *o);
    o->kind = q->flags & KIND;
    o->px0 = 1; o->px1 = 0; o->py0 = 1; o->py1 = 0;
    const int drape = (q->flags & DRAPE) != 0;
    float x0 = 0.0f, x1 = -1.0f, y0 = 0.0f, y1 = -1.0f;
    float a[4];
    to_clip(F, q->p0, drape, a);
    if (o->kind != SEGMENT) {
        if (!(finite4(a) && a[3] > 0.0f && !(a[2] < 0.0f) && !(a[2] > a[3]))) return;
        const float rw = 1.0f / a[3];
        const float sx = fmaf(a[0] * rw, F->hw, F->hw), sy = fmaf(-(a[1] * rw), F->hh, F->hh);
        if (!isfinite(sx) || !isfinite(sy)) return;
        const float r = q->size, R = r + 1.0f;
        o->g[0] = sx; o->g[1] = sy; o->g[2] = r;
        x0 = sx - R; x1 = sx + R; y0 = sy - R; y1 = sy + R;
    } else {
        float b[4];
        to_clip(F, q->p1, drape, b);
        if (!finite4(a) || !finite4(b)) return;
        int ext0 = (q->flags & EXT0) != 0, ext1 = (q->flags & EXT1) != 0;
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
            if (ain) ext1 = 0; else ext0 = 0;
        }
        if (!(a[3] > 0.0f && b[3] > 0.0f)) return;
        const float rwa = 1.0f / a[3], rwb = 1.0f / b[3];
        const float ax = fmaf(a[0] * rwa, F->hw, F->hw), ay = fmaf(-(a[1] * rwa), F->hh, F->hh);
        const float bx = fmaf(b[0] * rwb, F->hw, F->hw), by = fmaf(-(b[1] * rwb), F->hh, F->hh);
        const float ex = bx - ax, ey = by - ay;
        const float L = sqrtf(ex * ex + ey * ey);
        if (!(isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by) && L > 0.0f && isfinite(L))) return;
        const float hw = q->size, e0 = ext0 ? hw : 0.0f, e1 = ext1 ? hw : 0.0f;
        o->g[0] = ax; o->g[1] = ay; o->g[2] = ex / L; o->g[3] = ey / L;
        o->h[0] = L; o->h[1] = hw; o->h[2] = e0; o->h[3] = e1;
        const float R = hw + fmaxf(e0, e1) + 1.0f;
        x0 = fminf(ax, bx) - R; x1 = fmaxf(ax, bx) + R; y0 = fminf(ay, by) - R; y1 = fmaxf(ay, by) + R;
    }
    span(x0, x1, F->W, &o->px0, &o->px1);
    span(y0, y1, F->H, &o->py0, &o->py1);
}

static float cover(const Prim *p, float qx, float qy)
{
    float sd;
    const float dx = qx - p->g[0], dy = qy - p->g[1];
    if (p->kind == SEGMENT) {
        const float u = dx * p->g[2] + dy * p->g[3];
        const float v = fabsf(dy * p->g[2] - dx * p->g[3]);
        sd = fmaxf(v - p->h[1], fmaxf(-u - p->h[2], (u - p->h[0]) - p->h[3]));
    } else if (p->kind == CIRCLE) {
        sd = sqrtf(dx * dx + dy * dy) - p->g[2];
    } else {
        sd = fmaxf(fabsf(dx), fabsf(dy)) - p->g[2];
    }
    return fminf(fmaxf(0.5f - sd, 0.0f), 1.0f);
}

/* The frame rgba (H x W x 4, sRGB8, composited in place) under uniforms u[44], height texture tex (th x tw), grid vertices per side. */
int ovm_composite(uint8_t *rgba, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw, uint32_t th, uint32_t grid,
                  const OvIn *prims, uint32_t nprims)
{
    tables();
    Frame F;
    F.view = u; F.proj = u + 16;
    F.spacing = fmaxf(u[36], 1e-8f); F.exag = u[38];
    F.hw = 0.5f * (float)W; F.hh = 0.5f * (float)H;
    F.n = grid < 2 ? 2 : grid; F.nm1 = F.n - 1;
    F.step = (2.0f * 1.5f) / ((float)F.n - 1.0f);
    F.W = W; F.H = H; F.tw = tw; F.tex = tex;
    F.sinx = malloc(F.n * sizeof(float)); F.cosz = malloc(F.n * sizeof(float));
    F.txi = malloc(F.n * sizeof(int32_t)); F.tyj = malloc(F.n * sizeof(int32_t));
    const size_t npx = (size_t)W * H;
    float *lin = malloc(npx * 3 * sizeof(float)), *cov = calloc(npx, sizeof(float));
    uint8_t *touched = calloc(npx, 1);
    uint32_t *list = malloc(npx * sizeof(uint32_t));
    uint8_t *listed = calloc(npx, 1);
    if (!F.sinx || !F.cosz || !F.txi || !F.tyj || !lin || !cov || !touched || !list || !listed) return -1;
    const float nm1f = (float)F.n - 1.0f;
    for (uint32_t i = 0; i < F.n; ++i) {
        const float x = -1.5f + (float)i * F.step, uvc = (float)i / nm1f;
        F.sinx[i] = det_sin(x * 1.3f);
        F.cosz[i] = det_cos(x * 1.1f);
        int tx = (int)floorf(uvc * (float)tw), ty = (int)floorf(uvc * (float)th);
        F.txi[i] = tx < 0 ? 0 : (tx > (int)tw - 1 ? (int)tw - 1 : tx);
        F.tyj[i] = ty < 0 ? 0 : (ty > (int)th - 1 ? (int)th - 1 : ty);
    }
    uint32_t k = 0;
    while (k < nprims) {
        /* one feature: its primitives' coverage, max-folded, then one blend per pixel */
        const uint32_t feature = prims[k].feature, rgba_f = prims[k].rgba;
        uint32_t nl = 0;
        for (; k < nprims && prims[k].feature == feature; ++k) {
            Prim p;
            setup(&F, &prims[k], &p);
            for (int py = p.py0; py <= p.py1; ++py)
                for (int px = p.px0; px <= p.px1; ++px) {
                    const size_t o = (size_t)py * W + (size_t)px;
                    const float c = cover(&p, (float)px + 0.5f, (float)py + 0.5f);
                    cov[o] = fmaxf(cov[o], c);
                    if (!listed[o]) { listed[o] = 1; list[nl++] = (uint32_t)o; }
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
    free(F.sinx); free(F.cosz); free(F.txi); free(F.tyj); free(lin); free(cov); free(touched); free(list); free(listed);
    return 0;
}

/* drape height h (before exaggeration) at world (x, z): the vertex stage's surface, for the model's own tests */
float ovm_drape(const float *u, const float *tex, uint32_t tw, uint32_t th, uint32_t grid, float x, float z)
{
    Frame F;
    memset(&F, 0, sizeof F);
    F.spacing = fmaxf(u[36], 1e-8f);
    F.n = grid < 2 ? 2 : grid; F.nm1 = F.n - 1;
    F.step = (2.0f * 1.5f) / ((float)F.n - 1.0f);
    F.tw = tw; F.tex = tex;
    float sinx[8192], cosz[8192];
    int32_t txi[8192], tyj[8192];
    if (F.n > 8192) return NAN;
    F.sinx = sinx; F.cosz = cosz; F.txi = txi; F.tyj = tyj;
    const float nm1f = (float)F.n - 1.0f;
    for (uint32_t i = 0; i < F.n; ++i) {
        const float xx = -1.5f + (float)i * F.step, uvc = (float)i / nm1f;
        sinx[i] = det_sin(xx * 1.3f);
        cosz[i] = det_cos(xx * 1.1f);
        int tx = (int)floorf(uvc * (float)tw), ty = (int)floorf(uvc * (float)th);
        txi[i] = tx < 0 ? 0 : (tx > (int)tw - 1 ? (int)tw - 1 : tx);
        tyj[i] = ty < 0 ? 0 : (ty > (int)th - 1 ? (int)th - 1 : ty);
    }
    return ovm_drape_h(&F, x, z);
}

/* vertex (i, j)'s displaced height as the vertex stage forms it (h_tex + 0.25 sin(1.3 x_i) + 0.25 cos(1.1 z_j)) */
float ovm_vertex_height(const float *tex, uint32_t tw, uint32_t th, uint32_t grid, uint32_t i, uint32_t j)
{
    const uint32_t n = grid < 2 ? 2 : grid;
    const float step = (2.0f * 1.5f) / ((float)n - 1.0f), nm1f = (float)n - 1.0f;
    const float xi = -1.5f + (float)i * step, zj = -1.5f + (float)j * step;
    int tx = (int)floorf(((float)i / nm1f) * (float)tw), ty = (int)floorf(((float)j / nm1f) * (float)th);
    tx = tx < 0 ? 0 : (tx > (int)tw - 1 ? (int)tw - 1 : tx);
    ty = ty < 0 ? 0 : (ty > (int)th - 1 ? (int)th - 1 : ty);
    return tex[(size_t)ty * tw + tx] + (det_sin(xi * 1.3f) * 0.25f + det_cos(zj * 1.1f) * 0.25f);
}

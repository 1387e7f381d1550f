/* drape_mip_model.c -- CPU model of the mip pyramid under the draped image and of its trilinear filtering, the
 * contract the gfx950 kernels of vulkan_forge_amd/csrc/vf_drape_mips.h (k_drape_mips) and vf_relight.h (k_relight<., kDrapeMip>) are
 * held to bit for bit.  Written from the contract, layered on the drape model (included below): the pyramid is one plain loop per
 * level over the stored binary16 values of the level above; the frame is drm_frame with the level of detail of every covered pixel
 * formed from the varyings of the same piece of the same primitive one pixel to the right and one below.  binary16 is converted by
 * hand (round to nearest even, denormals kept).
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC drape_mip_model.c -o libdrmipmodel.so -lm     (drape_mip_model.py does this)
 */
#include "../drape_model/drape_model.c"

/* binary32 -> binary16, round to nearest even; values beyond the largest finite binary16 become infinity, NaN stays NaN */
static uint16_t dmm_half(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    const uint32_t sign = (b >> 16) & 0x8000u, e = (b >> 23) & 255u, m = b & 0x7FFFFFu;
    if (e == 255u) return (uint16_t)(sign | 0x7C00u | (m ? 0x200u : 0u));
    const int32_t E = (int32_t)e - 127 + 15;                 /* the binary16 exponent field of a normal result */
    if (E >= 31) return (uint16_t)(sign | 0x7C00u);
    uint32_t sig, shift;                                     /* the 24-bit significand, and how many of its low bits are dropped */
    if (E <= 0) {
        if (E < -10) return (uint16_t)sign;                  /* below half of the smallest denormal: zero (exactly half rounds to even: zero) */
        sig = m | 0x800000u; shift = (uint32_t)(14 - E);     /* a denormal result: 14 ... 24 bits go */
    } else { sig = m | 0x800000u; shift = 13u; }
    uint32_t r = sig >> shift;
    const uint32_t rest = sig & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rest > half || (rest == half && (r & 1u))) r++;
    /* r holds the hidden bit when normal: adding the exponent field less one lets a carry out of the mantissa raise the exponent */
    const uint32_t h = E <= 0 ? r : (((uint32_t)E - 1u) << 10) + r;
    return (uint16_t)(sign | h);                             /* (h == 0x7C00 after a carry at the top: infinity, as it should be) */
}

static float dmm_unhalf(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    float f;
    if (e == 0u) f = ldexpf((float)m, -24);
    else if (e == 31u) f = m ? NAN : INFINITY;
    else f = ldexpf((float)(m | 0x400u), (int)e - 25);
    uint32_t b;
    memcpy(&b, &f, 4);
    b |= sign;
    memcpy(&f, &b, 4);
    return f;
}

/* the sizes of the levels: w[0] = iw ..., each max(1, (size + 1) >> 1); -> the number of levels */
uint32_t dmm_levels(uint32_t iw, uint32_t ih, uint32_t *w, uint32_t *h)
{
    uint32_t n = 1;
    w[0] = iw; h[0] = ih;
    while (w[n - 1u] > 1u || h[n - 1u] > 1u) {
        w[n] = (w[n - 1u] + 1u) >> 1; h[n] = (h[n - 1u] + 1u) >> 1;
        if (w[n] < 1u) w[n] = 1u;
        if (h[n] < 1u) h[n] = 1u;
        ++n;
    }
    return n;
}

/* img (ih x iw x 4 bytes) -> levels 1 ... of the pyramid in `out`, one after the other, four binary16 values per texel.  A texel is
 * the mean of the parents (2i + {0, 1}, 2j + {0, 1}) that exist: the sum in the order (2i, 2j), (2i + 1, 2j), (2i, 2j + 1),
 * (2i + 1, 2j + 1) in binary32, times 1 / count, rounded to binary16.  Level 1's parents are drm_texel's values, a later level's the
 * stored binary16 values of the level above. */
int dmm_pyramid(uint16_t *out, const uint8_t *img, uint32_t iw, uint32_t ih)
{
    uint32_t w[16], h[16];
    const uint32_t n = dmm_levels(iw, ih, w, h);
    const uint16_t *above = NULL;
    for (uint32_t k = 1; k < n; ++k) {
        for (uint32_t j = 0; j < h[k]; ++j)
            for (uint32_t i = 0; i < w[k]; ++i) {
                float s[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                int count = 0;
                for (uint32_t b = 0; b < 2; ++b)
                    for (uint32_t a = 0; a < 2; ++a) {
                        const uint32_t pi = 2u * i + a, pj = 2u * j + b;
                        if (pi >= w[k - 1u] || pj >= h[k - 1u]) continue;
                        float q[4];
                        if (k == 1u) drm_texel(img, iw, (int)pi, (int)pj, q);
                        else for (int c = 0; c < 4; ++c) q[c] = dmm_unhalf(above[4u * ((size_t)pj * w[k - 1u] + pi) + (size_t)c]);
                        for (int c = 0; c < 4; ++c) s[c] = count ? s[c] + q[c] : q[c];
                        ++count;
                    }
                const float inv = 1.0f / (float)count;
                for (int c = 0; c < 4; ++c) out[4u * ((size_t)j * w[k] + i) + (size_t)c] = dmm_half(s[c] * inv);
            }
        above = out;
        out += 4u * (size_t)w[k] * h[k];
    }
    return (int)n;
}

/* a pyramid as the sampler reads it */
typedef struct {
    const uint8_t *img;
    const uint16_t *lvl[16];
    uint32_t w[16], h[16], levels;
    float x0, z0, sx, sz, bias;
    int linear;
} Mips;

/* item 3: the level of detail from the footprint; -inf: level 0, +inf: the top level */
static float dmm_lod(const Mips *M, float x, float z, float xr, float zr, float xd, float zd)
{
    const float dux = (xr - x) * M->sx, dvx = (zr - z) * M->sz;
    const float ax = fmaf(dux, dux, dvx * dvx);
    const float duy = (xd - x) * M->sx, dvy = (zd - z) * M->sz;
    const float ay = fmaf(duy, duy, dvy * dvy);
    const float rho2 = ay > ax ? ay : ax;
    uint32_t bits;
    memcpy(&bits, &rho2, 4);
    const uint32_t E = (bits >> 23) & 255u, Mn = bits & 0x7FFFFFu;
    if ((bits >> 31) != 0u || E == 0u || (E == 255u && Mn != 0u)) return -INFINITY;
    if (E == 255u) return INFINITY;
    return 0.5f * ((float)((int)E - 127) + (float)Mn * 0x1p-23f) + M->bias;
}

static void dmm_texel(const Mips *M, int k, int ix, int iy, float q[4])
{
    for (int c = 0; c < 4; ++c) q[c] = dmm_unhalf(M->lvl[k][4u * ((size_t)iy * M->w[k] + (size_t)ix) + (size_t)c]);
}

/* item 5: level k at the level-0 coordinates (fu, fv) of a point inside the image; level 0 is 4j's sample */
static void dmm_level(const Mips *M, int k, float x, float z, float fu, float fv, float val[4])
{
    if (k == 0) { (void)drm_sample(M->img, M->w[0], M->h[0], M->x0, M->z0, M->sx, M->sz, M->linear, x, z, val); return; }
    const float sc = ldexpf(1.0f, -k);
    const float fuk = fu * sc, fvk = fv * sc;
    const int mx = (int)M->w[k] - 1, my = (int)M->h[k] - 1;
    if (!M->linear) {
        int ix = (int)floorf(fuk), iy = (int)floorf(fvk);
        ix = ix < mx ? ix : mx; iy = iy < my ? iy : my;
        dmm_texel(M, k, ix, iy, val);
        return;
    }
    const float cu = fuk - 0.5f, cv = fvk - 0.5f;
    const float i0f = floorf(cu), j0f = floorf(cv);
    const float fx = cu - i0f, fy = cv - j0f;
    const int c0 = clampi((int)i0f, 0, mx), c1 = clampi((int)i0f + 1, 0, mx);
    const int r0 = clampi((int)j0f, 0, my), r1 = clampi((int)j0f + 1, 0, my);
    float q00[4], q01[4], q10[4], q11[4];
    dmm_texel(M, k, c0, r0, q00); dmm_texel(M, k, c1, r0, q01);
    dmm_texel(M, k, c0, r1, q10); dmm_texel(M, k, c1, r1, q11);
    for (int c = 0; c < 4; ++c) {
        const float top = fmaf(fx, q01[c] - q00[c], q00[c]);
        const float bot = fmaf(fx, q11[c] - q10[c], q10[c]);
        val[c] = fmaf(fy, bot - top, top);
    }
}

/* items 4-6: the image at world (x, z) with level of detail lod; 0 outside the extent */
static int dmm_sample(const Mips *M, float x, float z, float lod, float val[4])
{
    if (!(lod > 0.0f)) return drm_sample(M->img, M->w[0], M->h[0], M->x0, M->z0, M->sx, M->sz, M->linear, x, z, val);
    const float fu = (x - M->x0) * M->sx, fv = (z - M->z0) * M->sz;
    if (!(fu >= 0.0f && fu <= (float)M->w[0] && fv >= 0.0f && fv <= (float)M->h[0])) return 0;
    const int top = (int)M->levels - 1;
    if (!M->linear) {
        const float ln = lod + 0.5f;
        dmm_level(M, ln >= (float)top ? top : (int)floorf(ln), x, z, fu, fv, val);
        return 1;
    }
    if (lod >= (float)top) { dmm_level(M, top, x, z, fu, fv, val); return 1; }
    const float lf = floorf(lod), t = lod - lf;
    const int l = (int)lf;
    float lo[4], hi[4];
    dmm_level(M, l, x, z, fu, fv, lo);
    dmm_level(M, l + 1, x, z, fu, fv, hi);
    for (int c = 0; c < 4; ++c) val[c] = fmaf(t, hi[c] - lo[c], lo[c]);
    return 1;
}

/* tri_weights at another pixel centre, with no cover test: the edge functions of the piece go on outside it and outside the frame */
static void tri_weights_at(const Frame *F, const CVert *a, const CVert *b, const CVert *c, int32_t px, int32_t py, float q[3])
{
    int32_t X[3], Y[3];
    float rw[3];
    const CVert *v[3] = { a, b, c };
    for (int k = 0; k < 3; ++k) (void)snap(F, v[k], &X[k], &Y[k], &rw[k]);
    const int64_t area2 = (int64_t)(X[1] - X[0]) * (Y[2] - Y[0]) - (int64_t)(Y[1] - Y[0]) * (X[2] - X[0]);
    const int64_t Px = (int64_t)px * 256 + 128, Py = (int64_t)py * 256 + 128;
    const float fA = (float)(-area2);
    for (int k = 0; k < 3; ++k) {
        const int s = (k + 1) % 3, t = (k + 2) % 3;
        const int64_t e = -((int64_t)(X[t] - X[s]) * (Py - Y[s]) - (int64_t)(Y[t] - Y[s]) * (Px - X[s]));
        q[k] = ((float)e / fA) * rw[k];
    }
}

/* drm_frame through the pyramid.  pyr: what dmm_pyramid made.  sample (H x W x 7 floats, or NULL): drm_frame's six and the level of
 * detail (bias included; -inf and +inf as dmm_lod gives them) of the pixels inside the image's extent whose sample was taken. */
int dmm_frame(uint8_t *rgba, uint8_t *rewritten, float *sample, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex,
              uint32_t tw, uint32_t th, uint32_t grid, const uint8_t *lut_rgba8, int shade_mode, const uint8_t *img, uint32_t iw, uint32_t ih,
              const uint16_t *pyr, const float *extent, float opacity, int linear, float bias, const float *lit, const float *sky, float strength)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    Shade S;
    S.h_range = fmaxf(u[37], 1e-8f); S.exposure = u[35];
    {
        const float sx = u[32], sy = u[33], sz = u[34];
        const float inv = 1.0f / sqrtf(fmaf(sz, sz, fmaf(sy, sy, sx * sx)));
        S.Lx = sx * inv; S.Ly = sy * inv; S.Lz = sz * inv;
    }
    for (int k = 0; k < 256; ++k)
        for (int ch = 0; ch < 3; ++ch) S.lut[k][ch] = ovm_decode(lut_rgba8[4 * k + ch]);
    S.shade_mode = shade_mode; S.tex = tex; S.tw = tw; S.th = th; S.spacing = F.spacing; S.exag = F.exag;
    Mips M;
    M.img = img; M.levels = dmm_levels(iw, ih, M.w, M.h);
    M.lvl[0] = NULL;
    for (uint32_t k = 1; k < M.levels; ++k) { M.lvl[k] = pyr; pyr += 4u * (size_t)M.w[k] * M.h[k]; }
    M.x0 = extent[0]; M.z0 = extent[1];
    M.sx = (float)iw / (extent[2] - extent[0]); M.sz = (float)ih / (extent[3] - extent[1]);
    M.bias = bias; M.linear = linear;
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const size_t o = (size_t)py * W + px;
            rewritten[o] = 0;
            if (sample) for (int k = 0; k < 7; ++k) sample[7 * o + k] = 0.0f;
            const uint32_t id = vis[o];
            if (id == 0u) continue;
            const uint32_t prim = id - 1u, cell = prim >> 1, odd = prim & 1u;
            const uint32_t j = cell / F.nm1, i = cell - j * F.nm1;
            const uint32_t vi[3] = { odd ? i + 1u : i, i, i + 1u }, vj[3] = { j, j + 1u, odd ? j + 1u : j };
            float l[3], am[3];
            for (int k = 0; k < 3; ++k) {
                const size_t v = (size_t)vj[k] * F.n + vi[k];
                l[k] = lit ? lit[v] : 1.0f;
                am[k] = sky ? 1.0f - strength * (1.0f - sky[v]) : 1.0f;
            }
            const int plain_l = l[0] == 1.0f && l[1] == 1.0f && l[2] == 1.0f, plain_a = am[0] == 1.0f && am[1] == 1.0f && am[2] == 1.0f;
            AVert v[3], poly[8];
            float attr[3] = { 0.0f, 0.0f, 0.0f }, val[4], lv[3] = { 0.0f, 1.0f, 1.0f }, lod = 0.0f;
            int keep = 1;
            for (int pass = 0; pass < 3 && keep; ++pass) {
                if ((pass == 1 && plain_l) || (pass == 2 && plain_a)) continue;
                for (int k = 0; k < 3; ++k) { v[k] = attr_vertex(&F, vi[k], vj[k]); if (pass) v[k].a[0] = pass == 1 ? l[k] : am[k]; }
                const int np = clip_attr(v, poly);
                float r[3] = { 0.0f, 0.0f, 0.0f };
                int piece = 0;                                                 /* the last piece that covers the centre */
                for (int f = 1; f + 1 < np; ++f) {
                    float q[3];
                    if (!tri_weights(&F, &poly[0].c, &poly[f].c, &poly[f + 1].c, (int32_t)px, (int32_t)py, q)) continue;
                    const float rQ = 1.0f / ((q[0] + q[1]) + q[2]);
                    for (int a = 0; a < 3; ++a) r[a] = fmaf(q[2], poly[f + 1].a[a], fmaf(q[1], poly[f].a[a], q[0] * poly[0].a[a])) * rQ;
                    piece = f;
                }
                if (pass) { lv[pass] = fminf(r[0], 1.0f); continue; }
                memcpy(attr, r, sizeof r);
                /* item 1: the varyings of that piece at the centres to the right and below (zero when no piece covers the pixel) */
                float nb[2][3] = { { 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f } };
                if (piece)
                    for (int d = 0; d < 2; ++d) {
                        float q[3];
                        tri_weights_at(&F, &poly[0].c, &poly[piece].c, &poly[piece + 1].c, (int32_t)px + (d == 0), (int32_t)py + (d == 1), q);
                        const float rQ = 1.0f / ((q[0] + q[1]) + q[2]);
                        for (int a = 0; a < 3; ++a) nb[d][a] = fmaf(q[2], poly[piece + 1].a[a], fmaf(q[1], poly[piece].a[a], q[0] * poly[0].a[a])) * rQ;
                    }
                lod = dmm_lod(&M, attr[1], attr[2], nb[0][1], nb[0][2], nb[1][1], nb[1][2]);
                keep = dmm_sample(&M, attr[1], attr[2], lod, val) && val[3] * opacity > 0.0f;
            }
            if (!keep) continue;
            frag_alb(&S, attr, lv[1], lv[2], val, opacity, rgba + 4 * o);
            rewritten[o] = 1;
            if (sample) { memcpy(sample + 7 * o, val, sizeof val); sample[7 * o + 4] = lv[1]; sample[7 * o + 5] = lv[2]; sample[7 * o + 6] = lod; }
        }
    frame_free(&F);
    return 0;
}

/* how many covered pixels show a primitive that the near or the far plane cuts (the kernels' generic path): the cases must hold some */
int dmm_clipped_pixels(const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw, uint32_t th, uint32_t grid)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    int count = 0;
    for (size_t o = 0; o < (size_t)W * H; ++o) {
        if (vis[o] == 0u) continue;
        const uint32_t prim = vis[o] - 1u, cell = prim >> 1, odd = prim & 1u;
        const uint32_t j = cell / F.nm1, i = cell - j * F.nm1;
        const uint32_t vi[3] = { odd ? i + 1u : i, i, i + 1u }, vj[3] = { j, j + 1u, odd ? j + 1u : j };
        int cut = 0;
        for (int k = 0; k < 3; ++k) { const AVert v = attr_vertex(&F, vi[k], vj[k]); cut |= v.c.z < 0.0f || v.c.z > v.c.w; }
        count += cut;
    }
    frame_free(&F);
    return count;
}

/* for the tests of the conversion itself */
uint16_t dmm_half_bits(float f) { return dmm_half(f); }
float dmm_half_value(uint16_t h) { return dmm_unhalf(h); }

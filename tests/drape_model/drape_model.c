/* drape_model.c -- CPU model of the draped image layer, the contract the gfx950 kernel of
 * vulkan_forge_amd/csrc/vf_drape.h and vf_relight.h (k_relight<., kDrape>) is held to bit for bit.  Written from the contract: the frame takes a frame and
 * its visibility ids, forms the varyings (h, x, z) of every covered pixel as the shadow and ambient models do (included below: clip,
 * fan, last covering piece), samples the image at (x, z) and shades the pixels whose sample is not transparent again with a
 * restatement of fs_main in which the colormap value is mixed with the sample; lit and amb are formed by the rules of 4g and 4i.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC drape_model.c -o libdrmodel.so -lm     (drape_model.py does this)
 */
#include "../ambient_model/ambient_model.c"

/* item 3: texel (ix, iy) of the row-major RGBA8 image -> premultiplied linear colour and alpha */
static void drm_texel(const uint8_t *img, uint32_t iw, int ix, int iy, float q[4])
{
    const uint8_t *p = img + 4u * ((size_t)iy * iw + (size_t)ix);
    const float a = (float)p[3] / 255.0f;
    for (int ch = 0; ch < 3; ++ch) q[ch] = ovm_decode(p[ch]) * a;
    q[3] = a;
}

/* items 2, 4 and 5: the image at world (x, z); 0 outside the extent (a NaN is outside): the test comes first, the indices after */
static int drm_sample(const uint8_t *img, uint32_t iw, uint32_t ih, float x0, float z0, float sx, float sz, int linear, float x, float z, float val[4])
{
    const float fu = (x - x0) * sx, fv = (z - z0) * sz;
    if (!(fu >= 0.0f && fu <= (float)iw && fv >= 0.0f && fv <= (float)ih)) return 0;
    const int mx = (int)iw - 1, my = (int)ih - 1;
    if (!linear) {
        int ix = (int)floorf(fu), iy = (int)floorf(fv);
        ix = ix < mx ? ix : mx; iy = iy < my ? iy : my;
        drm_texel(img, iw, ix, iy, val);
        return 1;
    }
    const float cu = fu - 0.5f, cv = fv - 0.5f;
    const float i0f = floorf(cu), j0f = floorf(cv);
    const float fx = cu - i0f, fy = cv - j0f;
    const int c0 = clampi((int)i0f, 0, mx), c1 = clampi((int)i0f + 1, 0, mx);
    const int r0 = clampi((int)j0f, 0, my), r1 = clampi((int)j0f + 1, 0, my);
    float q00[4], q01[4], q10[4], q11[4];
    drm_texel(img, iw, c0, r0, q00); drm_texel(img, iw, c1, r0, q01);
    drm_texel(img, iw, c0, r1, q10); drm_texel(img, iw, c1, r1, q11);
    for (int k = 0; k < 4; ++k) {
        const float top = fmaf(fx, q01[k] - q00[k], q00[k]);
        const float bot = fmaf(fx, q11[k] - q10[k], q10[k]);
        val[k] = fmaf(fy, bot - top, top);
    }
    return 1;
}

/* items 6 and 7: frag_amb of the ambient model with the colormap value of each channel replaced by the mixed albedo */
static void frag_alb(const Shade *S, const float attr[3], float lit, float amb, const float val[4], float opacity, uint8_t out[4])
{
    const float Aop = val[3] * opacity;
    const float height = attr[0], x = attr[1], z = attr[2];
    float t = 0.5f + height / (2.0f * S->h_range);
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const float c = t * 256.0f - 0.5f;
    const float i0f = floorf(c);
    const float f = c - i0f;
    int i0 = (int)i0f, i1 = i0 + 1;
    i0 = clampi(i0, 0, 255); i1 = clampi(i1, 0, 255);
    float nx, ny, nz;
    if (S->shade_mode == 0) {
        const float dhdx = 1.3f * det_cos(x * 1.3f) * 0.25f;
        const float dhdz = -1.1f * det_sin(z * 1.1f) * 0.25f;
        const float d = fmaf(dhdz, dhdz, fmaf(dhdx, dhdx, 1.0f));
        const float inv = 1.0f / sqrtf(d);
        nx = -dhdx * inv; ny = inv; nz = -dhdz * inv;
    } else {
        const float third = 1.0f / 3.0f;
        const float uu = fmaf(x, third, 0.5f), vv = fmaf(z, third, 0.5f);
        const float du = 1.0f / (float)((S->tw > 2u ? S->tw : 2u) - 1u), dv = 1.0f / (float)((S->th > 2u ? S->th : 2u) - 1u);
        const int mx = (int)S->tw - 1, my = (int)S->th - 1;
        const int tx0 = clampi((int)floorf(uu * (float)S->tw), 0, mx), tx1 = clampi((int)floorf((uu + du) * (float)S->tw), 0, mx);
        const int ty0 = clampi((int)floorf(vv * (float)S->th), 0, my), ty1 = clampi((int)floorf((vv + dv) * (float)S->th), 0, my);
        const float h0 = S->tex[(size_t)ty0 * S->tw + tx0], hx = S->tex[(size_t)ty0 * S->tw + tx1], hy = S->tex[(size_t)ty1 * S->tw + tx0];
        const float ax = (hx - h0) * S->exag, az = (hy - h0) * S->exag, sp = S->spacing;
        const float vx = -(ax * sp), vy = sp * sp, vz = -(sp * az);
        const float d = fmaf(vz, vz, fmaf(vy, vy, vx * vx));
        const float inv = 1.0f / sqrtf(d);
        nx = vx * inv; ny = vy * inv; nz = vz * inv;
    }
    const float ndl = fmaf(nz, S->Lz, fmaf(ny, S->Ly, nx * S->Lx));
    const float lambert = fminf(fmaxf(ndl, 0.0f), 1.0f) * lit;
    const float shade = (0.15f * (1.0f - lambert) + lambert) * amb;
    for (int ch = 0; ch < 3; ++ch) {
        const float l0 = S->lut[i0][ch], l1 = S->lut[i1][ch];
        const float lc = fmaf(f, l1 - l0, l0);
        const float alb = fmaf(opacity, val[ch], (1.0f - Aop) * lc);
        float v = alb * S->exposure * shade;
        if (S->shade_mode != 0) v = v / (1.0f + v);
        out[ch] = (uint8_t)ovm_encode(v);
    }
    out[3] = 255;
}

/* rgba (H x W x 4, the plain frame) -> the frame with the image draped on it, in place; rewritten (H x W): 1 where the pixel was
 * written again; sample (H x W x 6 floats, or NULL): the filtered premultiplied (r, g, b, a) of those pixels and the lit and amb they were shaded
 * with, 0 elsewhere.
 * img: ih x iw x 4 bytes.  extent: (x0, z0, x1, z1).  lit, sky: the fields (n x n), or NULL when the feature is off. */
int drm_frame(uint8_t *rgba, uint8_t *rewritten, float *sample, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex,
              uint32_t tw, uint32_t th, uint32_t grid, const uint8_t *lut_rgba8, int shade_mode, const uint8_t *img, uint32_t iw, uint32_t ih,
              const float *extent, float opacity, int linear, const float *lit, const float *sky, float strength)
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
    /* item 2: the host's two divisions */
    const float x0 = extent[0], z0 = extent[1];
    const float sx = (float)iw / (extent[2] - extent[0]), sz = (float)ih / (extent[3] - extent[1]);
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const size_t o = (size_t)py * W + px;
            rewritten[o] = 0;
            if (sample) for (int k = 0; k < 6; ++k) sample[6 * o + k] = 0.0f;
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
            float attr[3] = { 0.0f, 0.0f, 0.0f }, val[4], lv[3] = { 0.0f, 1.0f, 1.0f };
            int keep = 1;
            for (int pass = 0; pass < 3 && keep; ++pass) {                    /* item 1: the varyings (h, x, z); item 7: lit, then amb in the place of h */
                if ((pass == 1 && plain_l) || (pass == 2 && plain_a)) continue;
                for (int k = 0; k < 3; ++k) { v[k] = attr_vertex(&F, vi[k], vj[k]); if (pass) v[k].a[0] = pass == 1 ? l[k] : am[k]; }
                const int np = clip_attr(v, poly);
                float r[3] = { 0.0f, 0.0f, 0.0f };
                for (int f = 1; f + 1 < np; ++f) {
                    float q[3];
                    if (!tri_weights(&F, &poly[0].c, &poly[f].c, &poly[f + 1].c, (int32_t)px, (int32_t)py, q)) continue;
                    const float rQ = 1.0f / ((q[0] + q[1]) + q[2]);
                    for (int a = 0; a < 3; ++a) r[a] = fmaf(q[2], poly[f + 1].a[a], fmaf(q[1], poly[f].a[a], q[0] * poly[0].a[a])) * rQ;
                }
                if (pass) lv[pass] = fminf(r[0], 1.0f);
                else {
                    memcpy(attr, r, sizeof r);
                    keep = drm_sample(img, iw, ih, x0, z0, sx, sz, linear, attr[1], attr[2], val) && val[3] * opacity > 0.0f;   /* item 6 */
                }
            }
            if (!keep) continue;
            frag_alb(&S, attr, lv[1], lv[2], val, opacity, rgba + 4 * o);
            rewritten[o] = 1;
            if (sample) { memcpy(sample + 6 * o, val, sizeof val); sample[6 * o + 4] = lv[1]; sample[6 * o + 5] = lv[2]; }
        }
    frame_free(&F);
    return 0;
}

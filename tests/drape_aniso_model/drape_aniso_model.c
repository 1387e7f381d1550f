/* drape_aniso_model.c -- CPU model of anisotropic filtering of the draped image's mip sampling, the contract the
 * gfx950 kernel of vulkan_forge_amd/csrc/vf_drape_aniso.h and vf_relight.h (k_relight<., kDrapeAniso>) is held to bit for bit.
 * Written from the contract, layered on the mip model (included below): the plan of a pixel from the two squared axis lengths of
 * its footprint, then the mean of its taps, each the mip model's sample at clamped texel coordinates.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC drape_aniso_model.c -o libdranisomodel.so -lm     (drape_aniso_model.py does this)
 */
#include "../drape_mip_model/drape_mip_model.c"

/* 4k item 3's bit procedure on a squared length, plus bias; -inf: level 0, +inf: the top level */
static float dam_lod_of(float rho2, float bias)
{
    uint32_t bits;
    memcpy(&bits, &rho2, 4);
    const uint32_t E = (bits >> 23) & 255u, Mn = bits & 0x7FFFFFu;
    if ((bits >> 31) != 0u || E == 0u || (E == 255u && Mn != 0u)) return -INFINITY;
    if (E == 255u) return INFINITY;
    return 0.5f * ((float)((int)E - 127) + (float)Mn * 0x1p-23f) + bias;
}

/* items 1 - 4 on the squared lengths ax, ay of the footprint's two screen axes: the major axis (0 = x, 1 = y), lod and N */
void dam_plan(float ax, float ay, uint32_t A, float bias, int *ymajor, float *lod, uint32_t *n)
{
    const float inv_a2 = 1.0f / (float)(A * A);
    *ymajor = ay > ax;
    const float amax = *ymajor ? ay : ax, amin = *ymajor ? ax : ay;
    if (!(amax > 1.5625f * amin)) { *lod = dam_lod_of(amax, bias); *n = 1u; return; }      /* item 2 */
    const float t = amax * inv_a2;
    const float m2 = amin > t ? amin : t;
    *lod = dam_lod_of(m2, bias);
    *n = A;
    for (uint32_t k = 1; k <= A; ++k)
        if (amax <= (float)(k * k) * m2) { *n = k; break; }
}

/* item 5: the offset of tap i of N along the major axis, in footprints */
float dam_offset(uint32_t n, uint32_t i)
{
    const float w = 1.0f / (float)n;
    return ((float)i + 0.5f) * w - 0.5f;
}

/* level k at level-0 texel coordinates (fu, fv) inside the image rectangle: level 0 is 4j's items 4 / 5 from (fu, fv) */
static void dam_level(const Mips *M, int k, float fu, float fv, float val[4])
{
    if (k != 0) { dmm_level(M, k, 0.0f, 0.0f, fu, fv, val); return; }
    const uint32_t iw = M->w[0], ih = M->h[0];
    const int mx = (int)iw - 1, my = (int)ih - 1;
    if (!M->linear) {
        int ix = (int)floorf(fu), iy = (int)floorf(fv);
        ix = ix < mx ? ix : mx; iy = iy < my ? iy : my;
        drm_texel(M->img, iw, ix, iy, val);
        return;
    }
    const float cu = fu - 0.5f, cv = fv - 0.5f;
    const float i0f = floorf(cu), j0f = floorf(cv);
    const float fx = cu - i0f, fy = cv - j0f;
    const int c0 = clampi((int)i0f, 0, mx), c1 = clampi((int)i0f + 1, 0, mx);
    const int r0 = clampi((int)j0f, 0, my), r1 = clampi((int)j0f + 1, 0, my);
    float q00[4], q01[4], q10[4], q11[4];
    drm_texel(M->img, iw, c0, r0, q00); drm_texel(M->img, iw, c1, r0, q01);
    drm_texel(M->img, iw, c0, r1, q10); drm_texel(M->img, iw, c1, r1, q11);
    for (int c = 0; c < 4; ++c) {
        const float top = fmaf(fx, q01[c] - q00[c], q00[c]);
        const float bot = fmaf(fx, q11[c] - q10[c], q10[c]);
        val[c] = fmaf(fy, bot - top, top);
    }
}

/* one tap: 4k items 4 - 6 at texel coordinates (fu, fv) with the pixel's lod */
static void dam_tap(const Mips *M, float fu, float fv, float lod, float val[4])
{
    if (!(lod > 0.0f)) { dam_level(M, 0, fu, fv, val); return; }
    const int top = (int)M->levels - 1;
    if (!M->linear) {
        const float ln = lod + 0.5f;
        dam_level(M, ln >= (float)top ? top : (int)floorf(ln), fu, fv, val);
        return;
    }
    if (lod >= (float)top) { dam_level(M, top, fu, fv, val); return; }
    const float lf = floorf(lod), t = lod - lf;
    const int l = (int)lf;
    float lo[4], hi[4];
    dam_level(M, l, fu, fv, lo);
    dam_level(M, l + 1, fu, fv, hi);
    for (int c = 0; c < 4; ++c) val[c] = fmaf(t, hi[c] - lo[c], lo[c]);
}

/* dmm_clipped_pixels per pixel: mask (H x W) is 1 where the covered pixel shows a primitive that the near or the far plane cuts */
int dam_clipped_mask(uint8_t *mask, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw, uint32_t th, uint32_t grid)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    for (size_t o = 0; o < (size_t)W * H; ++o) {
        mask[o] = 0;
        if (vis[o] == 0u) continue;
        const uint32_t prim = vis[o] - 1u, cell = prim >> 1, odd = prim & 1u;
        const uint32_t j = cell / F.nm1, i = cell - j * F.nm1;
        const uint32_t vi[3] = { odd ? i + 1u : i, i, i + 1u }, vj[3] = { j, j + 1u, odd ? j + 1u : j };
        for (int k = 0; k < 3; ++k) { const AVert v = attr_vertex(&F, vi[k], vj[k]); mask[o] |= v.c.z < 0.0f || v.c.z > v.c.w; }
    }
    frame_free(&F);
    return 0;
}

/* dmm_frame with the largest anisotropy A. sample (H x W x 10 floats, or NULL): dmm_frame's seven (lod is the plan's), then N, the
 * major axis (0 = x, 1 = y) and whether a tap was clamped to the image rectangle, of the pixels written again. */
int dam_frame(uint8_t *rgba, uint8_t *rewritten, float *sample, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex,
              uint32_t tw, uint32_t th, uint32_t grid, const uint8_t *lut_rgba8, int shade_mode, const uint8_t *img, uint32_t iw, uint32_t ih,
              const uint16_t *pyr, const float *extent, float opacity, int linear, float bias, uint32_t A, const float *lit, const float *sky,
              float strength)
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
            if (sample) for (int k = 0; k < 10; ++k) sample[10 * o + k] = 0.0f;
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
            uint32_t N = 1;
            int keep = 1, ymajor = 0, clamped = 0;
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
                /* 4k item 1: the varyings of that piece at the centres to the right and below (zero when no piece covers the pixel) */
                float nb[2][3] = { { 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f } };
                if (piece)
                    for (int d = 0; d < 2; ++d) {
                        float q[3];
                        tri_weights_at(&F, &poly[0].c, &poly[piece].c, &poly[piece + 1].c, (int32_t)px + (d == 0), (int32_t)py + (d == 1), q);
                        const float rQ = 1.0f / ((q[0] + q[1]) + q[2]);
                        for (int a = 0; a < 3; ++a) nb[d][a] = fmaf(q[2], poly[piece + 1].a[a], fmaf(q[1], poly[piece].a[a], q[0] * poly[0].a[a])) * rQ;
                    }
                const float x = attr[1], z = attr[2];
                const float fu = (x - M.x0) * M.sx, fv = (z - M.z0) * M.sz;
                if (!(fu >= 0.0f && fu <= (float)iw && fv >= 0.0f && fv <= (float)ih)) { keep = 0; break; }     /* the pixel's own inside test */
                /* item 1: the footprint, as 4k item 2 forms it */
                const float dux = (nb[0][1] - x) * M.sx, dvx = (nb[0][2] - z) * M.sz;
                const float ax = fmaf(dux, dux, dvx * dvx);
                const float duy = (nb[1][1] - x) * M.sx, dvy = (nb[1][2] - z) * M.sz;
                const float ay = fmaf(duy, duy, dvy * dvy);
                dam_plan(ax, ay, A, bias, &ymajor, &lod, &N);
                if (N == 1u) keep = dmm_sample(&M, x, z, lod, val);            /* items 2 and 4: 4k's sample at the pixel's own (x, z) */
                else {
                    const float dum = ymajor ? duy : dux, dvm = ymajor ? dvy : dvx;
                    const float w = 1.0f / (float)N;
                    float sum[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
                    for (uint32_t k = 0; k < N; ++k) {
                        const float off = ((float)k + 0.5f) * w - 0.5f;
                        const float su = fmaf(off, dum, fu), sv = fmaf(off, dvm, fv);
                        const float fuk = fminf(fmaxf(su, 0.0f), (float)iw), fvk = fminf(fmaxf(sv, 0.0f), (float)ih);
                        clamped |= !(fuk == su) || !(fvk == sv);
                        float q[4];
                        dam_tap(&M, fuk, fvk, lod, q);
                        for (int c = 0; c < 4; ++c) sum[c] = k ? sum[c] + q[c] : q[c];
                    }
                    for (int c = 0; c < 4; ++c) val[c] = sum[c] * w;
                }
                keep = keep && val[3] * opacity > 0.0f;
            }
            if (!keep) continue;
            frag_alb(&S, attr, lv[1], lv[2], val, opacity, rgba + 4 * o);
            rewritten[o] = 1;
            if (sample) {
                float *sp = sample + 10 * o;
                memcpy(sp, val, sizeof val); sp[4] = lv[1]; sp[5] = lv[2]; sp[6] = lod;
                sp[7] = (float)N; sp[8] = (float)ymajor; sp[9] = (float)clamped;
            }
        }
    frame_free(&F);
    return 0;
}

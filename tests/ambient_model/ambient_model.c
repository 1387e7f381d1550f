/* ambient_model.c -- CPU model of ambient occlusion from a sky-view scan, the contract the gfx950 kernels of
 * vulkan_forge_amd/csrc/vf_ambient.h (k_ambient_dir) and vf_relight.h (k_relight<., kAmbient>) are held to bit for bit.  Written from the contract: the field
 * is the plain walk over every direction, every sheared line of it (the lines of DESIGN.md 4g) and every vertex's R_t predecessors,
 * with no tiles and no table; the frame takes a frame and its visibility ids, interpolates lit and amb of every covered pixel as the
 * shadow model interpolates lit (included below) and shades the pixels where either is below 1 again with a restatement of fs_main
 * in which lambert is multiplied by lit and shade by amb.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC ambient_model.c -o libabmodel.so -lm     (ambient_model.py does this)
 */
#include "../shadow_model/shadow_model.c"

/* ---- the field (contract items 1-5) ---- */

/* sky (n x n, row j = z index, column i = x index) from the vertex heights h (same layout, before exaggeration) and D directions
 * dirs[2 t] = ux_t, dirs[2 t + 1] = uz_t; -1: a direction with no horizontal part or a non-finite one */
int abm_field_heights(float *sky, const float *h, uint32_t n, const float *dirs, uint32_t D, float spacing, float exag, float reach)
{
    const float step = (2.0f * 1.5f) / ((float)n - 1.0f);
    for (uint32_t t = 0; t < D; ++t) {
        /* item 2: the lines of 4g with the sun's horizontal part set to the direction */
        const float sx = dirs[2u * t], sz = dirs[2u * t + 1u];
        const float ax = fabsf(sx), az = fabsf(sz);
        const int zmajor = az > ax;                               /* a tie goes to x */
        const float amaj = zmajor ? az : ax, amin = zmajor ? ax : az;
        const float smaj = zmajor ? sz : sx, smin = zmajor ? sx : sz;
        if (!(amaj > 0.0f) || !isfinite(amaj) || !(amin <= amaj)) return -1;
        const int from_high = smaj > 0.0f, s = smin < 0.0f ? -1 : 1;
        const float a = amin / amaj;
        const int32_t Rs = (int32_t)rintf((float)(n - 1u) * a);
        /* item 3: distances */
        const float g = sqrtf(fmaf(a, a, 1.0f));
        const float ell = (step * spacing) * g;
        const float rf = floorf(reach / g);
        const uint32_t R = rf >= 1.0f ? (uint32_t)rf : 1u;
        for (int32_t c = s > 0 ? 0 : -Rs; c <= (s > 0 ? (int32_t)n - 1 + Rs : (int32_t)n - 1); ++c)
            for (uint32_t k = 0; k < n; ++k) {
                const int32_t minor = c - s * (int32_t)rintf((float)k * a);
                if (minor < 0 || minor >= (int32_t)n) continue;
                const uint32_t major = from_high ? n - 1u - k : k;
                const size_t o = zmajor ? (size_t)major * n + (size_t)minor : (size_t)minor * n + major;
                const float y = h[o] * exag;
                float occ = 0.0f;
                if (isfinite(y)) {
                    /* item 4: the horizon over the steps k - m that exist and are finite (fmaxf leaves a NaN product out) */
                    float T = 0.0f;
                    for (uint32_t m = 1; m <= R && m <= k; ++m) {
                        const int32_t mi = c - s * (int32_t)rintf((float)(k - m) * a);
                        if (mi < 0 || mi >= (int32_t)n) continue;
                        const uint32_t ma = from_high ? n - 1u - (k - m) : k - m;
                        const float y2 = h[zmajor ? (size_t)ma * n + (size_t)mi : (size_t)mi * n + ma] * exag;
                        if (!isfinite(y2)) continue;
                        const float inv = 1.0f / ((float)m * ell);
                        T = fmaxf(T, (y2 - y) * inv);
                    }
                    occ = 1.0f - 1.0f / (1.0f + T * T);
                }
                sky[o] = t == 0u ? occ : sky[o] + occ;            /* item 5: the sum in index order */
            }
    }
    for (size_t k = 0; k < (size_t)n * n; ++k) sky[k] = fmaxf(1.0f - sky[k] / (float)D, 0.0f);
    return 0;
}

/* ---- the shade pass (contract item 6) ---- */

/* fs_main + Rgba8UnormSrgb store with lambert * lit and shade * amb (frag_lit of the shadow model with one more product) */
static void frag_amb(const Shade *S, const float attr[3], float lit, float amb, uint8_t out[4])
{
    const float height = attr[0], x = attr[1], z = attr[2];
    float t = 0.5f + height / (2.0f * S->h_range);
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const float c = t * 256.0f - 0.5f;
    const float i0f = floorf(c);
    const float f = c - i0f;
    int i0 = (int)i0f, i1 = i0 + 1;
    i0 = i0 < 0 ? 0 : (i0 > 255 ? 255 : i0);
    i1 = i1 < 0 ? 0 : (i1 > 255 ? 255 : i1);
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
        int tx0 = (int)floorf(uu * (float)S->tw), tx1 = (int)floorf((uu + du) * (float)S->tw);
        int ty0 = (int)floorf(vv * (float)S->th), ty1 = (int)floorf((vv + dv) * (float)S->th);
        const int mx = (int)S->tw - 1, my = (int)S->th - 1;
        tx0 = tx0 < 0 ? 0 : (tx0 > mx ? mx : tx0); tx1 = tx1 < 0 ? 0 : (tx1 > mx ? mx : tx1);
        ty0 = ty0 < 0 ? 0 : (ty0 > my ? my : ty0); ty1 = ty1 < 0 ? 0 : (ty1 > my ? my : ty1);
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
        float v = lc * S->exposure * shade;
        if (S->shade_mode != 0) v = v / (1.0f + v);
        out[ch] = (uint8_t)ovm_encode(v);
    }
    out[3] = 255;
}

/* rgba (H x W x 4, the plain frame) -> the frame with ambient occlusion (and cast shadows where lit is not NULL), in place;
 * rewritten (H x W): 1 where a pixel's lit or amb is below 1.  sky, lit: the fields (n x n).  lut_rgba8: the handle's 256 sRGB texels. */
int abm_frame(uint8_t *rgba, uint8_t *rewritten, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw,
              uint32_t th, uint32_t grid, const uint8_t *lut_rgba8, int shade_mode, const float *lit, const float *sky, float strength)
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
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const size_t o = (size_t)py * W + px;
            rewritten[o] = 0;
            const uint32_t id = vis[o];
            if (id == 0u) continue;
            const uint32_t prim = id - 1u, cell = prim >> 1, odd = prim & 1u;
            const uint32_t j = cell / F.nm1, i = cell - j * F.nm1;
            const uint32_t vi[3] = { odd ? i + 1u : i, i, i + 1u }, vj[3] = { j, j + 1u, odd ? j + 1u : j };
            float l[3], am[3];
            for (int k = 0; k < 3; ++k) {
                const size_t v = (size_t)vj[k] * F.n + vi[k];
                l[k] = lit ? lit[v] : 1.0f;
                am[k] = 1.0f - strength * (1.0f - sky[v]);
            }
            const int plain_l = l[0] == 1.0f && l[1] == 1.0f && l[2] == 1.0f, plain_a = am[0] == 1.0f && am[1] == 1.0f && am[2] == 1.0f;
            if (plain_l && plain_a) continue;                                 /* item 6: 1 without interpolation */
            AVert v[3], poly[8];
            float attr[3] = { 0.0f, 0.0f, 0.0f }, val[3] = { 0.0f, 1.0f, 1.0f };
            for (int pass = 0; pass < 3; ++pass) {                            /* the varyings (h, x, z), then lit, then amb in the place of h */
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
                if (pass) val[pass] = r[0];
                else memcpy(attr, r, sizeof r);
            }
            if (!(val[1] < 1.0f) && !(val[2] < 1.0f)) continue;
            /* an interpolated value an ulp above 1 shades as 1 */
            frag_amb(&S, attr, fminf(val[1], 1.0f), fminf(val[2], 1.0f), rgba + 4 * o);
            rewritten[o] = 1;
        }
    frame_free(&F);
    return 0;
}

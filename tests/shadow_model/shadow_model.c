/* shadow_model.c -- CPU model of cast sun shadows, the contract the gfx950 kernels of
 * vulkan_forge_amd/csrc/vf_shadow.h (k_shadow_chunk_max / _carry / _lit) and vf_relight.h (k_relight) are held to bit for bit.  Written from the
 * contract: the field is the plain sequential walk along every sheared line, with no scan; the shadowed frame takes a frame and its
 * visibility ids, interpolates the three vertex values of every covered pixel with the geometry-buffer model's weights (included
 * below: clip, fan, last covering piece) and shades the pixels below 1 again with a restatement of fs_main and the sRGB store
 * (terrain.wgsl:69-91) in which lambert is multiplied by lit.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC shadow_model.c -o libshmodel.so -lm     (shadow_model.py does this)
 */
#include "../gbuffer_model/gbuffer_model.c"

/* ---- the field (contract items 1-3) ---- */

/* lit (n x n, row j = z index, column i = x index) from the vertex heights h (same layout, before exaggeration) */
int shm_field_heights(float *lit, const float *h, uint32_t n, const float *sun, float spacing, float exag, float strength, float softness, float bias)
{
    for (size_t k = 0; k < (size_t)n * n; ++k) lit[k] = 1.0f;
    /* item 1: axis, signs and the two ratios, from the sun vector as given */
    const float sx = sun[0], sy = sun[1], sz = sun[2];
    const float ax = fabsf(sx), az = fabsf(sz);
    const int zmajor = az > ax;                               /* a tie goes to x */
    const float amaj = zmajor ? az : ax, amin = zmajor ? ax : az;
    const float smaj = zmajor ? sz : sx, smin = zmajor ? sx : sz;
    if (!(amaj > 0.0f) || !isfinite(amaj) || !(amin <= amaj) || !isfinite(sy)) return 0;
    const float step = (2.0f * 1.5f) / ((float)n - 1.0f);
    const float d = sy > 0.0f ? ((step * spacing) * sy) / amaj : 0.0f;
    if (!isfinite(d)) return 0;
    const int from_high = smaj > 0.0f, s = smin < 0.0f ? -1 : 1;
    const float a = amin / amaj;
    const int32_t R = (int32_t)rintf((float)(n - 1u) * a);
    /* items 2 and 3: every line, from its sun-side end */
    for (int32_t c = s > 0 ? 0 : -R; c <= (s > 0 ? (int32_t)n - 1 + R : (int32_t)n - 1); ++c) {
        float run = -INFINITY;                                /* max over the steps before this one of y_j + j d */
        for (uint32_t k = 0; k < n; ++k) {
            const int32_t minor = c - s * (int32_t)rintf((float)k * a);
            if (minor < 0 || minor >= (int32_t)n) continue;
            const uint32_t major = from_high ? n - 1u - k : k;
            const size_t o = zmajor ? (size_t)major * n + (size_t)minor : (size_t)minor * n + major;
            const float y = h[o] * exag;
            if (!isfinite(y)) continue;                       /* occludes nothing, is lit */
            const float e = (run - (float)k * d) - y;
            const float cl = fminf(fmaxf((e - bias) / softness, 0.0f), 1.0f);
            lit[o] = 1.0f - strength * cl;
            run = fmaxf(run, y + (float)k * d);
        }
    }
    return 0;
}

/* the displaced heights the renderer draws: h_tex + h_ana on its own vertices (n x n) */
int shm_heights(float *h, const float *u, const float *tex, uint32_t tw, uint32_t th, uint32_t grid)
{
    Frame F;
    if (frame_init(&F, 1, 1, u, tex, tw, th, grid)) return -1;
    for (uint32_t j = 0; j < F.n; ++j)
        for (uint32_t i = 0; i < F.n; ++i) h[(size_t)j * F.n + i] = height_at(&F, i, j);
    frame_free(&F);
    return 0;
}

/* ---- the shade pass (contract item 4) ---- */

typedef struct { float h_range, exposure, Lx, Ly, Lz; float lut[256][3]; int shade_mode; const float *tex; uint32_t tw, th; float spacing, exag; } Shade;

/* fs_main + Rgba8UnormSrgb store with lambert * lit */
static void frag_lit(const Shade *S, const float attr[3], float lit, uint8_t out[4])
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
    const float shade = 0.15f * (1.0f - lambert) + lambert;
    for (int ch = 0; ch < 3; ++ch) {
        const float l0 = S->lut[i0][ch], l1 = S->lut[i1][ch];
        const float lc = fmaf(f, l1 - l0, l0);
        float v = lc * S->exposure * shade;
        if (S->shade_mode != 0) v = v / (1.0f + v);
        out[ch] = (uint8_t)ovm_encode(v);
    }
    out[3] = 255;
}

/* rgba (H x W x 4, the unshadowed frame) -> the shadowed frame, in place; shadowed (H x W): 1 where a pixel's lit is below 1.
 * lit: the field (n x n).  lut_rgba8: the handle's 256 sRGB texels. */
int shm_frame(uint8_t *rgba, uint8_t *shadowed, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw,
              uint32_t th, uint32_t grid, const uint8_t *lut_rgba8, int shade_mode, const float *lit)
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
            shadowed[o] = 0;
            const uint32_t id = vis[o];
            if (id == 0u) continue;
            const uint32_t prim = id - 1u, cell = prim >> 1, odd = prim & 1u;
            const uint32_t j = cell / F.nm1, i = cell - j * F.nm1;
            const uint32_t vi[3] = { odd ? i + 1u : i, i, i + 1u }, vj[3] = { j, j + 1u, odd ? j + 1u : j };
            float l[3];
            for (int k = 0; k < 3; ++k) l[k] = lit[(size_t)vj[k] * F.n + vi[k]];
            if (l[0] == 1.0f && l[1] == 1.0f && l[2] == 1.0f) continue;       /* item 4: lit without interpolation */
            AVert v[3], poly[8];
            float attr[3] = { 0.0f, 0.0f, 0.0f }, val = 0.0f;
            for (int pass = 0; pass < 2; ++pass) {                            /* the varyings (h, x, z), then lit in the place of h */
                for (int k = 0; k < 3; ++k) { v[k] = attr_vertex(&F, vi[k], vj[k]); if (pass) v[k].a[0] = l[k]; }
                const int np = clip_attr(v, poly);
                float r[3] = { 0.0f, 0.0f, 0.0f };
                for (int f = 1; f + 1 < np; ++f) {
                    float q[3];
                    if (!tri_weights(&F, &poly[0].c, &poly[f].c, &poly[f + 1].c, (int32_t)px, (int32_t)py, q)) continue;
                    const float rQ = 1.0f / ((q[0] + q[1]) + q[2]);
                    for (int a = 0; a < 3; ++a) r[a] = fmaf(q[2], poly[f + 1].a[a], fmaf(q[1], poly[f].a[a], q[0] * poly[0].a[a])) * rQ;
                }
                if (pass) val = r[0];
                else memcpy(attr, r, sizeof r);
            }
            if (!(val < 1.0f)) continue;
            frag_lit(&S, attr, val, rgba + 4 * o);
            shadowed[o] = 1;
        }
    frame_free(&F);
    return 0;
}

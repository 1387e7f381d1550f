/* haze_model.c -- CPU model of the atmospheric haze pass, the contract the gfx950 kernel of
 * vulkan_forge_amd/csrc/vf_haze.h (k_haze) is held to bit for bit.  Written from the contract: per pixel the view depth and the world
 * height of the surface point come from the geometry-buffer model (gb_pixel: clip, fan, last covering piece), the opacity from the
 * arithmetic below, the blend is the viewshed model's.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC haze_model.c -o libhzmodel.so -lm     (haze_model.py does this)
 *
 * Every float operation is a binary32 one in the order written (-ffp-contract=off; fmaf only where written). */
#include "../gbuffer_model/gbuffer_model.c"

/* ---- item 8: det_exp(x), x in [-87, 16] (callers clamp) ----
 * n = rintf(x log2e); r = x - n ln2 in two fmaf (ln2 split: the high part has nine significant bits, n ln2_hi is exact);
 * exp(r) = 1 + (r + r^2 p(r)), p of degree 5 (the coefficients of Cephes' expf), a Horner chain in fmaf; times 2^n built from bits.
 * Measured against float64 exp on the sweep of tests/test_haze_model.py: at most 1 ulp. */
float hzm_det_exp(float x)
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

void hzm_det_exp_n(float *out, const float *x, uint32_t n) { for (uint32_t k = 0; k < n; ++k) out[k] = hzm_det_exp(x[k]); }

/* ---- item 4: the eye's height, y of -R^T t of the column-major view matrix ---- */
float hzm_eye_y(const float *u)
{
    return -fmaf(u[6], u[14], fmaf(u[5], u[13], u[4] * u[12]));
}

/* ---- item 3: the height factor ----
 * The mean of exp(-(y - base) / falloff) along the straight line from the eye's height to the point's:
 * E_e (1 - exp(-s)) / s with s = k_p - k_e.  |s| < 1/2: its series to s^8, an fmaf Horner chain (truncation below 2^-30 relative);
 * otherwise the difference of two det_exp over s.  branch: -1 as the contract chooses, 0 the series, 1 the difference. */
#define HZ_SERIES_BELOW 0.5f
float hzm_g_branch(float k_e, float k_p, int branch)
{
    const float s = k_p - k_e;
    const float E_e = hzm_det_exp(-k_e);
    if (branch < 0) branch = fabsf(s) < HZ_SERIES_BELOW ? 0 : 1;
    if (branch == 0) {
        float t = fmaf(s, 2.7557319224e-6f, -2.4801587302e-5f);      /* 1/9!, -1/8! */
        t = fmaf(s, t, 1.9841269841e-4f);                            /* 1/7! */
        t = fmaf(s, t, -1.3888888889e-3f);                           /* -1/6! */
        t = fmaf(s, t, 8.3333333333e-3f);                            /* 1/5! */
        t = fmaf(s, t, -4.1666666667e-2f);                           /* -1/4! */
        t = fmaf(s, t, 1.6666666667e-1f);                            /* 1/3! */
        t = fmaf(s, t, -0.5f);
        t = fmaf(s, t, 1.0f);
        return E_e * t;
    }
    return (E_e - hzm_det_exp(-k_p)) / s;
}

static float hz_clamp_k(float k) { return fminf(fmaxf(k, -16.0f), 64.0f); }

float hzm_g(float eye_y, float y, float falloff, float base)
{
    if (!(falloff > 0.0f)) return 1.0f;
    return hzm_g_branch(hz_clamp_k((eye_y - base) / falloff), hz_clamp_k((y - base) / falloff), -1);
}

/* which branch a surface point takes: -1 uniform haze, 0 the series, 1 the difference */
int hzm_g_which(float eye_y, float y, float falloff, float base)
{
    if (!(falloff > 0.0f)) return -1;
    const float s = hz_clamp_k((y - base) / falloff) - hz_clamp_k((eye_y - base) / falloff);
    return fabsf(s) < HZ_SERIES_BELOW ? 0 : 1;
}

/* ---- items 1, 2, 5: the opacity of a surface point at view depth d and height y; 0: the pixel is untouched ---- */
float hzm_alpha(float d, float y, float eye_y, float density, float start, float falloff, float base, float max_opacity, uint32_t alpha8)
{
    if (!isfinite(d)) return 0.0f;
    const float l = fmaxf(d - start, 0.0f);
    if (!(l > 0.0f)) return 0.0f;
    const float g = hzm_g(eye_y, y, falloff, base);
    const float tau = (density * l) * g;
    const float a0 = 1.0f - hzm_det_exp(-fminf(tau, 87.0f));
    const float a = fminf(a0, max_opacity) * ((float)alpha8 / 255.0f);
    return a > 0.0f ? a : 0.0f;
}

/* ---- item 6: the blend of one pixel's three colour bytes, in linear light ---- */
void hzm_blend(uint8_t *px, uint32_t haze_rgba, float a)
{
    for (int k = 0; k < 3; ++k) {
        const float c = ovm_decode(px[k]);
        px[k] = (uint8_t)ovm_encode(ovm_decode((haze_rgba >> (8 * k)) & 255u) * a + c * (1.0f - a));
    }
}

/* rgba (H x W x 4, the frame without haze) -> the hazed frame, in place; opacity (H x W): a, 0 where the pass leaves the pixel;
 * which (H x W, may be NULL): -2 background, else hzm_g_which of the pixel */
int hzm_frame(uint8_t *rgba, float *opacity, int8_t *which, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw,
              uint32_t th, uint32_t grid, float density, uint32_t haze_rgba, float start, float falloff, float base, float max_opacity, int background)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    const float eye_y = hzm_eye_y(u);
    const uint32_t alpha8 = haze_rgba >> 24;
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const size_t o = (size_t)py * W + px;
            const uint32_t id = vis[o];
            opacity[o] = 0.0f;
            if (which) which[o] = -2;
            if (id == 0u) {                                              /* item 7 */
                if (!background) continue;
                const float a = max_opacity * ((float)alpha8 / 255.0f);
                if (!(a > 0.0f)) continue;
                opacity[o] = a;
                hzm_blend(rgba + 4 * o, haze_rgba, a);
                continue;
            }
            const GPixel g = gb_pixel(&F, id, (int32_t)px, (int32_t)py);
            if (which) which[o] = (int8_t)hzm_g_which(eye_y, g.pos[1], falloff, base);
            const float a = hzm_alpha(g.depth, g.pos[1], eye_y, density, start, falloff, base, max_opacity, alpha8);
            if (!(a > 0.0f)) continue;
            opacity[o] = a;
            hzm_blend(rgba + 4 * o, haze_rgba, a);
            rgba[4 * o + 3] = 255;
        }
    frame_free(&F);
    return 0;
}

/* viewshed_model.c -- CPU model of the viewshed analysis, the contract the gfx950 kernels of
 * vulkan_forge_amd/csrc/vf_viewshed.h (k_viewshed_chunk_max / _carry / _seen / _tint) are held to bit for bit.  Written from the
 * contract: the field is the plain sequential walk along every line of every quadrant, with no scan; the tinted frame takes a frame and
 * its visibility ids, interpolates the three vertex values of every covered pixel with the geometry-buffer model's weights (clip, fan,
 * last covering piece) and blends the two tints as the overlay model blends a feature.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC viewshed_model.c -o libvsmodel.so -lm     (viewshed_model.py does this)
 */
#include "../shadow_model/shadow_model.c"

/* ---- the field (contract items 1-3) ---- */

/* item 1: the observer's vertex from a world coordinate of the overlays' frame */
uint32_t vsm_observer_index(float x, float spacing, uint32_t n)
{
    const float step = (2.0f * 1.5f) / ((float)n - 1.0f);
    float mx = x / spacing;
    mx = fminf(fmaxf(mx, -1.5f), 1.5f);
    const float gx = (mx + 1.5f) / step;
    const uint32_t i = (uint32_t)rintf(gx);
    return i < n - 1u ? i : n - 1u;
}

/* item 2: minor offset of step k of line c, and the line that owns the vertex (k, m) */
int32_t vsm_minor(uint32_t L, int32_t c, uint32_t k)
{
    const uint32_t ac = (uint32_t)(c < 0 ? -c : c);
    const int32_t r = (int32_t)((2u * k * ac + L) / (2u * L));
    return c < 0 ? -r : r;
}

int32_t vsm_owner(uint32_t L, uint32_t k, int32_t m)
{
    const uint32_t am = (uint32_t)(m < 0 ? -m : m);
    const int32_t c = (int32_t)((2u * am * L + k) / (2u * k));
    return m < 0 ? -c : c;
}

/* seen (n x n, row j = z index, column i = x index) from the vertex heights h (same layout, before exaggeration) and the observer's
 * vertex (io, jo).  writers, when not NULL, counts the stores to every vertex (the ownership property: 1 everywhere). */
int vsm_field_heights(float *seen, uint32_t *writers, const float *h, uint32_t n, uint32_t io, uint32_t jo, float exag, float eye_height,
                      float target_height, float softness, float bias)
{
    if (n < 2u || io >= n || jo >= n) return -1;
    for (size_t k = 0; k < (size_t)n * n; ++k) seen[k] = 1.0f;
    if (writers) { memset(writers, 0, (size_t)n * n * sizeof *writers); writers[(size_t)jo * n + io] = 1u; }
    const float y_obs = h[(size_t)jo * n + io] * exag;
    const int blind = !isfinite(y_obs);                      /* the whole field is 1 */
    const float y_eye = y_obs + eye_height;
    const uint32_t L = n - 1u;
    const uint32_t steps[4] = { n - 1u - io, io, n - 1u - jo, jo };
    for (uint32_t q = 0; q < 4u; ++q) {
        const int zmajor = q >= 2u;
        const int32_t o_major = (int32_t)(zmajor ? jo : io), o_minor = (int32_t)(zmajor ? io : jo), dir = (q & 1u) ? -1 : 1;
        for (int32_t c = -(int32_t)L; c <= (int32_t)L; ++c) {
            float run = -INFINITY;                            /* max over the steps before this one of t_j */
            for (uint32_t k = 1; k <= steps[q]; ++k) {
                const int32_t r = vsm_minor(L, c, k);
                const int32_t minor = o_minor + r;
                if (minor < 0 || minor >= (int32_t)n) break;  /* |r| does not shrink: the line has left the grid */
                const int32_t major = o_major + dir * (int32_t)k;
                const size_t o = zmajor ? (size_t)major * n + (size_t)minor : (size_t)minor * n + (size_t)major;
                const float D = sqrtf((float)(k * k + (uint32_t)(r * r)));
                const float y = h[o] * exag;
                const uint32_t ar = (uint32_t)(r < 0 ? -r : r);
                const int owned = (zmajor ? ar < k : 1) && vsm_owner(L, k, r) == c;
                if (owned && writers) writers[o]++;
                if (!isfinite(y)) continue;                   /* contributes nothing, is seen */
                if (owned && !blind) {
                    const float s = ((y + target_height) - y_eye) / D;
                    const float e = (run - s) * D;
                    seen[o] = 1.0f - fminf(fmaxf((e - bias) / softness, 0.0f), 1.0f);
                }
                run = fmaxf(run, (y - y_eye) / D);
            }
        }
    }
    return 0;
}

/* ---- the tint pass (contract item 4) ---- */

static int vsm_blend(float c[3], uint32_t rgba, float cov)
{
    const float a = cov * ((float)(rgba >> 24) / 255.0f);
    if (!(a > 0.0f)) return 0;
    for (int k = 0; k < 3; ++k) c[k] = ovm_decode((rgba >> (8 * k)) & 255u) * a + c[k] * (1.0f - a);
    return 1;
}

/* rgba (H x W x 4, the untinted frame) -> the tinted frame, in place.  sval (H x W): the pixel's seen value s, -1 where the pass does
 * not treat the pixel (background, or outside the radius).  seen: the field (n x n); radius in world units, 0: none. */
int vsm_frame(uint8_t *rgba, float *sval, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex, uint32_t tw,
              uint32_t th, uint32_t grid, const float *seen, uint32_t io, uint32_t jo, float radius, uint32_t visible_rgba, uint32_t hidden_rgba)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    const float xo = -1.5f + (float)io * F.step, zo = -1.5f + (float)jo * F.step;
    const float R = radius / F.spacing, RR = R * R;
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const size_t o = (size_t)py * W + px;
            sval[o] = -1.0f;
            const uint32_t id = vis[o];
            if (id == 0u) continue;
            const uint32_t prim = id - 1u, cell = prim >> 1, odd = prim & 1u;
            const uint32_t j = cell / F.nm1, i = cell - j * F.nm1;
            const uint32_t vi[3] = { odd ? i + 1u : i, i, i + 1u }, vj[3] = { j, j + 1u, odd ? j + 1u : j };
            float l[3];
            for (int k = 0; k < 3; ++k) l[k] = seen[(size_t)vj[k] * F.n + vi[k]];
            const int plain = l[0] == 1.0f && l[1] == 1.0f && l[2] == 1.0f;
            AVert v[3], poly[8];
            float attr[3] = { 0.0f, 0.0f, 0.0f }, val = 0.0f;
            for (int pass = 0; pass < 2; ++pass) {                            /* the varyings (h, x, z), then seen in the place of h */
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
            if (radius > 0.0f) {
                const float dx = attr[1] - xo, dz = attr[2] - zo;
                const float d2 = dx * dx + dz * dz;
                if (!(d2 <= RR)) continue;
            }
            const float s = plain ? 1.0f : fminf(fmaxf(val, 0.0f), 1.0f);
            sval[o] = s;
            float c[3];
            for (int k = 0; k < 3; ++k) c[k] = ovm_decode(rgba[4 * o + k]);
            const int hid = vsm_blend(c, hidden_rgba, 1.0f - s);
            const int see = vsm_blend(c, visible_rgba, s);
            if (!hid && !see) continue;
            for (int k = 0; k < 3; ++k) rgba[4 * o + k] = (uint8_t)ovm_encode(c[k]);
            rgba[4 * o + 3] = 255;
        }
    frame_free(&F);
    return 0;
}

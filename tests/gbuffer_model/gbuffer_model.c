/* gbuffer_model.c -- CPU model of the geometry-buffer pass, the contract the gfx950 kernels of
 * vulkan_forge_amd/csrc/vf_gbuffer.h (k_gbuffer, k_gbuffer_pick) are held to bit for bit.  Written from the contract: depth, world
 * position and geometric normal at every pixel come from the visibility ids and a restatement of the vertex stage, the clipper and
 * the coverage rule (the occlusion model's, included below); every primitive takes the generic path (clip, fan, last covering
 * piece), which for an unclipped primitive is the same arithmetic as the kernels' vertex-record path.  The clipper is stated again
 * here because the varyings (h, x, z) have to pass through it beside the clip coordinates.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC gbuffer_model.c -o libgbmodel.so -lm     (gbuffer_model.py does this)
 */
#include "../occlusion_model/occlusion_model.c"

/* a clip-space vertex with its varyings: height, x, z (terrain.wgsl:63-64) */
typedef struct { CVert c; float a[3]; } AVert;

static AVert attr_vertex(const Frame *F, uint32_t i, uint32_t j)
{
    AVert v;
    v.c = terrain_vertex(F, i, j);
    v.a[0] = height_at(F, i, j);
    v.a[1] = -1.5f + (float)i * F->step;
    v.a[2] = -1.5f + (float)j * F->step;
    return v;
}

/* clip_tri with the varyings carried along: a crossing's varyings are fma(t, out - in, in), as its clip coordinates */
static int clip_attr(const AVert v[3], AVert poly[8])
{
    for (int k = 0; k < 3; ++k)
        if (!(isfinite(v[k].c.x) && isfinite(v[k].c.y) && isfinite(v[k].c.z) && isfinite(v[k].c.w))) return 0;
    int out_near = 0, out_far = 0;
    for (int k = 0; k < 3; ++k) { out_near += v[k].c.z < 0.0f; out_far += v[k].c.z > v[k].c.w; }
    if (out_near == 3 || out_far == 3) return 0;
    for (int k = 0; k < 3; ++k) poly[k] = v[k];
    if (out_near == 0 && out_far == 0) return 3;
    AVert tmp[8];
    int n = 3;
    for (int plane = 0; plane < 2; ++plane) {
        int m = 0;
        for (int k = 0; k < n; ++k) {
            const AVert *cur = &poly[k], *nxt = &poly[(k + 1) % n];
            const float dc = plane_d(&cur->c, plane), dn = plane_d(&nxt->c, plane);
            const int cin = dc >= 0.0f, nin = dn >= 0.0f;
            if (cin) tmp[m++] = *cur;
            if (cin != nin) {
                const AVert *in = cin ? cur : nxt, *ou = cin ? nxt : cur;
                const float di = cin ? dc : dn, dou = cin ? dn : dc;
                const float t = di / (di - dou);
                AVert r;
                r.c.x = fmaf(t, ou->c.x - in->c.x, in->c.x);
                r.c.y = fmaf(t, ou->c.y - in->c.y, in->c.y);
                r.c.z = fmaf(t, ou->c.z - in->c.z, in->c.z);
                r.c.w = fmaf(t, ou->c.w - in->c.w, in->c.w);
                for (int a = 0; a < 3; ++a) r.a[a] = fmaf(t, ou->a[a] - in->a[a], in->a[a]);
                tmp[m++] = r;
            }
        }
        n = m;
        for (int k = 0; k < n; ++k) poly[k] = tmp[k];
        if (n < 3) return 0;
    }
    return n;
}

/* tri_q with the three perspective weights handed out: 1 if the (sub-)triangle is front-facing and covers the pixel centre */
static int tri_weights(const Frame *F, const CVert *a, const CVert *b, const CVert *c, int32_t px, int32_t py, float q[3])
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
    for (int k = 0; k < 3; ++k) {
        const int s = (k + 1) % 3, t = (k + 2) % 3;
        e[k] = -((int64_t)(X[t] - X[s]) * (Py - Y[s]) - (int64_t)(Y[t] - Y[s]) * (Px - X[s]));
        const int32_t ea = Y[t] - Y[s], eb = -(X[t] - X[s]);
        if (!(e[k] > 0 || (e[k] == 0 && (ea > 0 || (ea == 0 && eb > 0))))) return 0;
    }
    const float fA = (float)(-area2);
    for (int k = 0; k < 3; ++k) q[k] = ((float)e[k] / fA) * rw[k];
    return 1;
}

/* the eight words of one pixel: depth, position, normal, id */
typedef struct { float depth, pos[3], nrm[3]; uint32_t id; } GPixel;

static GPixel gb_pixel(const Frame *F, uint32_t id, int32_t px, int32_t py)
{
    GPixel g = { INFINITY, { 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f }, id };
    if (id == 0u) return g;
    const uint32_t prim = id - 1u, cell = prim >> 1, odd = prim & 1u;
    const uint32_t j = cell / F->nm1, i = cell - j * F->nm1;
    const uint32_t vi[3] = { odd ? i + 1u : i, i, i + 1u }, vj[3] = { j, j + 1u, odd ? j + 1u : j };
    AVert v[3], poly[8];
    for (int k = 0; k < 3; ++k) v[k] = attr_vertex(F, vi[k], vj[k]);
    /* steps 1-4: weights of the last covering piece, depth = 1 / Q, varyings, position */
    const int np = clip_attr(v, poly);
    float Q = 0.0f, attr[3] = { 0.0f, 0.0f, 0.0f };
    for (int f = 1; f + 1 < np; ++f) {
        float q[3];
        if (!tri_weights(F, &poly[0].c, &poly[f].c, &poly[f + 1].c, px, py, q)) continue;
        Q = (q[0] + q[1]) + q[2];
        const float rQ = 1.0f / Q;
        for (int a = 0; a < 3; ++a) attr[a] = fmaf(q[2], poly[f + 1].a[a], fmaf(q[1], poly[f].a[a], q[0] * poly[0].a[a])) * rQ;
    }
    g.depth = 1.0f / Q;
    g.pos[0] = attr[1] * F->spacing; g.pos[1] = attr[0] * F->exag; g.pos[2] = attr[2] * F->spacing;
    /* step 5: the geometric normal of the unclipped primitive */
    float P[3][3];
    for (int k = 0; k < 3; ++k) { P[k][0] = v[k].a[1] * F->spacing; P[k][1] = v[k].a[0] * F->exag; P[k][2] = v[k].a[2] * F->spacing; }
    const float ax = P[1][0] - P[0][0], ay = P[1][1] - P[0][1], az = P[1][2] - P[0][2];
    const float bx = P[2][0] - P[0][0], by = P[2][1] - P[0][1], bz = P[2][2] - P[0][2];
    float nx = fmaf(ay, bz, -(az * by)), ny = fmaf(az, bx, -(ax * bz)), nz = fmaf(ax, by, -(ay * bx));
    if (ny < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    const float len = sqrtf(fmaf(nz, nz, fmaf(ny, ny, nx * nx)));
    if (len > 0.0f && isfinite(len)) { g.nrm[0] = nx / len; g.nrm[1] = ny / len; g.nrm[2] = nz / len; }
    return g;
}

/* depth (H x W), position and normal (H x W x 3) from the visibility ids; any plane may be NULL */
int gbm_planes(float *depth, float *position, float *normal, const uint32_t *vis, uint32_t W, uint32_t H, const float *u, const float *tex,
               uint32_t tw, uint32_t th, uint32_t grid)
{
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    for (uint32_t py = 0; py < H; ++py)
        for (uint32_t px = 0; px < W; ++px) {
            const size_t o = (size_t)py * W + px;
            const GPixel g = gb_pixel(&F, vis[o], (int32_t)px, (int32_t)py);
            if (depth) depth[o] = g.depth;
            if (position) memcpy(position + 3 * o, g.pos, sizeof g.pos);
            if (normal) memcpy(normal + 3 * o, g.nrm, sizeof g.nrm);
        }
    frame_free(&F);
    return 0;
}

/* n pixels (x, y) -> n x 8 words {depth, x, y, z, nx, ny, nz, id}; -1 and nothing written if a pixel lies outside the frame */
int gbm_pick(uint32_t *out8, const int32_t *pixels_xy, uint32_t n, const uint32_t *vis, uint32_t W, uint32_t H, const float *u,
             const float *tex, uint32_t tw, uint32_t th, uint32_t grid)
{
    for (uint32_t k = 0; k < n; ++k)
        if (pixels_xy[2 * k] < 0 || pixels_xy[2 * k] >= (int32_t)W || pixels_xy[2 * k + 1] < 0 || pixels_xy[2 * k + 1] >= (int32_t)H) return -1;
    Frame F;
    if (frame_init(&F, W, H, u, tex, tw, th, grid)) return -1;
    for (uint32_t k = 0; k < n; ++k) {
        const int32_t px = pixels_xy[2 * k], py = pixels_xy[2 * k + 1];
        const GPixel g = gb_pixel(&F, vis[(size_t)py * W + (size_t)px], px, py);
        memcpy(out8 + 8 * (size_t)k, &g, 32);
    }
    frame_free(&F);
    return 0;
}

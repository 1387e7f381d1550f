/* contour_model.c -- CPU model of contour extraction, the contract the gfx950 kernels of
 * vulkan_forge_amd/csrc/vf_contour.h (k_ct_count, k_ct_scan, k_ct_emit, k_ct_bounds) are held to bit for bit.  Written from the
 * contract: every triangle of the renderer's grid is tested against every level with the "above iff h >= L" rule, one at a time, in
 * the record order of rule 4; nothing of the kernels' block skipping or index-range search is restated here.  Vertex heights are the
 * overlay model's ovm_vertex_height (included below), so the records append to that model's layers and its composite draws them.
 *
 *   gcc -std=c11 -O2 -ffp-contract=off -shared -fPIC contour_model.c -o libctmodel.so -lm     (contour_model.py does this)
 */
#include "../overlay_model/overlay_model.c"

/* h[j * n + i] = displaced height of vertex (i, j) */
void ctm_heights(const float *tex, uint32_t tw, uint32_t th, uint32_t grid, float *h)
{
    const uint32_t n = grid < 2 ? 2 : grid;
    for (uint32_t j = 0; j < n; ++j)
        for (uint32_t i = 0; i < n; ++i) h[(size_t)j * n + i] = ovm_vertex_height(tex, tw, th, grid, i, j);
}

typedef struct { float x, z, h; } CtVert;

/* rule 3: the crossing of L with an edge, from its below vertex P to its above vertex Q */
static void ct_cross(float L, const CtVert *P, const CtVert *Q, float *x, float *z)
{
    const float t = (L - P->h) / (Q->h - P->h);
    *x = fmaf(t, Q->x - P->x, P->x);
    *z = fmaf(t, Q->z - P->z, P->z);
}

/* rules 1 and 2: 1 and the segment p0 -> p1 when L crosses triangle v[0..2], else 0 */
static int ct_segment(float L, const CtVert v[3], float p0[2], float p1[2])
{
    int above[3], na = 0;
    for (int k = 0; k < 3; ++k) {
        if (!isfinite(v[k].h)) return 0;
        above[k] = v[k].h >= L;
        na += above[k];
    }
    if (na == 0 || na == 3) return 0;
    int s = 0;
    for (int k = 0; k < 3; ++k)
        if (above[k] == (na == 1)) s = k;                               /* the vertex alone on its side */
    const CtVert *S = &v[s], *N = &v[(s + 1) % 3], *R = &v[(s + 2) % 3];
    if (above[s]) {
        ct_cross(L, N, S, &p0[0], &p0[1]);
        ct_cross(L, R, S, &p1[0], &p1[1]);
    } else {
        ct_cross(L, S, R, &p0[0], &p0[1]);
        ct_cross(L, S, N, &p1[0], &p1[1]);
    }
    return 1;
}

/* first index k with levels[k] > v */
static uint32_t ct_upper(const float *levels, uint32_t nlevels, float v)
{
    uint32_t lo = 0, hi = nlevels;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (levels[mid] <= v) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

/* The layer's records -> out (when not NULL; room for `cap` records), in the order of rule 4.  Returns the number of segments
 * (also when out is NULL or too small: nothing is written beyond cap).  flags: DRAPE [| 32 occlude]; round: a disc at every p0.
 * bracket == 0: every level is tested against every triangle (the contract as stated).  bracket != 0: the levels at or below a
 * triangle's lowest and above its highest vertex are skipped by binary search -- the same records (tests/test_contour_model.py), in a
 * time that lets tools/exp_contours.py use this as the host route on large grids. */
uint64_t ctm_extract(const float *h, uint32_t n, float spacing, const float *levels, uint32_t nlevels, float hw, uint32_t rgba,
                     uint32_t flags, uint32_t feature, uint32_t pad0, float lift, int round, int bracket, OvIn *out, uint64_t cap)
{
    const uint32_t nm1 = n - 1, nb = (nm1 + 7u) / 8u;
    const float step = (2.0f * 1.5f) / ((float)n - 1.0f);
    uint64_t nseg = 0, w = 0;
    for (uint32_t b = 0; b < nb * nb; ++b)
        for (uint32_t cell = 0; cell < 64u; ++cell) {
            const uint32_t i = (b % nb) * 8u + cell % 8u, j = (b / nb) * 8u + cell / 8u;
            if (i >= nm1 || j >= nm1) continue;
            const float x0 = (-1.5f + (float)i * step) * spacing, x1 = (-1.5f + (float)(i + 1u) * step) * spacing;
            const float z0 = (-1.5f + (float)j * step) * spacing, z1 = (-1.5f + (float)(j + 1u) * step) * spacing;
            const CtVert A = { x0, z0, h[(size_t)j * n + i] }, B = { x1, z0, h[(size_t)j * n + i + 1u] };
            const CtVert Cv = { x0, z1, h[(size_t)(j + 1u) * n + i] }, D = { x1, z1, h[(size_t)(j + 1u) * n + i + 1u] };
            const CtVert tri[2][3] = { { A, Cv, B }, { B, Cv, D } };
            for (int t = 0; t < 2; ++t) {
                uint32_t k = 0, k1 = nlevels;
                if (bracket) {
                    const CtVert *v = tri[t];
                    if (!(isfinite(v[0].h) && isfinite(v[1].h) && isfinite(v[2].h))) continue;
                    k = ct_upper(levels, nlevels, fminf(v[0].h, fminf(v[1].h, v[2].h)));
                    k1 = ct_upper(levels, nlevels, fmaxf(v[0].h, fmaxf(v[1].h, v[2].h)));
                }
                for (; k < k1; ++k) {
                    float p0[2], p1[2];
                    if (!ct_segment(levels[k], tri[t], p0, p1)) continue;
                    nseg++;
                    for (int rec = 0; rec < (round ? 2 : 1); ++rec, ++w) {
                        if (!out || w >= cap) continue;
                        OvIn q;
                        memset(&q, 0, sizeof q);
                        q.p0[0] = p0[0]; q.p0[1] = lift; q.p0[2] = p0[1];
                        q.p1[0] = rec ? p0[0] : p1[0]; q.p1[1] = lift; q.p1[2] = rec ? p0[1] : p1[1];
                        q.size = hw; q.flags = (rec ? CIRCLE : SEGMENT) | flags; q.rgba = rgba; q.feature = feature; q.pad[0] = pad0;
                        out[w] = q;
                    }
                }
            }
        }
    return nseg;
}

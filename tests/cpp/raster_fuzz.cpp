// raster_fuzz.cpp -- host check of vulkan_forge_amd/csrc/vf_raster.h (the span solver of the tile kernel's fast raster path)
// against a brute-force int64 evaluation of the coverage rule of DESIGN.md section 4 (pixel centres, top-left rule on
// inside-positive edge functions).  Built and run by tests/test_raster_spans.py:
//     g++ -O2 -ffp-contract=off [-DVF_RASTER_RCP_ULPS=-1|0|1] tests/cpp/raster_fuzz.cpp -o raster_fuzz && ./raster_fuzz <cases> <seed> [target extent]
// For every random triangle x tile window x line it requires
//   - stage 1 (span_line) to contain the true span,
//   - stage 2 (span_confirm), when it accepts, to make the stage-1 span equal to the true span,
//   - span_exact to equal the true span always,
//   - the group bound (span_group) of every run of up to four adjacent lines to contain the stage-1 span of each of its lines.
// It also reports how often stage 2 falls back (the FP32 path must decide nearly every line by itself).
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include "raster_cases.h"           // the triangle / window stream and the brute-force covered(): shared with tests/hip/raster_device_fuzz.hip
#include "../../vulkan_forge_amd/csrc/vf_raster.h"

using namespace vf;
using raster_cases::covered;

int main(int argc, char **argv)
{
    const long cases = argc > 1 ? atol(argv[1]) : 200000;
    raster_cases::Stream stream(argc > 2 ? (uint64_t)atoll(argv[2]) : 1, argc > 3 ? atol(argv[3]) : 4096);
    long lines = 0, nonempty = 0, fallback = 0, irregular_tris = 0, tris = 0, bad = 0;
    long k_tris[10] = {0}, k_irr[10] = {0}, k_lines[10] = {0}, k_fb[10] = {0};
    long group_lines = 0, group_slack = 0;
    for (long c = 0; c < cases && bad < 10; ++c) {
        raster_cases::Case rc;
        if (!stream.draw(rc)) continue;
        ++tris;
        const raster_cases::SolverArgs sa = raster_cases::solver_args(rc);
        const int kind = rc.kind;
        const int32_t *X = rc.X, *Y = rc.Y, *U = sa.U, *V = sa.V;
        const int32_t px0 = rc.px0, py0 = rc.py0, n_outer = sa.n_outer, n_inner = sa.n_inner, u0c = sa.u0c, v0c = sa.v0c;
        const bool cols = sa.cols;
        SpanSetup S;
        span_setup(U, V, !cols, u0c, v0c, n_outer, S);
        irregular_tris += S.regular ? 0 : 1;
        k_tris[kind]++; k_irr[kind] += S.regular ? 0 : 1;
        if (S.regular)                                     // stage 0: the bound of lines oa .. oa + 3 holds every one of their stage-1 spans
            for (int32_t oa = 0; oa <= n_outer && bad < 10; oa += 4) {
                const int32_t ob = std::min(oa + 3, n_outer);
                int32_t glo, ghi;
                span_group(S, oa, ob, n_inner, glo, ghi);
                for (int32_t o = oa; o <= ob; ++o) {
                    int32_t F[3], lo, hi;
                    span_line(S, o, n_inner, F, lo, hi);
                    ++group_lines;
                    if (lo <= hi && (glo > lo || ghi < hi)) { printf("group bound cuts a line: case %ld lines %d..%d line %d: [%d,%d] vs group [%d,%d]\n", c, oa, ob, o, lo, hi, glo, ghi); ++bad; break; }
                    group_slack += (lo <= hi) ? (lo - glo) + (ghi - hi) : 0;
                }
            }
        for (int32_t o = 0; o <= n_outer; ++o) {
            ++lines; k_lines[kind]++;
            int32_t tlo = n_inner + 1, thi = -1;           // brute force: first / last covered offset (coverage along a line is an interval)
            int ncov = 0;
            for (int32_t r = 0; r <= n_inner; ++r) {
                const int32_t px = cols ? px0 + o : px0 + r, py = cols ? py0 + r : py0 + o;
                if (covered(X, Y, px, py)) { tlo = std::min(tlo, r); thi = std::max(thi, r); ++ncov; }
            }
            if (ncov && ncov != thi - tlo + 1) { printf("NOT AN INTERVAL?! case %ld\n", c); ++bad; break; }
            nonempty += ncov ? 1 : 0;
            int32_t F[3], lo, hi;
            span_line(S, o, n_inner, F, lo, hi);
            bool use_exact = !S.regular;
            if (S.regular) {
                if (ncov && (lo > tlo || hi < thi || lo > hi)) { printf("stage 1 cuts the span: case %ld line %d: [%d,%d] vs true [%d,%d]\n", c, o, lo, hi, tlo, thi); ++bad; break; }
                if (lo <= hi) {
                    if (span_confirm(S, o, n_inner, F)) {
                        const bool same = ncov ? (lo == tlo && hi == thi) : false;
                        if (!same) { printf("stage 2 accepts a wrong span: case %ld line %d: [%d,%d] vs true [%d,%d] (ncov %d)\n", c, o, lo, hi, tlo, thi, ncov); ++bad; break; }
                    } else { use_exact = true; ++fallback; k_fb[kind]++; }
                }
            }
            int32_t elo, ehi;
            span_exact(U, V, !cols, u0c, v0c, o, n_inner, elo, ehi);
            elo = std::max(elo, 0); ehi = std::min(ehi, n_inner);
            const bool eok = ncov ? (elo == tlo && ehi == thi) : (elo > ehi);
            if (!eok) { printf("span_exact wrong: case %ld line %d: [%d,%d] vs true [%d,%d] (ncov %d)\n", c, o, elo, ehi, tlo, thi, ncov); ++bad; break; }
            (void)use_exact;
        }
    }
    printf("triangles %ld (irregular %ld = %.3f %%)  lines %ld  non-empty %ld  stage-2 fallbacks %ld (%.4f %% of lines)  failures %ld\n",
           tris, irregular_tris, 100.0 * irregular_tris / (tris ? tris : 1), lines, nonempty, fallback, 100.0 * fallback / (lines ? lines : 1), bad);
    printf("group bounds: %ld lines checked, mean slack %.2f pixels per non-empty line\n", group_lines, (double)group_slack / (group_lines ? group_lines : 1));
    for (int k = 0; k < 10; ++k) printf("  kind %d: triangles %ld irregular %.3f %%  lines %ld fallback %.4f %%\n", k, k_tris[k], 100.0 * k_irr[k] / (k_tris[k] ? k_tris[k] : 1), k_lines[k], 100.0 * k_fb[k] / (k_lines[k] ? k_lines[k] : 1));
    return bad ? 1 : 0;
}

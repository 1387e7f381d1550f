// AddressSanitizer + UBSan run of the line-loop chooser's decision (vulkan_forge_amd/csrc/vf_line_loop.h; tests/test_sanitizers.py).
// The expectations restate the schedule in words, not through the header's constants: settle 4 frames on the default variant, probe 16
// frames ABBA, then the default unless the other variant's mean is below 0.97 of its own, and a look at both (B A A B, probed) in the
// last four frames of every 128.
#include "../../vulkan_forge_amd/csrc/vf_line_loop.h"
#include <cstdio>
#include <initializer_list>

static int failures = 0;
static void expect(bool ok, const char *what, int guess, unsigned e)
{
    if (!ok) { std::printf("FAILED: %s (guess %d, epoch frame %u)\n", what, guess, e); ++failures; }
}

int main()
{
    using vf::LoopPick;
    using vf::line_loop_pick;
    const uint32_t none[2] = { 0u, 0u }, both[2] = { 8u, 8u };
    const float zero[2] = { 0.0f, 0.0f };
    for (int guess = 0; guess <= 1; ++guess) {
        const int other = guess ^ 1;
        // frames 0-3: the default variant, not probed -- whatever has been measured
        for (unsigned e = 0; e < 4; ++e) {
            const LoopPick p = line_loop_pick(-1, e, guess, zero, none, true);
            expect(p.variant == guess && !p.probe, "settle frames draw the default, unprobed", guess, e);
        }
        // frames 4-19: A B B A repeating from the default, all probed -- with or without samples
        const int abba[4] = { 0, 1, 1, 0 };
        for (unsigned e = 4; e < 20; ++e)
            for (const uint32_t *n : { none, both }) {
                const LoopPick p = line_loop_pick(-1, e, guess, zero, n, true);
                expect(p.variant == (guess ^ abba[(e - 4) % 4]) && p.probe, "the probe window alternates ABBA, probed", guess, e);
            }
        // from frame 20: means on both sides of the 3 % rule, and samples for no, one and both variants
        float clearly[2], barely[2], slower[2];
        clearly[guess] = 1.0f; clearly[other] = 0.9699f;       // the other one is clearly faster
        barely[guess] = 1.0f; barely[other] = 0.9701f;         // faster, not by 3 %
        slower[guess] = 1.0f; slower[other] = 1.2f;
        uint32_t only_default[2] = { 0u, 0u }, only_other[2] = { 0u, 0u };
        only_default[guess] = 5u; only_other[other] = 5u;
        for (unsigned e = 20; e < 3u * 128u + 40u; ++e) {
            const bool look = e % 128u >= 124u;
            const unsigned k = e % 128u - 124u;                // (meaningful when look)
            const int baab[4] = { 1, 0, 0, 1 };                // B A A B seen from the variant in use
            struct { const float *ms; int in_use; } cases[3] = { { clearly, other }, { barely, guess }, { slower, guess } };
            for (const auto &c : cases) {
                const LoopPick p = line_loop_pick(-1, e, guess, c.ms, both, true);
                expect(p.variant == (look ? c.in_use ^ baab[k] : c.in_use), "the choice after the window (3 % rule, B A A B looks)", guess, e);
                expect(p.probe == look, "only the look frames are probed after the window", guess, e);
            }
            for (const uint32_t *n : { none, (const uint32_t *)only_default, (const uint32_t *)only_other }) {
                const LoopPick p = line_loop_pick(-1, e, guess, clearly, n, true);
                expect(p.variant == guess, "fewer than two variants sampled: the default, also in a look", guess, e);
                expect(p.probe == look, "look frames are probed without samples too", guess, e);
            }
        }
        // a shard without tiles is never probed (the variant is chosen as usual); a forced mode always wins and never probes
        for (unsigned e = 0; e < 300; ++e) {
            const LoopPick q = line_loop_pick(-1, e, guess, clearly, both, false), with = line_loop_pick(-1, e, guess, clearly, both, true);
            expect(!q.probe && q.variant == with.variant, "no tiles: never probed", guess, e);
            for (int forced = 0; forced <= 1; ++forced)
                for (int tiles = 0; tiles <= 1; ++tiles) {
                    const LoopPick p = line_loop_pick(forced, e, guess, clearly, both, tiles != 0);
                    expect(p.variant == forced && !p.probe, "a forced mode picks its variant, unprobed", guess, e);
                }
        }
    }
    if (failures) return 1;
    std::printf("line-loop chooser under ASan + UBSan: ok\n");
    return 0;
}

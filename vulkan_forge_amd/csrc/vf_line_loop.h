// vf_line_loop.h -- which line loop of the raster draws a frame: the decision, without a HIP call (the handle's LineLoop in vf_hip.hip
// takes the samples and arms the probes; tests/cpp/line_loop_main.cpp pins this schedule).  Host code only.
#pragma once
#include <cstdint>

namespace vf {

// The schedule of an epoch (frames counted from a shard change, a height upload, a camera that starts to move): the plan settles for
// four frames on the default variant; then sixteen frames ABBA ABBA ABBA ABBA, each one probed (both variants see the same mean
// position in the window: a drift of the frame cost -- the plan still settling, a camera under way -- cancels); then the faster one,
// looked at again in the last four frames of every 128 (B A A B seen from the variant in use: two probed frames of each).
constexpr uint32_t kLoopSettle = 4, kLoopProbe = 16, kLoopAgain = 128, kLoopLook = 4;
// (round 6: the default variant stays unless the other one measured CLEARLY faster, 3 %.  Where the choice matters the two are
//  5-17 % apart -- profiles/r06_line_loops.log -- but a probed frame carries two event records and reads 10 % high, and two
//  noisy means 0.01 % apart once made a C4 handle draw with the strip variant: 0.787 ms instead of 0.723)
constexpr float kLoopClearlyFaster = 0.97f;

struct LoopPick {
    int variant;                         // 1: line groups in the raster's line loop, 0: the plain loop
    bool probe;                          // the frame is timed: a sample for `variant`
};

inline int loop_abba(uint32_t k) { return (k & 3u) == 1u || (k & 3u) == 2u ? 1 : 0; }

// forced: 0 / 1 a fixed variant (never probed), -1 measure and choose; e: the frame's number in its epoch; guess: the default variant;
// ms / n: mean and count of the samples of each variant in this epoch; has_tiles: the shard draws something (an empty one has nothing to time).
inline LoopPick line_loop_pick(int forced, uint32_t e, int guess, const float ms[2], const uint32_t n[2], bool has_tiles)
{
    if (forced >= 0) return { forced != 0 ? 1 : 0, false };
    const bool window = e >= kLoopSettle && e < kLoopSettle + kLoopProbe;
    const bool look = e >= kLoopSettle + kLoopProbe && e % kLoopAgain >= kLoopAgain - kLoopLook;
    int variant = guess;
    if (window) variant = guess ^ loop_abba(e - kLoopSettle);
    else if (e >= kLoopSettle + kLoopProbe && n[0] && n[1]) {
        variant = ms[guess ^ 1] < kLoopClearlyFaster * ms[guess] ? (guess ^ 1) : guess;
        if (look) variant ^= loop_abba(e % kLoopAgain - (kLoopAgain - kLoopLook)) ^ 1;
    }
    // (no samples yet -- a host that queues frames faster than the GPU draws them is past the window before its first probe
    //  completes: the default stays until they arrive; they are taken whenever they complete)
    return { variant, has_tiles && (window || look) };
}

} // namespace vf

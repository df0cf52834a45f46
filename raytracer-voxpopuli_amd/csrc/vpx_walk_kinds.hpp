// The walkers' policies per walk kind (walk_wave<KIND>, vpx_trace.hpp): types with constant
// members, a derived kind stating only what differs from its base.  Every combination is exact
// (each lane runs skip::walk_skip's sequence); a field only decides what the wave pays for.
// Each field names the measurement that decided it (ms per step on one MI355X, interleaved
// runs); DESIGN.md section 4, "Walk kinds", has the histories and the rejected values.
// An A/B build copies this file, edits a field by name and is built with
// -DVPX_WALK_KINDS='"<the copy>"' (tools/build_var.sh).
#pragma once

#include <stdint.h>

namespace vpx {

// FindNearest outside k_frame0 (k_primary, the instance pass, the ray and hit-cell queries).
struct NearestWalk {
    // Keep stepping while steppers x skipw >= waiting skippers.  C1 0.666 vs 0.671 with 2 (with
    // the two-compare step; round 2).
    static constexpr uint32_t skipw = 1;
    // Smallest distance-field cube (bricks) worth a skip.  C1's FindNearest stage 0.430 with 2 /
    // 0.435 with 1 (rounds 1-2).
    static constexpr uint32_t minc = 2;
    // Brick runs: up to `run` cells on the register copy of a brick's word, `passes` brick loads
    // per step-phase iteration.  C1 0.5419-0.5446 with 3 x 3 vs 0.5491-0.5496 with 3 x 2 (round
    // 5); runs above 4 spill.
    static constexpr uint32_t run = 3, passes = 3;
    // An empty brick below minc still skips when its axis box is this many bricks long.  C1
    // 0.4664-0.4707 with 2 / 0.4703-0.4706 with 3 (round 7).
    static constexpr uint32_t minlen = 2;
    // The skip takes the plain-step prefix (skip::skip_box_lean's PRE).  C2 2.164-2.180 with it
    // against 2.127-2.168 (round 12).
    static constexpr bool pre = false;
    // The skip's second closed-form segment only when a lane of the wave needs it.  C1 0.713 ->
    // 0.693, C3 5.57 -> 5.34 (round 2).
    static constexpr bool seg2 = true;
    // skip::step1's two-compare axis choice.  C1 0.678 vs 0.687 with three compares (round 2).
    static constexpr bool min2 = true;
    // The skip phase works its axes out behind a barrier, so the compares' results are not kept
    // in scratch all walk long.  Without it anywhere C1 gained 3.3 % from round 8 instead of 5.9 %.
    static constexpr bool local = true;
    // The instruction forms of round 16: the boxes' byte selectors packed once per walk (skip::box_sel,
    // read back by skip::df_box_sel) instead of dom_axis / sec_axis and the select chains in every
    // skip phase; the class outcomes from a table; the cell's bit and the moved test in one-instruction
    // asm forms (skip::cell_bit, skip::xor_add).  The word is live through the walk loops and an asm
    // statement kept the pool kernels' run loop from unrolling, so only k_frame0's kinds take them:
    // C1 0.3790-0.3834 against the parent's 0.3867-0.3922 (eight interleaved runs); the selectors
    // alone 0.3836-0.3887 against 0.3876-0.3930, not enough by themselves.
    static constexpr bool packed = false;
    // The maturity gate (skip::gate_open): a class-2 lane whose skip would be clipped at an
    // immature axis's next event (exponent of tmax below exponent of tdelta + gate_g, that event
    // within gate_n events of the dominant axis) steps instead.  For the shadow walks of the
    // tiles only (round 10); gate_g 2 or gate_n 8 measured the same on C1.
    static constexpr bool gate = false;
    static constexpr uint32_t gate_g = 1, gate_n = 4;
    // First word of the kind's walk-phase profile (-DVPX_PHASE_PROF, g_phase).
    static constexpr int phase_slot = 0;
};
// k_frame0's FindNearest (7 waves/SIMD).  Four passes: C1 0.5433-0.5444 vs 0.5456-0.5482 in three
// (round 5).  The prefix: C1 0.4458-0.4524 in thirteen runs vs 0.4524-0.4593 in eight (round 12).
struct FrameNearestWalk : NearestWalk {
    static constexpr uint32_t passes = 4;
    static constexpr bool pre = true;
    static constexpr bool packed = true;
};
// The bounce walks (k_tail, k_nearest_tile, k_nearest_pool): rays leaving surfaces.
struct BounceWalk : NearestWalk {
    // 2 on C2 (round 1); 1 / 4 in the pool C2 2.60-2.64 / 2.66-2.75 vs 2.59-2.65.
    static constexpr uint32_t skipw = 2;
    // C2's bounce stage 0.654 -> 0.569 with runs of 4 in one pass (round 2); 3 x 2 in the pool C2
    // 2.65-2.71 vs 2.59-2.65.
    static constexpr uint32_t run = 4, passes = 1;
    // Z1 1.560-1.572 vs 1.604-1.612, C2 and C4 unchanged (round 12).
    static constexpr bool pre = true;
    // Their boxes cross binades in most waves: C2 4.27 -> 4.34 with it (round 2).
    static constexpr bool seg2 = false;
    // They have the registers to keep the axes: with the barrier Z1 1.5191-1.5578 vs the parent's
    // 1.4628-1.5018 (round 8).
    static constexpr bool local = false;
};
// IsOccluded in the tile, list, finish and volume-loop shadow walkers (72 VGPRs, 7 waves/SIMD).
struct ShadowWalk : NearestWalk {
    // 4 on C3 (round 1).
    static constexpr uint32_t skipw = 4;
    // C1's IsOccluded stage 0.354 with 1 / 0.383 with 2 (rounds 1-2); 2 the same as 1 with the gate
    // (round 10).
    static constexpr uint32_t minc = 1;
    // C3 4.01 -> 3.82 with 3 x 1 (round 2); two passes C2 2.466-2.480 vs 2.427-2.452 (round 5).
    static constexpr uint32_t passes = 1;
    // Spilled two more VGPRs with the two-compare step: C3 5.26 -> 5.53 (round 2).
    static constexpr bool min2 = false;
    // Shadow rays start at t = 0 with every axis immature, a compacted wave's lanes all at
    // once: C4 24.90-25.42 -> 24.38-24.87 (round 10).
    static constexpr bool gate = true;
    static constexpr int phase_slot = 16;
};
// k_frame0's shadow walks.  The two-compare step at 7 waves/SIMD: C1 0.5418-0.5489 vs
// 0.5456-0.5539 (seven runs, round 5).  Three passes with the gate: C1 0.4514-0.4522 vs
// 0.4560-0.4626 in two (round 10).  The prefix on top: C1 0.4526-0.4622 vs 0.4524-0.4593, off
// (rounds 12 and 13).
struct FrameShadowWalk : ShadowWalk {
    static constexpr uint32_t passes = 3;
    static constexpr bool min2 = true;
    static constexpr bool packed = true;
};
// k_shadow_pool (96 VGPRs, 5 waves/SIMD).  It takes the two-compare step without spilling: C3
// 3.684-3.719 vs 3.724-3.756 (round 3).  Its lanes start at different times, so a gated lane
// holds its wave in the step phase: C3 3.307-3.351 -> 3.355-3.389 with the gate (round 10).
struct ShadowPoolWalk : ShadowWalk {
    static constexpr bool min2 = true;
    static constexpr bool gate = false;
};
// The instance grids' shadow walks: cubes of one brick are stepped through.  C4 42.43-42.51
// with 2 vs 42.71-42.96 with 1 (five runs; 3: 42.82-42.90).
struct InstShadowWalk : ShadowWalk {
    static constexpr uint32_t minc = 2;
};

}  // namespace vpx

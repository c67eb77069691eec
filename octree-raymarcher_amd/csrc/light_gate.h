// light_gate.h — which of the three shadow-ray shortcuts a stack-kernel launch may use: the state of a world's light
// clearance and the one decision that turns it, the launch and svo_trace_params.shadow's switches into TraceArgs::light_clear.
// Plain C++: no HIP and no svo_world, so that host/light_gate_check.cpp prints the whole table (tests/test_light_gate_cpu.py).
#pragma once
#include <stdint.h>

#include "../../include/svo.h"
#include "svo_format.h"

namespace svo {

// What svo_world_prepare_light has left on a world (hip_own.h LightClearance::state).
//     FRESH    unchanged since its upload, never prepared: the one state in which a launch prepares the world on its own
//     DROPPED  the pools changed after the upload (or a pass failed half issued): only svo_world_prepare_light brings the bits back
//     UNUSED   prepared for `sdir`, but the direction or the world fails the rule's premises: nothing was decided, nothing is used
//     NODES    WIDE_CLEAR_BIT of the wide pool's EMPTY entries holds for `sdir`; the world fails the premises of the brick flags
//     BRICKS   the bits and the per-brick flags (BMAT_CLEAR_BIT) hold for `sdir`
// Transitions:
//     upload (and generation on the device)   -> FRESH: Hbm is made anew; the upload's own wide build drops nothing (drop_wide
//                                                drops only what was prepared)
//     a change to the pools (install_chunk,   -> DROPPED from every state, the pass's scratch freed; drop_wide: from UNUSED, NODES
//       drop_wide)                               and BRICKS only
//     a re-pack inside an edit                -> DROPPED (it is an upload that is no fresh world)
//     prepare_light  no wide pool, or         -> NODES and BRICKS fall to UNUSED (the old bits are used no more), the others stay
//                      hipSetDevice fails
//                    premises fail            -> UNUSED, `sdir` the new direction
//                    a failure once the pass  -> DROPPED
//                      is being issued
//                    issued                   -> NODES or BRICKS, `sdir` the new direction
enum class ClearState : int { FRESH, DROPPED, UNUSED, NODES, BRICKS };

// What light_gate asks of a launch and its world:
//     eligible       shadow rays, a camera launch of the CPU march, no far ends, no see-through view, no tile costs
//     switches       svo_trace_params.shadow
//     auto_work      wide entries x chunks is within what a launch prepares on its own
//     same_dir       the launch's shadow direction is the prepared one bit for bit
//     eps_pow2       eps is a power of two
//     eps_covers     eps is at least twice the float spacing at the world's largest coordinate
//     dark_premises  dark at birth's own: exact geometry, a finite shadow direction, no world corner with a negative coordinate
// and what it answers: the LIGHT_CLEAR_* bits, and whether to prepare the world for this launch's light first and ask again with the
// state that leaves
struct LightGateIn { bool eligible; int32_t switches; ClearState state; bool auto_work, same_dir, eps_pow2, eps_covers, dark_premises; };
struct LightGateOut { int32_t bits; bool prepare; };

// What each switch takes away.  SVO_SHADOW_NO_BRICK_CLEARANCE means "no shadow ray is settled at its primary hit", so it removes DARK
// with BRICKS: tests/test_brick_clearance.py compares the lane-steps of a default launch with those of a launch under that bit and
// asks for half of what the flags' rays take; with dark at birth on under the bit the difference fell below that (DESIGN.md 6v "Off"
// has the figures).  DARK also asks for eps_covers, which is no premise of its rule (it reads the hit brick's cells only: no prepared
// light, no bit of the pools, any eps), only of its default: tests/test_clearance_positions.py::test_beyond_the_limit_no_lane_retires
// wants a default launch below that eps to take about as many lane-steps as one under SVO_SHADOW_NO_CLEARANCE, and the rule removes
// lane-steps from the default launch alone.
constexpr struct { int32_t bit, removes; } LIGHT_SWITCHES[] = {
    { SVO_SHADOW_NO_CLEARANCE,       LIGHT_CLEAR_NODES | LIGHT_CLEAR_BRICKS | LIGHT_CLEAR_DARK },
    { SVO_SHADOW_NO_BRICK_CLEARANCE, LIGHT_CLEAR_BRICKS | LIGHT_CLEAR_DARK },
    { SVO_SHADOW_NO_DARK_BIRTH,      LIGHT_CLEAR_DARK },
};

constexpr LightGateOut light_gate(const LightGateIn &g)
{
    if (!g.eligible) return { 0, false };
    int32_t allowed = LIGHT_CLEAR_NODES | LIGHT_CLEAR_BRICKS | LIGHT_CLEAR_DARK;
    for (const auto &sw : LIGHT_SWITCHES) if (g.switches & sw.bit) allowed &= ~sw.removes;
    const bool prepared = g.same_dir && g.eps_pow2 && g.eps_covers;     // what was prepared holds for this launch
    int32_t held = 0;
    if (prepared && (g.state == ClearState::NODES || g.state == ClearState::BRICKS)) held |= LIGHT_CLEAR_NODES;
    if (prepared && g.state == ClearState::BRICKS) held |= LIGHT_CLEAR_BRICKS;
    if (g.dark_premises && g.eps_covers) held |= LIGHT_CLEAR_DARK;
    return { allowed & held, (allowed & LIGHT_CLEAR_NODES) != 0 && g.state == ClearState::FRESH && g.auto_work };
}

} // namespace svo

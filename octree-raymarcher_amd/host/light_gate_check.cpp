// light_gate_check.cpp — csrc/light_gate.h's decision for every combination of its inputs, one line each (tests/test_light_gate_cpu.py
// holds them against the rules of include/svo.h, stated on their own in Python).
//   g++ -std=c++17 -I../csrc light_gate_check.cpp -o light_gate_check
// A line: eligible switches state auto_work same_dir eps_pow2 eps_covers dark_premises -> bits prepare; the switches are
// svo_trace_params.shadow's three bits with bit 0 (shadow rays on) set, the states are named.
#include <cstdio>

#include "light_gate.h"

int main()
{
    using namespace svo;
    const struct { ClearState s; const char *name; } states[] = { { ClearState::FRESH, "FRESH" }, { ClearState::DROPPED, "DROPPED" }, { ClearState::UNUSED, "UNUSED" },
                                                                    { ClearState::NODES, "NODES" }, { ClearState::BRICKS, "BRICKS" } };
    int lines = 0;
    for (int eligible = 0; eligible < 2; ++eligible)
        for (int sw = 0; sw < 8; ++sw)
            for (const auto &st : states)
                for (int flags = 0; flags < 32; ++flags) {
                    LightGateIn g = {};
                    g.eligible = eligible != 0;
                    g.switches = 1 | (sw & 1 ? SVO_SHADOW_NO_CLEARANCE : 0) | (sw & 2 ? SVO_SHADOW_NO_BRICK_CLEARANCE : 0) | (sw & 4 ? SVO_SHADOW_NO_DARK_BIRTH : 0);
                    g.state = st.s;
                    g.auto_work = (flags & 1) != 0; g.same_dir = (flags & 2) != 0; g.eps_pow2 = (flags & 4) != 0; g.eps_covers = (flags & 8) != 0; g.dark_premises = (flags & 16) != 0;
                    const LightGateOut o = light_gate(g);
                    std::printf("%d %d %s %d %d %d %d %d -> %d %d\n", eligible, (int)g.switches, st.name, (int)g.auto_work, (int)g.same_dir, (int)g.eps_pow2, (int)g.eps_covers,
                                (int)g.dark_premises, (int)o.bits, (int)o.prepare);
                    ++lines;
                }
    std::fprintf(stderr, "light_gate_check: %d lines\n", lines);
    return 0;
}

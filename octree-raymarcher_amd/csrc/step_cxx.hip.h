// step_cxx.hip.h — the march step of k_trace_stack as C++: the readable statement of the algorithm that step_asm.hip.h runs as one
// hand-scheduled statement, and its A/B partner (-DSVO_CXX_STEP builds the kernel with it).  Same parameters as march_steps_asm
// (the statement's own counters stay untouched), same results; it chases a BRANCH entry inside the step,
// ignores `shadow_lanes` (a shadow ray that marches on past a clear cell ends the same way) and the drain bit of the step count.
// Included by kernel_stack.hip.h behind its helpers (recip_pow2, wide_slot, is_branch, ld_node).
#pragma once

namespace svo {

// entry `e` (64 per wide node, counted from the chunk's top wide node) of a chunk's wide tree
template <bool BIG>
__device__ __forceinline__ uint32_t ld_wide_entry(const uint32_t *wide, WideRef<BIG> wide_b, uint32_t e)
{
    if constexpr (BIG) return *reinterpret_cast<const uint32_t *>((size_t)wide_b + ((size_t)e << 2));
    else return ld_node(wide, wide_b + (e << 2));
}

template <bool BIG, bool GLSL>
__device__ __forceinline__ void march_steps_cxx(
    int &mode, V3 &O, V3 &Blo, float &bsize, float &res, float &t, int &cnt, float &tt_saved, float &t_miss, int &it_saved,
    float &tw, int &cw, int &pux, int &puy, int &puz, int &valid, int &plev, unsigned long long &bmask, int &creepn,
    const V3 beta, const V3 g, const V3 clo, const V3 alpha, const int levels, const int nw, const float res_tree,
    const WideRef<BIG> wide_b, const uint32_t twig_off, const uint32_t lds_lane, const StepUniform U, const int nsteps_sure,
    const unsigned long long, StepStats &)
{
    const float csize = U.csize, eps = U.eps;
    const auto stk = (__attribute__((address_space(3))) uint32_t *)(size_t)lds_lane;      // the lane's descent column: wide level k at stk[64 k]
    // ---- one step of the current level: tree (src/Traverse.cpp:79-111) or brick (:54-70) -----
    //      First decide what the step does (locate the cell, read its node / mask bit), then apply exactly one of
    //      the outcomes below as a flat sequence of predicated updates of the lane state.
    for (int step = nsteps_sure & 0xFFFF; step > 0; --step) {
        if (mode == M_TREE || mode == M_TWIG) {
            enum : int { S_LEAVE = 0, S_ADVANCE = 1, S_ENTER = 2, S_HIT_LEAF = 3, S_HIT_CELL = 4, S_BAD = 5 };
            const bool twig = mode == M_TWIG;
            const float Bsize = twig ? res * 4.0f : csize, inv_res = recip_pow2(res);
            const int crept = creepn < 0 ? -creepn : creepn;
            creepn = -crept;                                        // disarmed unless this step advances (see the creep block)
            bool leave = cnt <= 0;                                  // the level's step cap (src/Traverse.cpp:54,79)
            cnt -= 1;                                               // (a lane that leaves restores or resets cnt below)
            const V3 p = O + beta * t;
            leave |= !inside(p, Blo, Blo + Bsize);
            // lattice coordinates of p inside the box.  Brick: truncation, as the reference (:58).  Tree: the number
            // of cell boundaries <= p; truncation gives exactly that unless the quotient is integral (p on a lattice
            // plane, or rounded onto one), which the rare branch below settles with the reference's own comparison.
            const float fx = (p.x - Blo.x) * inv_res, fy = (p.y - Blo.y) * inv_res, fz = (p.z - Blo.z) * inv_res;
            int ux = (int)fx, uy = (int)fy, uz = (int)fz;
            const bool on_lattice = !twig && ((fx == (float)ux) | (fy == (float)uy) | (fz == (float)uz));
            if (SVO_UNLIKELY(on_lattice)) {
                const int nmax = (1 << levels) - 1;
                ux = ux > nmax ? nmax : ux; uy = uy > nmax ? nmax : uy; uz = uz > nmax ? nmax : uz;
                ux -= (Blo.x + (float)ux * res > p.x) ? 1 : 0;
                uy -= (Blo.y + (float)uy * res > p.y) ? 1 : 0;
                uz -= (Blo.z + (float)uz * res > p.z) ? 1 : 0;
            }
            if (twig) leave |= (ux > 3) | (uy > 3) | (uz > 3);      // isInsideCube(off, 0, 3), :59 (off >= 0 always: p >= Blo)

            int what = S_LEAVE;
            int low = 0;                                            // the located cell spans (low+1) lattice steps
            uint32_t payload = 0;                                   // node word (tree) / cell index (brick)
            if (SVO_LIKELY(!leave)) {
                if (!twig) {
                    // descend through the chunk's wide tree (wide_tree.hip.h: two reference levels per node) from the
                    // deepest cached wide level whose node is unchanged: wide level k is selected by the coordinate bits
                    // above 2 (nw - k), so it survives while the highest differing bit lies below that
                    const uint32_t diff = (uint32_t)((ux ^ pux) | (uy ^ puy) | (uz ^ puz));
                    const int hb = 32 - __clz((int)(diff | 1u));    // (diff == 0 reads as "bit 0 differs": keep = nw - 1 >= valid either way)
                    const int keep = nw - ((hb + 1) >> 1);
                    int k;                                          // min(keep, valid), never below the top level (one v_med3_i32)
                    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(k) : "v"(keep), "v"(valid));
                    uint32_t wnode = stk[64 * k];                   // (row 0 holds node 0: no branch for k == 0)
                    int sh = 2 * (nw - 1 - k);                      // the two coordinate bits that select the entry
                    uint32_t word = ld_wide_entry<BIG>(U.wide, wide_b, (wnode << 6) + wide_slot(ux, uy, uz, sh));
                    while (is_branch(word)) {
                        wnode = word & WIDE_PAYLOAD;
                        ++k;
                        stk[64 * k] = wnode;
                        sh -= 2;
                        word = ld_wide_entry<BIG>(U.wide, wide_b, (wnode << 6) + wide_slot(ux, uy, uz, sh));
                    }
                    valid = k; pux = ux; puy = uy; puz = uz;
                    plev = (int)((word >> 25) & 31u);               // the reference node's level: it spans 2^(levels - level) cells
                    low = (1 << (levels - plev)) - 1;
                    const uint32_t type = node_type(word);
                    what = type == EMPTY ? S_ADVANCE : type == LEAF ? S_HIT_LEAF : S_ENTER;
                    payload = word;
                } else {
                    payload = (uint32_t)(uz * 16 + uy * 4 + ux);
                    what = ((bmask >> payload) & 1ull) ? S_HIT_CELL : S_ADVANCE;
                }
            }

            // ---- the one escape evaluation of the step, out of the located cell from p (src/Traverse.cpp:89,104-105,67):
            //      an EMPTY node or an empty brick cell advances by it; a TWIG node about to be entered remembers where the
            //      tree level goes on if the brick march misses - t + (escape(p, node box) + EPS), :104-105, the same
            //      expression with the same operands - so that leaving the brick later costs no evaluation of its own.
            //      A lane that leaves its level evaluates nothing here: out of a brick it resumes the tree level at the
            //      remembered parameter; out of the chunk (:164-168) it only raises the "escape pending" bit of cw, and the
            //      chunk step, for which it has to wait anyway, advances tw from the tree frame's origin, which stays put.
            if (what == S_ADVANCE || what == S_ENTER) {
                const V3 E_lo = mk(Blo.x + (float)(ux & ~low) * res, Blo.y + (float)(uy & ~low) * res, Blo.z + (float)(uz & ~low) * res);
                const float E_size = res * (float)(low + 1);
                const float e = (GLSL ? guarded(escape(p, g, E_lo, E_lo + E_size), eps) : escape(p, g, E_lo, E_lo + E_size)) + eps;
                if (what == S_ADVANCE) {
                    t += e;
                    creepn = e < U.eps2 ? crept + 1 : 0;            // pinned on a lattice plane: see the creep block
                } else {                                            // twigmarch(p, b, node box, ...): a = p, t = 0 (:99,53)
                    bmask = U.mask[twig_off + (payload & WIDE_PAYLOAD)];
                    tt_saved = t; t_miss = t + e; it_saved = cnt;
                    O = p; t = 0.0f; cnt = U.cap_twig;
                    Blo = E_lo;
                    bsize = E_size;
                    res = E_size * 0.25f;                           // leafsize = node size / 4, exact
                    mode = M_TWIG;
                }
            }
            if (leave) {
                if (twig) {                                         // back to the tree level that entered the brick
                    t = t_miss;
                    cnt = it_saved;
                    O = alpha + beta * tw;                          // the chunk march's p (src/Traverse.cpp:144,158)
                    Blo = clo;
                    bsize = csize;
                    res = res_tree;                                 // csize / 2^levels
                    mode = M_TREE;
                } else {                                            // out of the chunk
                    cw |= CW_ESCAPE_PENDING;
                    mode = M_WORLD;
                }
            }
            if (what == S_HIT_LEAF) {
                tw = tw + (GLSL ? t : t - eps);                     // src/Traverse.cpp:93,160 (t - EPS); shaders/Chunkmarch.glsl:266 (t)
                cnt = (int)SVO_CELL_NONE;
                mode = M_HIT;
            }
            if (what == S_HIT_CELL) {
                float sdist = t;                                    // src/Traverse.cpp:63
                sdist += tt_saved;                                  // :101
                tw = tw + sdist;                                    // :160
                cnt = (int)payload;
                mode = M_HIT;
            }
        }
    }
}

} // namespace svo

// chunk_step_cxx.hip.h — the chunk step of k_trace_stack (src/Traverse.cpp:142-168) as C++: the readable statement of what
// chunk_step_asm.hip.h does in one hand-scheduled statement, and its A/B partner (-DSVO_CXX_STEP builds the kernel with it).
// Same parameters as ChunkStepAsm<...>::run, same results: the chunk's lane registers, bsize / res_tree / nw included, are written
// here and nowhere else, and the lanes whose ray ends come back as a mask (their mode is still M_WORLD).
// Included by kernel_stack.hip.h behind its helpers (ChunkGrid, chunk_cell_pow2, chunk_index_u24, vote).
#pragma once

namespace svo {

template <bool BIG, bool GLSL, bool SEG>
struct ChunkStepCxx {
template <int TAB>
static __device__ __forceinline__ unsigned long long run(
    int &mode, float &tw, int &cw, int &ci, int &valid, int &pux, int &puy, int &puz, V3 &clo, WideRef<BIG> &wide_b,
    uint32_t &twig_off, int &levels, V3 &O, float &t, int &cnt, V3 &Blo, float &res, float &bsize, float &res_tree, int &nw,
    const V3 alpha, const V3 beta, const V3 g, [[maybe_unused]] const float far,
    const float Ginv, const int Goff0, const int Goff1, const int Goff2, const int Gdimw, const int Gdimh, const int Gdimd,
    const uint32_t table_in_lds, const uint32_t lds_tab, const ChunkStepUniform U)
{
    const float csize = U.csize, eps = U.eps;
    const V3 wlo = U.wlo, whi = U.whi;
    bool miss = false;
    if (mode == M_WORLD) {
        if (cw < 0) {                               // left its chunk in the step: t += escape(chunk box) + EPS, src/Traverse.cpp:164-168
            cw &= ~CW_ESCAPE_PENDING;
            if constexpr (GLSL) tw += guarded(escape(O, g, clo, clo + csize), eps) + eps;       // (the guard's threshold IS the march's EPS, Chunkmarch.glsl:113)
            else tw += escape(O, g, clo, clo + csize) + eps;
        }
        miss = cw >= U.cap_chunk;
        if constexpr (SEG) miss |= (GLSL ? tw : tw - eps) >= far;          // every later hit lies at tw + s, s >= -leaf_back: the ray has passed its far end
        if (!miss) {
            cw++;
            const V3 p = alpha + beta * tw;
            miss = !inside(p, wlo, whi);
            if (!miss) {
                ChunkGrid G;
                G.inv = Ginv; G.off[0] = Goff0; G.off[1] = Goff1; G.off[2] = Goff2; G.dimw = Gdimw; G.dimh = Gdimh; G.dimd = Gdimd;
                int mx, my, mz;
                chunk_cell_pow2(G, p, mx, my, mz);
                const int ci_new = chunk_index_u24(G, mx, my, mz);
                // The descent cache (stk column, pux/puy/puz, valid) is keyed by chunk and cell, not by ray: a ray that
                // enters the chunk this lane marched last - a shadow ray leaving its primary hit, the next pixel of the
                // tile, a ray pinned on a chunk face - restarts below the deepest common level instead of at the root.
                // Another chunk: nothing of the cache holds.  The cached cell goes too: chunks may differ in depth
                // (src/Octree.h:56-76: an Ocroot carries its own), and a cell of a deeper chunk would make the next
                // descent compute a common prefix above this chunk's top level (keep < 0).
                if (ci_new != ci) { valid = 0; pux = 0; puy = 0; puz = 0; }
                ci = ci_new;
                uint32_t ch_levels, ch_wide, ch_twig;
                if (table_in_lds) {                 // (wave-uniform) the chunk table of k_trace_stack, TAB entries per row
                    const auto tab = (const __attribute__((address_space(3))) uint32_t *)(size_t)lds_tab;
                    clo = mk(__uint_as_float(tab[ci]), __uint_as_float(tab[TAB + ci]), __uint_as_float(tab[2 * TAB + ci]));
                    ch_levels = tab[3 * TAB + ci]; ch_wide = tab[4 * TAB + ci]; ch_twig = tab[5 * TAB + ci];
                } else {                            // TraceArgs::wchunks, read from the launch arguments where it is needed
                    const DevWide *wchunks = *(const DevWide *const __attribute__((address_space(4))) *)((const char __attribute__((address_space(4))) *)U.kernarg + __builtin_offsetof(TraceArgs, wchunks));
                    const DevWide ch = wchunks[ci];
                    clo = ld3(ch.bmin);
                    ch_levels = ch.levels; ch_wide = ch.wide_off; ch_twig = (uint32_t)ch.twig_off;
                }
                bool contained = inside(p, clo, clo + csize);
                // src/Traverse.cpp:154-155: a position outside the box of the chunk found for it ends the ray.  The shader has no
                // such check (shaders/Chunkmarch.glsl:297-330): its treemarch fails at once, and rootmarch steps on out of that box
                if (GLSL && !contained) tw += guarded(escape(p, g, clo, clo + csize), eps) + eps;     // (stays M_WORLD; cw counts it)
                else miss = !contained;
                if (contained) {                    // treemarch(p, beta, chunk): a = p, t = 0 (src/Traverse.cpp:158,78)
                    if constexpr (BIG) wide_b = (unsigned long long)(size_t)U.wide + ((unsigned long long)ch_wide << 8);
                    else wide_b = ch_wide << 8;                  // 64 entries of 4 bytes per wide node
                    twig_off = ch_twig;
                    levels = (int)ch_levels;
                    O = p; t = 0.0f; cnt = U.cap_tree;
                    Blo = clo;
                    res = csize * __uint_as_float((uint32_t)(127 - levels) << 23);     // csize / 2^levels, exact
                    bsize = csize; res_tree = res; nw = levels ? (levels + 1) >> 1 : 1;
                    mode = M_TREE;
                }
            }
        }
    }
    return vote(miss);
}
};

} // namespace svo

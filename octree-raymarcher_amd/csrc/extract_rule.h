// extract_rule.h — the window of svo_chunk_extract / svo_world_chunk_extract, once, for the host twin (extract.cpp, plain g++) and the
// kernels (extract.hip): the image of a node of C in A, the descent to the root's neighbourhood, what a neighbour hands down and the
// cell of A that a cell of C reads.  The extract is the stamp's inverse and reads the placement as stamp_rule.h does; A is walked in
// its own frame, and the orientation lives on C's side: in the corner of a node's image and in the cell a lane reads.  The hood, the
// "overlapped" test and the neighbour step are stamp_rule.h's.  Integer arithmetic only; no HIP include.
//   C       the result, depth D_C, N_C = 2^D_C: cell q of C is cell offset + d of A, q[pi(i)] = flip_i ? N_C - 1 - d_i : d_i
//   image   of a node of C with corner x and edge e: the cube of A of edge e that its cells read
#pragma once
#include "stamp_rule.h"

namespace svo {

constexpr uint32_t EXTRACT_MIN_DEPTH = STAMP_MIN_DEPTH, EXTRACT_MAX_DEPTH = STAMP_MAX_DEPTH;

// what the walk knows of a call: the placement as the stamp reads it, and C's depth
struct ExtractPlace { StampPlace P; uint32_t depth_c; };

// A's coordinate on axis i of the image of the cube of C with corner x and edge `edge` (a node: 2^shift, a cell: 1)
SVO_MESH_HD int32_t extract_image(const ExtractPlace &E, const uint32_t x[3], uint32_t edge, uint32_t i)
{
    const uint32_t at = x[stamp_pi(E.P, i)];
    return E.P.offset[i] + (int32_t)((E.P.flips >> i) & 1u ? (1u << E.depth_c) - edge - at : at);
}

// The neighbourhood of a node of C with corner x and edge 2^shift: A's nodes of that edge at indices k + j, k = floor(image / edge);
// d is the image's corner.  `unaligned` is the offset's, whatever the node: x and N_C are multiples of the edge
SVO_MESH_HD StampHood extract_hood(const ExtractPlace &E, const uint32_t x[3], uint32_t shift)
{
    StampHood H{ { 0, 0, 0 }, { 0, 0, 0 }, 0u };
    for (uint32_t i = 0; i < 3u; ++i) {
        H.d[i] = extract_image(E, x, 1u << shift, i);
        H.k[i] = H.d[i] >> shift;                            // (arithmetic: the floor, also below 0)
        if (H.d[i] & (int32_t)((1u << shift) - 1u)) H.unaligned |= 1u << i;
    }
    return H;
}

// Neighbour j of C's root: the node of A at level D_A - D_C with index floor(offset / N_C) + j, found from A's root word.  An index
// outside A is EMPTY; EMPTY and LEAF met on the way down are handed on.  follow(w, slot) reads child `slot` of the BRANCH w (the
// device's checks the offset first).  *left: the levels that were not descended - a TWIG with *left > 0 lies above level depth - 2
template <class Follow> SVO_MESH_HD uint32_t extract_root_word(const ExtractPlace &E, uint32_t depth_a, uint32_t j, uint32_t root_a, uint32_t *left, Follow &&follow)
{
    const uint32_t levels = depth_a - E.depth_c;
    int32_t at[3];
    *left = 0u;
    for (uint32_t i = 0; i < 3u; ++i) {
        at[i] = (E.P.offset[i] >> E.depth_c) + (int32_t)((j >> i) & 1u);
        if (at[i] < 0 || at[i] >= (int32_t)(1u << levels)) return node_make(EMPTY, 0);
    }
    uint32_t w = root_a;
    for (*left = levels; *left > 0u && node_type(w) == BRANCH; --*left) {
        const uint32_t bit = *left - 1u;
        w = follow(w, (((uint32_t)at[0] >> bit) & 1u) | (((uint32_t)at[1] >> bit) & 1u) << 1 | (((uint32_t)at[2] >> bit) & 1u) << 2);
    }
    return w;
}

// what the word w of A hands down to its slot (A's own: nothing is permuted): EMPTY and LEAF themselves, a BRANCH its child
template <class Tree> SVO_MESH_HD uint32_t extract_hand_down(uint32_t w, uint32_t slot, Tree &&tree)
{
    return node_type(w) == BRANCH ? tree(node_offset(w) + slot) : w;
}

// At the brick level (edge 4) cell (c0, c1, c2) of C's node with corner x reads neighbour `from`, and in it cell `index` of A's brick
SVO_MESH_HD StampCell extract_cell(const ExtractPlace &E, const StampHood &H, const uint32_t x[3], uint32_t c0, uint32_t c1, uint32_t c2)
{
    const uint32_t cell[3] = { x[0] + c0, x[1] + c1, x[2] + c2 };
    uint32_t s[3];
    for (uint32_t i = 0; i < 3u; ++i) s[i] = (uint32_t)(extract_image(E, cell, 1u, i) - H.k[i] * 4);      // in [0, 8)
    return StampCell{ (s[0] >> 2) | (s[1] >> 2) << 1 | (s[2] >> 2) << 2, (s[0] & 3u) | (s[1] & 3u) << 2 | (s[2] & 3u) << 4 };
}

// an entry is settled where it is met if all overlapped neighbours are uniform with one value: *v is it
SVO_MESH_HD bool extract_settled(const uint32_t nb[8], uint32_t unaligned, uint32_t *v)
{
    *v = combine_value(nb[0]);                              // (neighbour 0 is always overlapped)
    for (uint32_t j = 0; j < 8u; ++j)
        if (stamp_overlapped(j, unaligned) && (!combine_uniform(nb[j]) || combine_value(nb[j]) != *v)) return false;
    return true;
}

} // namespace svo

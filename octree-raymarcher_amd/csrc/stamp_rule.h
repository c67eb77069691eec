// stamp_rule.h — the placement of svo_chunk_stamp / svo_world_chunk_stamp, once, for the host twin (stamp.cpp, plain g++) and the
// kernels (stamp.hip): the orientation's child slot sigma and brick index, the neighbourhood's "overlapped" test and the step from a
// node's 2x2x2 neighbourhood to a child's.  combine_rule.h holds the cell function.  Integer arithmetic only; no HIP include.
//   B'      chunk B in the placement's orientation: cell d of B' is cell q of B, q[pi(i)] = flip_i ? N_B - 1 - d_i : d_i
//   d       a cell or a corner of A relative to the placement's offset, per axis (0: x, 1: y, 2: z); floor division throughout
#pragma once
#include "combine_rule.h"

namespace svo {

constexpr uint32_t STAMP_ORIENTS = 48, STAMP_MIN_DEPTH = 2, STAMP_MAX_DEPTH = 16;
constexpr int32_t STAMP_OFFSET_LIMIT = 65536;
// a virtual ancestor of B's root, met while a node's edge exceeds N_B: its child 0 is the next ancestor or B's root word, its other
// children are EMPTY.  BRANCH | 0 is free for it: a real BRANCH has offset >= 1
constexpr uint32_t STAMP_MARKER = node_make(BRANCH, 0);

// a placement as the walk reads it: sigma(c') in bits [3c', 3c' + 3), pi(i) in bits [2i, 2i + 2)
struct StampPlace { int32_t offset[3]; uint32_t perm, flips, sigma; };

// what both forms ask of a placement: orient 0 .. 47, every offset in [-65536, 65536]
SVO_MESH_HD bool stamp_placement_ok(const int32_t offset[3], uint32_t orient)
{
    for (uint32_t i = 0; i < 3u; ++i) if (offset[i] < -STAMP_OFFSET_LIMIT || offset[i] > STAMP_OFFSET_LIMIT) return false;
    return orient < STAMP_ORIENTS;
}

SVO_MESH_HD uint32_t stamp_pi(const StampPlace &P, uint32_t i) { return (P.perm >> (2u * i)) & 3u; }

// orient = perm * 8 + flips; perm indexes (x,y,z), (x,z,y), (y,x,z), (y,z,x), (z,x,y), (z,y,x), flips has one bit per OUTPUT axis
SVO_MESH_HD StampPlace stamp_place(const int32_t offset[3], uint32_t orient)
{
    // pi(0) | pi(1) << 2 | pi(2) << 4 of the six permutations, eight bits each
    const uint64_t table = 0x24ull | 0x18ull << 8 | 0x21ull << 16 | 0x09ull << 24 | 0x12ull << 32 | 0x06ull << 40;
    StampPlace P{ { offset[0], offset[1], offset[2] }, (uint32_t)(table >> (8u * (orient >> 3))) & 0x3Fu, orient & 7u, 0u };
    // slot c' of B' is B's child whose bit pi(i) is c'_i XOR flip_i
    for (uint32_t c = 0; c < 8u; ++c) {
        uint32_t to = 0u;
        for (uint32_t i = 0; i < 3u; ++i) to |= (((c ^ P.flips) >> i) & 1u) << stamp_pi(P, i);
        P.sigma |= to << (3u * c);
    }
    return P;
}
SVO_MESH_HD uint32_t stamp_sigma(const StampPlace &P, uint32_t c) { return (P.sigma >> (3u * c)) & 7u; }

// the proper orientations (rotations): parity(perm) * (-1)^popcount(flips) = +1.  The permutations 0, 3, 4 of the table are even
SVO_MESH_HD bool stamp_proper(uint32_t orient)
{
    const uint32_t perm = orient >> 3, f = orient & 7u, odd_perm = (perm == 1u || perm == 2u || perm == 5u) ? 1u : 0u;
    return ((odd_perm + (f & 1u) + ((f >> 1) & 1u) + (f >> 2)) & 1u) == 0u;
}

// cell (t0, t1, t2) of a brick of B' as the index of B's brick (z * 16 + y * 4 + x): output axis i reads B's coordinate pi(i)
SVO_MESH_HD uint32_t stamp_brick_index(const StampPlace &P, uint32_t t0, uint32_t t1, uint32_t t2)
{
    const uint32_t f = P.flips;
    return ((f & 1u ? 3u - t0 : t0) << (2u * stamp_pi(P, 0))) | ((f & 2u ? 3u - t1 : t1) << (2u * stamp_pi(P, 1))) | ((f & 4u ? 3u - t2 : t2) << (2u * stamp_pi(P, 2)));
}

// The neighbourhood of a node of A with corner x and edge 2^shift: the nodes of B' of that edge at indices k + j, j in {0,1}^3
// (bit i of j: axis i), k = floor(d / edge), d = x - offset.  `unaligned` has bit i set where d_i mod edge != 0
struct StampHood { int32_t d[3], k[3]; uint32_t unaligned; };
SVO_MESH_HD StampHood stamp_hood(const StampPlace &P, const uint32_t x[3], uint32_t shift)
{
    StampHood H{ { 0, 0, 0 }, { 0, 0, 0 }, 0u };
    for (uint32_t i = 0; i < 3u; ++i) {
        H.d[i] = (int32_t)x[i] - P.offset[i];
        H.k[i] = H.d[i] >> shift;                            // (arithmetic: the floor, also below 0)
        if (H.d[i] & (int32_t)((1u << shift) - 1u)) H.unaligned |= 1u << i;
    }
    return H;
}
// neighbour j is overlapped by the node's region on axis i only if j_i = 0 or d_i mod edge != 0
SVO_MESH_HD bool stamp_overlapped(uint32_t j, uint32_t unaligned) { return (j & ~unaligned) == 0u; }

// the word at index k + j of the root's neighbourhood (A's root has edge N_A >= N_B): B's cube lies in the node at index (0, 0, 0)
SVO_MESH_HD uint32_t stamp_root_word(const StampHood &H, uint32_t j, bool same_edge, uint32_t root_b)
{
    for (uint32_t i = 0; i < 3u; ++i) if (H.k[i] + (int32_t)((j >> i) & 1u) != 0) return node_make(EMPTY, 0);
    return same_edge ? root_b : STAMP_MARKER;
}

// The neighbour step.  A child of the node has the neighbourhood C (one level down); its neighbour j' is slot `slot` of the parent's
// neighbour `from`: floor((k' + j') / 2) - k lies in {0, 1} on every axis
struct StampStep { uint32_t from, slot; };
SVO_MESH_HD StampStep stamp_step(const StampHood &parent, const StampHood &C, uint32_t j)
{
    StampStep S{ 0u, 0u };
    for (uint32_t i = 0; i < 3u; ++i) {
        const int32_t at = C.k[i] + (int32_t)((j >> i) & 1u);
        S.from |= (uint32_t)((at >> 1) - parent.k[i]) << i;
        S.slot |= (uint32_t)(at & 1) << i;
    }
    return S;
}
// what the word w of B' hands down to its slot: EMPTY and LEAF themselves, a BRANCH tree(offset + sigma(slot)), a virtual ancestor
// the next one - or B's root word where the children have B's edge (`to_root`) - in slot 0 and EMPTY elsewhere.  tree(i) reads node
// word i of B (the device's checks the pool's bounds)
template <class Tree> SVO_MESH_HD uint32_t stamp_hand_down(const StampPlace &P, uint32_t w, uint32_t slot, bool to_root, Tree &&tree)
{
    if (w == STAMP_MARKER) return slot != 0u ? node_make(EMPTY, 0) : to_root ? tree(0u) : STAMP_MARKER;
    if (node_type(w) == BRANCH) return tree(node_offset(w) + stamp_sigma(P, slot));
    return w;
}

// At the brick level (edge 4) cell (c0, c1, c2) of the node reads neighbour `from`, and in it the cell `index` of B's brick
struct StampCell { uint32_t from, index; };
SVO_MESH_HD StampCell stamp_cell(const StampPlace &P, const StampHood &H, uint32_t c0, uint32_t c1, uint32_t c2)
{
    const uint32_t s0 = (uint32_t)(H.d[0] & 3) + c0, s1 = (uint32_t)(H.d[1] & 3) + c1, s2 = (uint32_t)(H.d[2] & 3) + c2;
    return StampCell{ (s0 >> 2) | (s1 >> 2) << 1 | (s2 >> 2) << 2, stamp_brick_index(P, s0 & 3u, s1 & 3u, s2 & 3u) };
}

// an entry is settled where it is met if A's word is uniform and all overlapped neighbours are uniform with one value: *b is it
SVO_MESH_HD bool stamp_settled(uint32_t wa, const uint32_t nb[8], uint32_t unaligned, uint32_t *b)
{
    if (!combine_uniform(wa)) return false;
    *b = combine_value(nb[0]);                              // (neighbour 0 is always overlapped)
    for (uint32_t j = 0; j < 8u; ++j)
        if (stamp_overlapped(j, unaligned) && (!combine_uniform(nb[j]) || combine_value(nb[j]) != *b)) return false;
    return true;
}

} // namespace svo

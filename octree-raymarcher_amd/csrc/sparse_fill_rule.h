// sparse_fill_rule.h — the bit arithmetic of svo_chunk_fill_enclosed / svo_world_chunk_fill_enclosed, once, for the host twin
// (sparse_fill.cpp, plain g++) and the kernels (sparse_fill.hip).  Integer arithmetic only; no HIP include.
//   mask    one bit per cell of a brick in the brick's own order: bit cz * 16 + cy * 4 + cx
//   face    f = 2 * axis + side (side 0: the low face, coordinate 0; side 1: the high face, coordinate 3)
#pragma once
#include <cstdint>

#include "mesh_rule.h"
#include "svo_format.h"

namespace svo {

constexpr uint64_t FILL_X0 = 0x1111111111111111ull, FILL_X3 = 0x8888888888888888ull;
constexpr uint64_t FILL_Y0 = 0x000F000F000F000Full, FILL_Y3 = 0xF000F000F000F000ull;
constexpr uint64_t FILL_Z0 = 0x000000000000FFFFull, FILL_Z3 = 0xFFFF000000000000ull;

// a node word that holds no material: EMPTY, or LEAF | 0 ("a value of 0 is empty however it is stored")
SVO_MESH_HD bool fill_is_empty(uint32_t w) { return node_type(w) == EMPTY || (node_type(w) == LEAF && (node_offset(w) & 0xFFFFu) == 0u); }

// the cells of face f
SVO_MESH_HD uint64_t fill_face(uint32_t f)
{
    return f == 0u ? FILL_X0 : f == 1u ? FILL_X3 : f == 2u ? FILL_Y0 : f == 3u ? FILL_Y3 : f == 4u ? FILL_Z0 : FILL_Z3;
}
// `bits` of a brick, seen through its face f, as the cells of the opposite face of the brick behind that face
SVO_MESH_HD uint64_t fill_face_pull(uint64_t bits, uint32_t f)
{
    const uint32_t shift = f < 2u ? 3u : f < 4u ? 12u : 48u;
    const uint64_t mine = bits & fill_face(f);
    return (f & 1u) ? mine >> shift : mine << shift;
}
// the cells of the brick at corner (x, y, z) that have a coordinate of 0 or N - 1
SVO_MESH_HD uint64_t fill_border_cells(uint32_t x, uint32_t y, uint32_t z, uint32_t N)
{
    return (x == 0u ? FILL_X0 : 0ull) | (x + TWIG_SIZE == N ? FILL_X3 : 0ull) | (y == 0u ? FILL_Y0 : 0ull) | (y + TWIG_SIZE == N ? FILL_Y3 : 0ull) |
           (z == 0u ? FILL_Z0 : 0ull) | (z + TWIG_SIZE == N ? FILL_Z3 : 0ull);
}
// the flood inside one brick to its fixed point: `seed` (a subset of `empty`) and every empty cell that 6-neighbour steps through
// empty cells connect to it
SVO_MESH_HD uint64_t fill_flood_brick(uint64_t seed, uint64_t empty)
{
    uint64_t o = seed & empty;
    for (;;) {
        const uint64_t n = (o | ((o & ~FILL_X3) << 1) | ((o & ~FILL_X0) >> 1) | ((o & ~FILL_Y3) << 4) | ((o & ~FILL_Y0) >> 4) | (o << 16) | (o >> 16)) & empty;
        if (n == o) return o;
        o = n;
    }
}
// the result word of a brick whose cells `in` (a subset of its empty ones) take `material`: the LEAF of its one value, EMPTY if that is
// 0, TWIG | 0 if it holds several
SVO_MESH_HD uint32_t fill_brick_result(const uint16_t *cells, uint64_t in, uint32_t material)
{
    const uint32_t first = (in & 1ull) ? material : cells[0];
    for (uint32_t i = 1; i < TWIG_WORDS; ++i)
        if (((in >> i) & 1ull ? material : (uint32_t)cells[i]) != first) return node_make(TWIG, 0);
    return first ? node_make(LEAF, first) : node_make(EMPTY, 0);
}

} // namespace svo

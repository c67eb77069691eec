// sparse_mesh_rule.h — the packed word of svo_chunk_from_mesh / svo_world_chunk_from_mesh, once, for the host twin
// (sparse_mesh.cpp, plain g++) and the kernels (sparse_mesh.hip).  Integer arithmetic only; no HIP include.
//   key     the Morton code of cell (x, y, z) of a (2^depth)^3 grid, 3 * depth bits: bit 3b of x's bit b, 3b + 1 of y's, 3b + 2 of z's.
//           A child's slot is x + 2y + 4z, so the node of level L that holds the cell is key >> 3 * (depth - L), its slot in its
//           parent the low three bits of that, and ascending keys are the FIFO walk's visiting order within every level
//   word    key << 16 | material: one ascending sort puts a cell's largest material last among its duplicates (depth 16: 64 bits)
//   brick   the low six key bits of a cell are its place in its 4^3 block; the brick's index is cz*16 + cy*4 + cx
#pragma once
#include <cstdint>

#include "mesh_rule.h"

namespace svo {

constexpr uint32_t SPARSE_MATERIAL_BITS = 16;
constexpr uint64_t SPARSE_MAX_WORDS = 0x7FFFFFFFull;       // an overlap list of this many words or more is refused (the sort's item count)

// bit b of v (16 bits) to bit 3b
SVO_MESH_HD uint64_t sparse_spread(uint32_t v)
{
    uint64_t x = v & 0xFFFFu;
    x = (x | (x << 16)) & 0x0000FF0000FFull;
    x = (x | (x << 8)) & 0x00F00F00F00Full;
    x = (x | (x << 4)) & 0x0C30C30C30C3ull;
    x = (x | (x << 2)) & 0x249249249249ull;
    return x;
}
SVO_MESH_HD uint64_t sparse_key(uint32_t x, uint32_t y, uint32_t z) { return sparse_spread(x) | (sparse_spread(y) << 1) | (sparse_spread(z) << 2); }
SVO_MESH_HD uint64_t sparse_word(uint32_t x, uint32_t y, uint32_t z, uint32_t material) { return (sparse_key(x, y, z) << SPARSE_MATERIAL_BITS) | material; }
SVO_MESH_HD uint64_t sparse_word_key(uint64_t word) { return word >> SPARSE_MATERIAL_BITS; }
SVO_MESH_HD uint32_t sparse_word_material(uint64_t word) { return (uint32_t)word & 0xFFFFu; }
SVO_MESH_HD uint64_t sparse_word_block(uint64_t word) { return word >> (SPARSE_MATERIAL_BITS + 6); }     // the key of its 4^3 block
// where the cell of `word` sits in its block's brick
SVO_MESH_HD uint32_t sparse_brick_index(uint64_t word)
{
    const uint32_t k = (uint32_t)(word >> SPARSE_MATERIAL_BITS) & 63u;
    const uint32_t cx = (k & 1u) | ((k >> 2) & 2u), cy = ((k >> 1) & 1u) | ((k >> 3) & 2u), cz = ((k >> 2) & 1u) | ((k >> 4) & 2u);
    return cz * 16u + cy * 4u + cx;
}

} // namespace svo

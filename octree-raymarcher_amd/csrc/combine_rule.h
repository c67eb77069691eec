// combine_rule.h — the cell function of svo_chunk_combine / svo_world_chunk_combine, once, for the host twin (combine.cpp, plain g++)
// and the kernels (combine.hip), and the words both fold into.  Integer arithmetic only; no HIP include.
//   a, b    the values of one cell of chunk A and of chunk B (0: empty, however it is stored)
//   op      SVO_COMBINE_* of include/svo.h
#pragma once
#include <cstdint>

#include "mesh_rule.h"
#include "svo_format.h"

namespace svo {

enum : uint32_t { COMBINE_MAX = 0, COMBINE_UNDER = 1, COMBINE_OVER = 2, COMBINE_SUBTRACT = 3, COMBINE_INTERSECT = 4, COMBINE_OPS = 5 };

// f_op(a, b): what the cell holds afterwards
SVO_MESH_HD uint32_t combine_cell(uint32_t op, uint32_t a, uint32_t b)
{
    switch (op) {
    case COMBINE_MAX:       return a > b ? a : b;           // svo_grid_add_mesh's merge
    case COMBINE_UNDER:     return a != 0u ? a : b;         // SVO_EDIT_BUILD: B only where A is empty
    case COMBINE_OVER:      return b != 0u ? b : a;         // SVO_EDIT_REPLACE: B on top
    case COMBINE_SUBTRACT:  return b != 0u ? 0u : a;        // SVO_EDIT_DESTROY: B's shape carved out of A
    default:                return b != 0u ? a : 0u;        // COMBINE_INTERSECT: A where B is
    }
}

// a node word that is neither BRANCH nor TWIG covers its cube with one value: EMPTY 0, LEAF offset & 0xFFFF
SVO_MESH_HD bool combine_uniform(uint32_t w) { return node_type(w) == EMPTY || node_type(w) == LEAF; }
SVO_MESH_HD uint32_t combine_value(uint32_t w) { return node_type(w) == LEAF ? node_offset(w) & 0xFFFFu : 0u; }
// the word of a cube that holds the one value v
SVO_MESH_HD uint32_t combine_word(uint32_t v) { return v != 0u ? node_make(LEAF, v) : node_make(EMPTY, 0); }

} // namespace svo

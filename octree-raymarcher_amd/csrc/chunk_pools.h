// chunk_pools.h — what the host code that reads or produces a chunk's pools shares: the forward validation pass over the node words,
// the FIFO emit over per-node result words, and the svo_chunk_desc a producer hands out.  Header-only plain C++, no HIP include: the
// sanitizer programs under host/ compile it with whichever .cpp includes it.  world.h includes it at its end (validate_chunk's pass
// comes with its declaration), so it needs world.h's declarations and nothing else of the project.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "world.h"

namespace svo {

// what the tree rebuilders (fill, combine; host and device) say to a brick above the last level
constexpr const char *SHALLOW_TWIG_WHY = "a TWIG above level depth-2 (a sparsely refined chunk) is not supported";

// One forward pass over the node words of a chunk of `depth` >= 2 whose `trees` are 1 + 8k.  Accepts what grow() and the box edits
// produce (child blocks lie after their parent, at indices 1 + 8k); names the first word a kernel could run off: an offset outside
// its pool, a back edge (a cycle), a block with two parents, a BRANCH below level depth-2.  Blocks no reachable BRANCH points at
// (orphans left behind by Ocroot::destroy) are ignored.  Returns that word's `why`, or null.  *shallow (if asked for) is set when a
// TWIG above level depth-2 was met before the pass stopped; what that means is the caller's: the fill and combine refuse it, a world
// holds it.
inline const char *pools_walk(const uint32_t *tree, uint64_t trees, uint64_t twigs, uint32_t depth, bool *shallow)
{
    const uint32_t maxlevel = depth - TWIG_LEVELS;
    std::vector<int8_t> block_level((trees - 1) / 8, (int8_t)-1);
    for (uint64_t i = 0; i < trees; ++i) {
        const int level = i ? block_level[(i - 1) / 8] : 0;
        if (level < 0) continue;                            // an orphan: nothing reaches it
        const uint64_t off = node_offset(tree[i]);
        if (node_type(tree[i]) == BRANCH) {
            if ((uint32_t)level >= maxlevel) return "BRANCH below level depth-2";
            if (off <= i || off + 8 > trees || (off - 1) % 8 != 0) return "BRANCH offset outside pool or not a forward 8-block";
            if (block_level[(off - 1) / 8] >= 0) return "child block referenced twice";
            block_level[(off - 1) / 8] = (int8_t)(level + 1);
        } else if (node_type(tree[i]) == TWIG) {
            if (off >= twigs) return "TWIG offset outside brick pool";
            if ((uint32_t)level != maxlevel && shallow) *shallow = true;
        }
    }
    return nullptr;
}

// The FIFO walk of svo_chunk_from_grid over result words that some fold left per id (a node, a pair): the pools come out minimal
// and in visiting order whatever the input was.  res(id) is the id's result word (BRANCH / TWIG without an offset), child(id, c)
// the id of child c of an id whose result is a BRANCH, cells(id, otwig) appends the 64 cells of an id whose result is a TWIG.
template <class Id, class Res, class Child, class Cells>
void emit_fifo(Id root, Res res, Child child, Cells cells, std::vector<uint32_t> &otree, std::vector<uint16_t> &otwig)
{
    struct Out { Id id; uint32_t at; };
    otree.assign(1, node_make(EMPTY, 0));
    otwig.clear();
    std::vector<Out> level(1, Out{ root, 0 }), next;
    while (!level.empty()) {
        next.clear();
        for (const Out &o : level) {
            const uint32_t r = res(o.id);
            if (node_type(r) == TWIG) {
                otree[o.at] = node_make(TWIG, (uint32_t)(otwig.size() / TWIG_WORDS));
                cells(o.id, otwig);
            } else if (node_type(r) == BRANCH) {
                const uint32_t first = (uint32_t)otree.size();
                otree[o.at] = node_make(BRANCH, first);
                otree.resize(otree.size() + 8, node_make(EMPTY, 0));
                for (uint32_t c = 0; c < 8; ++c) next.push_back(Out{ child(o.id, c), first + c });
            } else otree[o.at] = r;
        }
        level.swap(next);
    }
}

// *out takes malloc'd copies of the two pools (svo_chunk_free frees them; the brick pool is allocated even when it holds nothing)
// and the frame; 0, or SVO_ERR_OUT_OF_MEMORY with *out untouched
inline int chunk_desc_take(svo_chunk_desc *out, const float position[3], float size, uint32_t depth, const std::vector<uint32_t> &tree,
                           const std::vector<uint16_t> &twig, const char *who)
{
    uint32_t *t = (uint32_t *)std::malloc(tree.size() * sizeof(uint32_t));
    uint16_t *b = (uint16_t *)std::malloc(std::max<size_t>(twig.size(), TWIG_WORDS) * sizeof(uint16_t));
    if (!t || !b) { std::free(t); std::free(b); set_error(std::string(who) + ": out of memory"); return SVO_ERR_OUT_OF_MEMORY; }
    std::memcpy(t, tree.data(), tree.size() * sizeof(uint32_t));
    if (!twig.empty()) std::memcpy(b, twig.data(), twig.size() * sizeof(uint16_t));
    std::memcpy(out->position, position, sizeof out->position);
    out->size = size; out->depth = depth; out->_pad = 0;
    out->tree = t; out->trees = tree.size();
    out->twig = b; out->twigs = twig.size() / TWIG_WORDS;
    return SVO_OK;
}

} // namespace svo

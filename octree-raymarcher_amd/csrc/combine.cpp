// combine.cpp — svo_chunk_combine: two chunks of one depth combined cell by cell on their trees, on the host.  The readable statement of
// the chunk CSG and the twin of combine.hip; depth 2 .. 16.  combine_rule.h holds the cell function f_op.
//   walk    recursive over PAIRS of node words (w_A, w_B) from the two roots.  A side that is EMPTY or LEAF hands its own word down to
//           all eight children, a BRANCH hands down tree[offset + c]; a pair is descended iff either side is a BRANCH.  The rule has no
//           geometry, so a pair carries no corner
//   fold    on the way back, a result word per pair: two uniform sides give the word of f(a, b) and edge^3 changed cells if that
//           differs from a; at level depth-2 a TWIG on either side gives 64 cells f(a, b), one value among them its LEAF / EMPTY, several
//           TWIG | 0; a descended pair whose eight results are one EMPTY / LEAF word is that word, else BRANCH | 0
//   emit    the FIFO walk over the results (chunk_pools.h: emit_fifo, which also holds the validation pass and the desc's producer)
// Working memory is proportional to the node words and the bricks the two roots reach; nothing has N^3 entries.  No HIP include: plain
// g++ compiles this file (host/combine_check.cpp runs it under the sanitizers), and it links without world.cpp.
#include <cmath>
#include <new>

#include "chunk_pools.h"
#include "combine_rule.h"

namespace svo {

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;

struct Side { const uint32_t *tree; const uint16_t *twig; };

struct Combine {
    Side A, B;
    uint32_t op, maxlevel, N;
    // a visited pair: its two words, its result (BRANCH / TWIG without an offset) and what hangs below it - the first of its eight
    // child pairs (a BRANCH result) or its 64 cells in `cells` (a TWIG result)
    struct Pair { uint32_t wa, wb, res, below; };
    std::vector<Pair> pairs;
    std::vector<uint16_t> cells;
    uint64_t changed = 0;

    uint32_t visit(uint32_t at, uint32_t level)
    {
        const uint32_t wa = pairs[at].wa, wb = pairs[at].wb;
        uint32_t r, below = NONE;
        if (node_type(wa) == BRANCH || node_type(wb) == BRANCH) {               // (above level depth-2: the validation saw to it)
            below = (uint32_t)pairs.size();
            for (uint32_t c = 0; c < 8; ++c)
                pairs.push_back(Pair{ node_type(wa) == BRANCH ? A.tree[node_offset(wa) + c] : wa, node_type(wb) == BRANCH ? B.tree[node_offset(wb) + c] : wb, 0, NONE });
            uint32_t first = 0;
            bool one = true;
            for (uint32_t c = 0; c < 8; ++c) {
                const uint32_t k = visit(below + c, level + 1);
                if (c == 0) first = k;
                one = one && k == first;
            }
            r = one && combine_uniform(first) ? first : node_make(BRANCH, 0);
        } else if (node_type(wa) == TWIG || node_type(wb) == TWIG) {            // (at level depth-2)
            const uint16_t *ca = node_type(wa) == TWIG ? A.twig + (size_t)node_offset(wa) * TWIG_WORDS : nullptr;
            const uint16_t *cb = node_type(wb) == TWIG ? B.twig + (size_t)node_offset(wb) * TWIG_WORDS : nullptr;
            uint16_t out[TWIG_WORDS];
            bool one = true;
            for (uint32_t i = 0; i < TWIG_WORDS; ++i) {
                const uint32_t a = ca ? ca[i] : combine_value(wa), b = cb ? cb[i] : combine_value(wb);
                out[i] = (uint16_t)combine_cell(op, a, b);
                changed += out[i] != a;
                one = one && out[i] == out[0];
            }
            if (one) r = combine_word(out[0]);
            else {
                r = node_make(TWIG, 0);
                below = (uint32_t)(cells.size() / TWIG_WORDS);
                cells.insert(cells.end(), out, out + TWIG_WORDS);
            }
        } else {
            const uint32_t a = combine_value(wa), v = combine_cell(op, a, combine_value(wb));
            const uint64_t e = N >> level;
            if (v != a) changed += e * e * e;
            r = combine_word(v);
        }
        pairs[at].below = below;
        return pairs[at].res = r;
    }

    void emit(std::vector<uint32_t> &otree, std::vector<uint16_t> &otwig) const
    {
        emit_fifo(0u, [&](uint32_t at) { return pairs[at].res; }, [&](uint32_t at, uint32_t c) { return pairs[at].below + c; },
                  [&](uint32_t at, std::vector<uint16_t> &to) {
                      const auto first = cells.begin() + (size_t)pairs[at].below * TWIG_WORDS;
                      to.insert(to.end(), first, first + TWIG_WORDS);
                  }, otree, otwig);
    }
};

// one chunk's pools, for a depth in [2, 16], against what a world asks of them (chunk_pools.h: pools_walk): 0, or SVO_ERR_INVALID_ARG
// with the message set - any malformed word, wherever a shallow TWIG lies.  *shallow: the root reaches a TWIG above level depth-2
int pools_status(const svo_chunk_desc &c, const char *who, const char *which, bool *shallow)
{
    const char *why = (c.trees - 1) % 8 != 0 || c.trees > (1ull << 30) || c.twigs > (1ull << 30) ? "the tree pool is not 1 + 8k node words"
                                                                                                  : pools_walk(c.tree, c.trees, c.twigs, c.depth, shallow);
    if (!why) return SVO_OK;
    set_error(std::string(who) + ": chunk " + which + ": " + why);
    return SVO_ERR_INVALID_ARG;
}

bool depth_ok(uint32_t depth) { return depth >= SVO_COMBINE_MIN_DEPTH && depth <= SVO_COMBINE_MAX_DEPTH; }

} // namespace

} // namespace svo

extern "C" {

int svo_chunk_combine(const svo_chunk_desc *a, const svo_chunk_desc *b, int op, svo_chunk_desc *out, uint64_t *changed_out)
{
    using namespace svo;
    const char *who = "svo_chunk_combine";
    const auto pools = [](const svo_chunk_desc *c) { return c->tree && c->trees != 0 && (c->twigs == 0 || c->twig); };
    if (!a || !b || !out || out == a || out == b || op < 0 || op >= (int)COMBINE_OPS || !pools(a) || !pools(b) || !(a->size > 0.0f) || !std::isfinite(a->size)) {
        set_error(std::string(who) + ": bad argument (a, b and out, out neither of the two; a known op; pools; a positive finite size of a)");
        return SVO_ERR_INVALID_ARG;
    }
    try {
        bool shallow = false;
        if (depth_ok(a->depth)) if (const int rc = pools_status(*a, who, "a", &shallow)) return rc;
        if (depth_ok(b->depth)) if (const int rc = pools_status(*b, who, "b", &shallow)) return rc;
        if (a->depth != b->depth) { set_error(std::string(who) + ": the two chunks differ in depth"); return SVO_ERR_UNSUPPORTED; }
        if (!depth_ok(a->depth)) { set_error(std::string(who) + ": the chunks' depth is outside [2, 16]"); return SVO_ERR_UNSUPPORTED; }
        if (shallow) { set_error(std::string(who) + ": " + SHALLOW_TWIG_WHY); return SVO_ERR_UNSUPPORTED; }
        Combine K;
        K.A = Side{ a->tree, a->twig }; K.B = Side{ b->tree, b->twig };
        K.op = (uint32_t)op; K.maxlevel = a->depth - TWIG_LEVELS; K.N = 1u << a->depth;
        K.pairs.reserve((size_t)a->trees + (size_t)b->trees);          // every descended pair holds a BRANCH of a or of b that no other pair holds
        K.pairs.push_back(Combine::Pair{ a->tree[0], b->tree[0], 0, NONE });
        K.visit(0, 0);
        std::vector<uint32_t> tree;
        std::vector<uint16_t> twig;
        K.emit(tree, twig);
        if (tree.size() > (1ull << 30) || twig.size() / TWIG_WORDS > (1ull << 30)) { set_error(std::string(who) + ": 2^30 nodes or bricks"); return SVO_ERR_UNSUPPORTED; }
        if (const int rc = chunk_desc_take(out, a->position, a->size, a->depth, tree, twig, who)) return rc;
        if (changed_out) *changed_out = K.changed;
        return SVO_OK;
    } catch (const std::bad_alloc &) {
        set_error(std::string(who) + ": out of host memory");
        return SVO_ERR_OUT_OF_MEMORY;
    }
}

} // extern "C"

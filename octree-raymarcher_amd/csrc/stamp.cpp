// stamp.cpp — svo_chunk_stamp: chunk B placed into chunk A at an integer cell offset, in one of the 48 orientations of the cube,
// through one of the SVO_COMBINE_* rules, on the two trees, on the host.  The readable statement of the stamp and the twin of
// stamp.hip; depth 2 .. 16, D_B <= D_A.  stamp_rule.h holds the placement (sigma, the brick index, the neighbour step), combine_rule.h
// the cell function f_op.
//   walk    recursive over ENTRIES: a node word of A with its corner and edge e, and the 2x2x2 neighbourhood of the words of the
//           oriented B's nodes of edge e that its region can overlap.  A's side hands down as in combine.cpp; each of a child's eight
//           neighbours is a child of one of the parent's eight (stamp_step, stamp_hand_down).  An entry whose A word is uniform and
//           whose overlapped neighbours are uniform with one value is settled where it is met; every other entry above edge 4 is
//           descended - also where neither tree has a BRANCH: two uniform neighbours of different value make a region mixed down to
//           the bricks, so the entries follow the RESULT, not trees_A + trees_B
//   fold    as combine.cpp's; at edge 4 the 64 cells f(a, b), each cell's b read from the neighbour it falls into
//   emit    the FIFO walk over the results (chunk_pools.h: emit_fifo)
// Working memory is proportional to the entries; nothing has N^3 entries.  No HIP include: plain g++ compiles this file
// (host/stamp_check.cpp runs it under the sanitizers), and it links without world.cpp.
#include <cmath>
#include <new>

#include "chunk_pools.h"
#include "stamp_rule.h"

namespace svo {

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
struct TooManyEntries {};

struct Stamp {
    const uint32_t *ta, *tb;
    const uint16_t *ka, *kb;
    StampPlace P;
    uint32_t op, depth_a, depth_b;
    // a visited entry: A's word, the neighbourhood, the result (BRANCH / TWIG without an offset) and what hangs below it - the first
    // of its eight children (a BRANCH result) or its 64 cells in `cells` (a TWIG result)
    struct Entry { uint32_t wa, nb[8], res, below; };
    std::vector<Entry> entries;
    std::vector<uint16_t> cells;
    uint64_t changed = 0;

    uint32_t visit(uint32_t at, const uint32_t x[3], uint32_t shift)
    {
        const Entry E = entries[at];                        // (a copy: the vector grows below)
        const StampHood H = stamp_hood(P, x, shift);
        uint32_t r, below = NONE, b = 0;
        if (stamp_settled(E.wa, E.nb, H.unaligned, &b)) {
            const uint32_t a = combine_value(E.wa), v = combine_cell(op, a, b);
            const uint64_t e = 1ull << shift;
            if (v != a) changed += e * e * e;
            r = combine_word(v);
        } else if (shift > TWIG_LEVELS) {
            if (entries.size() + 8 > (1ull << 30)) throw TooManyEntries{};
            below = (uint32_t)entries.size();
            const uint32_t h = 1u << (shift - 1);
            for (uint32_t c = 0; c < 8; ++c) {
                const uint32_t xc[3] = { x[0] + (c & 1u) * h, x[1] + ((c >> 1) & 1u) * h, x[2] + (c >> 2) * h };
                const StampHood C = stamp_hood(P, xc, shift - 1);
                Entry K{ node_type(E.wa) == BRANCH ? ta[node_offset(E.wa) + c] : E.wa, {}, 0, NONE };
                for (uint32_t j = 0; j < 8; ++j) {
                    const StampStep S = stamp_step(H, C, j);
                    K.nb[j] = stamp_hand_down(P, E.nb[S.from], S.slot, shift - 1 == depth_b, [&](uint32_t i) { return tb[i]; });
                }
                entries.push_back(K);
            }
            uint32_t first = 0;
            bool one = true;
            for (uint32_t c = 0; c < 8; ++c) {
                const uint32_t xc[3] = { x[0] + (c & 1u) * h, x[1] + ((c >> 1) & 1u) * h, x[2] + (c >> 2) * h };
                const uint32_t k = visit(below + c, xc, shift - 1);
                if (c == 0) first = k;
                one = one && k == first;
            }
            r = one && combine_uniform(first) ? first : node_make(BRANCH, 0);
        } else {                                            // edge 4: a TWIG in A or in an overlapped neighbour, or two values among them
            const uint16_t *ca = node_type(E.wa) == TWIG ? ka + (size_t)node_offset(E.wa) * TWIG_WORDS : nullptr;
            uint16_t out[TWIG_WORDS];
            bool one = true;
            for (uint32_t i = 0; i < TWIG_WORDS; ++i) {
                const StampCell at_b = stamp_cell(P, H, i & 3u, (i >> 2) & 3u, i >> 4);
                const uint32_t wb = E.nb[at_b.from];
                const uint32_t a = ca ? ca[i] : combine_value(E.wa);
                const uint32_t vb = node_type(wb) == TWIG ? kb[(size_t)node_offset(wb) * TWIG_WORDS + at_b.index] : combine_value(wb);
                out[i] = (uint16_t)combine_cell(op, a, vb);
                changed += out[i] != a;
                one = one && out[i] == out[0];
            }
            if (one) r = combine_word(out[0]);
            else {
                r = node_make(TWIG, 0);
                below = (uint32_t)(cells.size() / TWIG_WORDS);
                cells.insert(cells.end(), out, out + TWIG_WORDS);
            }
        }
        entries[at].below = below;
        return entries[at].res = r;
    }

    void emit(std::vector<uint32_t> &otree, std::vector<uint16_t> &otwig) const
    {
        emit_fifo(0u, [&](uint32_t at) { return entries[at].res; }, [&](uint32_t at, uint32_t c) { return entries[at].below + c; },
                  [&](uint32_t at, std::vector<uint16_t> &to) {
                      const auto first = cells.begin() + (size_t)entries[at].below * TWIG_WORDS;
                      to.insert(to.end(), first, first + TWIG_WORDS);
                  }, otree, otwig);
    }
};

// one chunk's pools against what a world asks of them, as combine.cpp's: 0, or SVO_ERR_INVALID_ARG with the message set
int pools_status(const svo_chunk_desc &c, const char *who, const char *which, bool *shallow)
{
    const char *why = (c.trees - 1) % 8 != 0 || c.trees > (1ull << 30) || c.twigs > (1ull << 30) ? "the tree pool is not 1 + 8k node words"
                                                                                                  : pools_walk(c.tree, c.trees, c.twigs, c.depth, shallow);
    if (!why) return SVO_OK;
    set_error(std::string(who) + ": chunk " + which + ": " + why);
    return SVO_ERR_INVALID_ARG;
}

bool depth_ok(uint32_t depth) { return depth >= STAMP_MIN_DEPTH && depth <= STAMP_MAX_DEPTH; }

} // namespace

} // namespace svo

extern "C" {

int svo_chunk_stamp(const svo_chunk_desc *a, const svo_chunk_desc *b, const svo_placement *pl, int op, svo_chunk_desc *out, uint64_t *changed_out)
{
    using namespace svo;
    const char *who = "svo_chunk_stamp";
    const auto pools = [](const svo_chunk_desc *c) { return c->tree && c->trees != 0 && (c->twigs == 0 || c->twig); };
    if (!a || !b || !out || out == a || out == b || op < 0 || op >= (int)COMBINE_OPS || !pools(a) || !pools(b) || !(a->size > 0.0f) || !std::isfinite(a->size) ||
        !pl || !stamp_placement_ok(pl->offset, pl->orient)) {
        set_error(std::string(who) + ": bad argument (a, b and out, out neither of the two; a known op; pools; a positive finite size of a; a placement with orient <= 47 and "
                                     "offsets in [-65536, 65536])");
        return SVO_ERR_INVALID_ARG;
    }
    try {
        bool shallow = false;
        if (depth_ok(a->depth)) if (const int rc = pools_status(*a, who, "a", &shallow)) return rc;
        if (depth_ok(b->depth)) if (const int rc = pools_status(*b, who, "b", &shallow)) return rc;
        if (b->depth > a->depth) { set_error(std::string(who) + ": chunk b is deeper than chunk a"); return SVO_ERR_UNSUPPORTED; }
        if (!depth_ok(a->depth) || !depth_ok(b->depth)) { set_error(std::string(who) + ": a chunk's depth is outside [2, 16]"); return SVO_ERR_UNSUPPORTED; }
        if (shallow) { set_error(std::string(who) + ": " + SHALLOW_TWIG_WHY); return SVO_ERR_UNSUPPORTED; }
        Stamp K{ a->tree, b->tree, a->twig, b->twig, stamp_place(pl->offset, pl->orient), (uint32_t)op, a->depth, b->depth, {}, {}, 0 };
        const uint32_t x[3] = { 0, 0, 0 };
        const StampHood H = stamp_hood(K.P, x, a->depth);
        Stamp::Entry root{ a->tree[0], {}, 0, NONE };
        for (uint32_t j = 0; j < 8; ++j) root.nb[j] = stamp_root_word(H, j, a->depth == b->depth, b->tree[0]);
        K.entries.push_back(root);
        K.visit(0, x, a->depth);
        std::vector<uint32_t> tree;
        std::vector<uint16_t> twig;
        K.emit(tree, twig);
        if (tree.size() > (1ull << 30) || twig.size() / TWIG_WORDS > (1ull << 30)) { set_error(std::string(who) + ": 2^30 nodes or bricks"); return SVO_ERR_UNSUPPORTED; }
        if (const int rc = chunk_desc_take(out, a->position, a->size, a->depth, tree, twig, who)) return rc;
        if (changed_out) *changed_out = K.changed;
        return SVO_OK;
    } catch (const TooManyEntries &) {
        set_error(std::string(who) + ": 2^30 entries");
        return SVO_ERR_UNSUPPORTED;
    } catch (const std::bad_alloc &) {
        set_error(std::string(who) + ": out of host memory");
        return SVO_ERR_OUT_OF_MEMORY;
    }
}

} // extern "C"

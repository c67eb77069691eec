// extract.cpp — svo_chunk_extract: a cube of N_C^3 cells copied out of chunk A at an integer cell offset, in one of the 48
// orientations of the cube, into a chunk C of depth D_C <= D_A, on the tree, on the host.  The inverse of svo_chunk_stamp (stamp.cpp),
// the readable statement of the extract and the twin of extract.hip; depth 2 .. 16.  extract_rule.h holds the window: a node's image
// in A, the descent to the root's neighbourhood, the cell a cell of C reads.
//   walk    recursive over ENTRIES: a node of C with its corner and edge e, and the 2x2x2 neighbourhood of the words of A's nodes of
//           edge e that its image can overlap.  The root's neighbourhood is found by a descent of D_A - D_C levels from A's root
//           (extract_root_word); each of a child's eight neighbours is a child of one of the parent's eight (stamp_step,
//           extract_hand_down).  An entry whose overlapped neighbours are uniform with one value is settled where it is met; every
//           other entry above edge 4 is descended, so the entries follow the RESULT
//   fold    a descended entry whose children came back as one uniform word is that word; at edge 4 the 64 cells, each read from the
//           neighbour its image falls into
//   emit    the FIFO walk over the results (chunk_pools.h: emit_fifo)
// Working memory is proportional to the entries; nothing has N^3 entries, and every array is a std::vector.  No HIP include: plain
// g++ compiles this file (host/extract_check.cpp runs it under the sanitizers), and it links without world.cpp.
#include <cmath>
#include <new>

#include "chunk_pools.h"
#include "extract_rule.h"

namespace svo {

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
struct TooManyEntries {};

struct Extract {
    const uint32_t *ta;
    const uint16_t *ka;
    ExtractPlace E;
    // a visited entry: the neighbourhood, the result (BRANCH / TWIG without an offset) and what hangs below it - the first of its
    // eight children (a BRANCH result) or its 64 cells in `cells` (a TWIG result)
    struct Entry { uint32_t nb[8], res, below; };
    std::vector<Entry> entries;
    std::vector<uint16_t> cells;
    uint64_t occupied = 0;

    uint32_t visit(uint32_t at, const uint32_t x[3], uint32_t shift)
    {
        const Entry N = entries[at];                        // (a copy: the vector grows below)
        const StampHood H = extract_hood(E, x, shift);
        uint32_t r, below = NONE, v = 0;
        if (extract_settled(N.nb, H.unaligned, &v)) {
            const uint64_t e = 1ull << shift;
            if (v != 0) occupied += e * e * e;
            r = combine_word(v);
        } else if (shift > TWIG_LEVELS) {
            if (entries.size() + 8 > (1ull << 30)) throw TooManyEntries{};
            below = (uint32_t)entries.size();
            const uint32_t h = 1u << (shift - 1);
            for (uint32_t c = 0; c < 8; ++c) {
                const uint32_t xc[3] = { x[0] + (c & 1u) * h, x[1] + ((c >> 1) & 1u) * h, x[2] + (c >> 2) * h };
                const StampHood C = extract_hood(E, xc, shift - 1);
                Entry K{ {}, 0, NONE };
                for (uint32_t j = 0; j < 8; ++j) {
                    const StampStep S = stamp_step(H, C, j);
                    K.nb[j] = extract_hand_down(N.nb[S.from], S.slot, [&](uint32_t i) { return ta[i]; });
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
        } else {                                            // edge 4: a TWIG in an overlapped neighbour, or two values among them
            uint16_t out[TWIG_WORDS];
            bool one = true;
            for (uint32_t i = 0; i < TWIG_WORDS; ++i) {
                const StampCell from = extract_cell(E, H, x, i & 3u, (i >> 2) & 3u, i >> 4);
                const uint32_t wa = N.nb[from.from];
                out[i] = (uint16_t)(node_type(wa) == TWIG ? ka[(size_t)node_offset(wa) * TWIG_WORDS + from.index] : combine_value(wa));
                occupied += out[i] != 0;
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

bool depth_ok(uint32_t depth) { return depth >= EXTRACT_MIN_DEPTH && depth <= EXTRACT_MAX_DEPTH; }

} // namespace

} // namespace svo

extern "C" {

int svo_chunk_extract(const svo_chunk_desc *a, const svo_placement *pl, uint32_t depth, const float position[3], float size, svo_chunk_desc *out, uint64_t *occupied_out)
{
    using namespace svo;
    const char *who = "svo_chunk_extract";
    if (!a || !out || out == a || !a->tree || a->trees == 0 || (a->twigs != 0 && !a->twig) || !position || !(size > 0.0f) || !std::isfinite(size) || !pl ||
        !stamp_placement_ok(pl->offset, pl->orient)) {
        set_error(std::string(who) + ": bad argument (a and out, out not a; pools; a position and a positive finite size; a placement with orient <= 47 and offsets in "
                                     "[-65536, 65536])");
        return SVO_ERR_INVALID_ARG;
    }
    try {
        bool shallow = false;
        if (depth_ok(a->depth)) {                           // what svo_world_create's validation refuses
            const char *why = (a->trees - 1) % 8 != 0 || a->trees > (1ull << 30) || a->twigs > (1ull << 30) ? "the tree pool is not 1 + 8k node words"
                                                                                                           : pools_walk(a->tree, a->trees, a->twigs, a->depth, &shallow);
            if (why) { set_error(std::string(who) + ": chunk a: " + why); return SVO_ERR_INVALID_ARG; }
        }
        if (depth > a->depth) { set_error(std::string(who) + ": the result is deeper than chunk a (that direction is the stamp into an empty chunk)"); return SVO_ERR_UNSUPPORTED; }
        if (!depth_ok(a->depth) || !depth_ok(depth)) { set_error(std::string(who) + ": a depth is outside [2, 16]"); return SVO_ERR_UNSUPPORTED; }
        if (shallow) { set_error(std::string(who) + ": " + SHALLOW_TWIG_WHY); return SVO_ERR_UNSUPPORTED; }
        Extract K{ a->tree, a->twig, ExtractPlace{ stamp_place(pl->offset, pl->orient), depth }, {}, {}, 0 };
        Extract::Entry root{ {}, 0, NONE };
        for (uint32_t j = 0; j < 8; ++j) {
            uint32_t left;
            root.nb[j] = extract_root_word(K.E, a->depth, j, a->tree[0], &left, [&](uint32_t w, uint32_t slot) { return a->tree[node_offset(w) + slot]; });
        }
        K.entries.push_back(root);
        const uint32_t x[3] = { 0, 0, 0 };
        K.visit(0, x, depth);
        std::vector<uint32_t> tree;
        std::vector<uint16_t> twig;
        K.emit(tree, twig);
        if (tree.size() > (1ull << 30) || twig.size() / TWIG_WORDS > (1ull << 30)) { set_error(std::string(who) + ": 2^30 nodes or bricks"); return SVO_ERR_UNSUPPORTED; }
        if (const int rc = chunk_desc_take(out, position, size, depth, tree, twig, who)) return rc;
        if (occupied_out) *occupied_out = K.occupied;
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

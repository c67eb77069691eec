// world.cpp — host half of the C ABI: world construction, validation, World::index helpers.
//
// Reference surface mirrored (see include/svo.h for the full map):
//   World::init          src/World.cpp:19-43     -> svo_world_generate
//   World::index(_float) src/World.cpp:276-293,323-332
//   Ocroot               src/Octree.h:56-76      -> svo_chunk_desc / ChunkPools
// The reference aborts on malformed input (assert / die(), src/Util.cpp:72-78); this library
// validates and returns an error code instead.
#include "world.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

namespace svo {

static thread_local std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }

// A chunk a world may hold: its own pre-checks, then the forward pass over the node words (chunk_pools.h: pools_walk).  A TWIG above
// level depth-2 is no refusal here: the kernels march a sparsely refined chunk.
int validate_chunk(const ChunkPools &c, std::string &why)
{
    const uint64_t n = c.tree.size();
    const char *bad = nullptr;
    if (n == 0) bad = "empty tree pool";
    else if (c.depth < TWIG_LEVELS || c.depth > 30) bad = "depth out of range [2,30]";
    else if ((n - 1) % 8 != 0) bad = "tree pool is not 1 + 8k nodes";
    else if (!(c.size > 0.0f) || !std::isfinite(c.size)) bad = "chunk size must be positive";
    else bad = pools_walk(c.tree.data(), n, c.twig_count(), c.depth, nullptr);
    if (!bad) return SVO_OK;
    why = bad;
    return SVO_ERR_MALFORMED_TREE;
}

// True when every corner of every possible node / brick cell of the chunk is an exactly
// representable float, i.e. the reference's incremental bmin arithmetic (src/Traverse.cpp:39-45)
// never rounds.  Then integer cell coordinates reproduce its comparisons exactly, which is what
// the stack kernel relies on.
bool chunk_is_exact(const ChunkPools &c, int chunksize)
{
    if (c.size != (float)chunksize) return false;
    int e = 0;
    if (std::frexp(c.size, &e) != 0.5f) return false;             // power-of-two edge
    const float voxel = std::ldexp(c.size, -(int)c.depth);
    if (!(voxel > 0.0f) || !std::isnormal(voxel)) return false;
    for (int a = 0; a < 3; ++a) {
        const float lo = c.position[a], hi = c.position[a] + c.size;
        if (!std::isfinite(lo) || !std::isfinite(hi)) return false;
        const double k = (double)lo / (double)voxel;
        if (k != std::floor(k)) return false;                      // position on the voxel lattice
        const double m = std::fmax(std::fabs((double)lo), std::fabs((double)hi)) / (double)voxel;
        if (m > 16777216.0) return false;                          // 2^24 lattice steps
    }
    return true;
}

void classify_world(svo_world &w)
{
    w.exact_geometry = true;
    w.max_levels = 0;
    for (const ChunkPools &c : w.chunks) {
        if (!chunk_is_exact(c, w.chunksize)) w.exact_geometry = false;
        w.max_levels = std::max(w.max_levels, (int)(c.depth - TWIG_LEVELS));
    }
}

} // namespace svo

using namespace svo;

extern "C" {

int svo_abi_version(void) { return SVO_ABI_VERSION; }
const char *svo_last_error(void) { return g_error.c_str(); }

int svo_world_generate(int w, int h, int d, int chunksize, const int ccm[3],
                       const svo_terrain_params *tp, svo_world **out)
{
    if (!out || !tp || w <= 0 || h <= 0 || d <= 0 || chunksize <= 0) { set_error("svo_world_generate: bad argument"); return SVO_ERR_INVALID_ARG; }
    if (tp->depth < TWIG_LEVELS || tp->depth > 20) { set_error("svo_world_generate: depth must be in [2,20]"); return SVO_ERR_INVALID_ARG; }
    if (tp->coarse_depth != 0 && (tp->coarse_depth < TWIG_LEVELS || tp->coarse_depth >= tp->depth)) { set_error("svo_world_generate: coarse_depth must be in [2, depth)"); return SVO_ERR_INVALID_ARG; }
    const uint32_t res = pyramid_resolution_or_default(tp->pyramid_resolution, tp->depth);
    if (res & (res - 1)) { set_error("svo_world_generate: pyramid_resolution must be a power of two"); return SVO_ERR_INVALID_ARG; }
    int status = SVO_OK;            // (SVO_OK_LITERAL_ONLY: generated on the device, resident there, but without the stack kernel's wide trees)
    try {
        svo_world *world = new svo_world();
        world->width = w; world->height = h; world->depth = d; world->chunksize = chunksize;
        for (int i = 0; i < 3; ++i) world->chunkcoordmin[i] = ccm ? ccm[i] : 0;
        TerrainParams p;
        p.depth = tp->depth; p.pyramid_resolution = tp->pyramid_resolution;
        p.amplitude = tp->amplitude; p.yshift = tp->yshift; p.seed = tp->seed;
        p.water = tp->water; p.water_level = tp->water_level; p.water_material = tp->water_material;
        p.threads = tp->threads;
        p.coarse_depth = tp->coarse_depth;
        for (int i = 0; i < 3; ++i) { p.refine_min[i] = tp->refine_min[i]; p.refine_max[i] = tp->refine_max[i]; }
        if (tp->build_device_plus1 > 0) {
            world->terrain = p;
            status = generate_world_resident(*world, tp->build_device_plus1 - 1);
            if (status < 0) { svo_world_destroy(world); return status; }
        } else {
            const TerrainWindow win = TerrainWindow::whole(w, h, d, chunksize, world->chunkcoordmin);
            std::vector<ChunkPools> grown;
            if (generate_window(win, p, grown) != 0) {
                delete world;
                set_error("svo_world_generate: out of host memory in a generator thread");
                return SVO_ERR_OUT_OF_MEMORY;
            }
            world->chunks.resize(grown.size());
            for (int k = 0; k < win.size(); ++k) world->chunks[(size_t)win.chunk(k).index] = std::move(grown[(size_t)k]);
        }
        world->terrain = p;
        world->has_terrain = true;
        classify_world(*world);
        *out = world;
        return status;
    } catch (const std::bad_alloc &) {
        set_error("svo_world_generate: out of host memory");
        return SVO_ERR_OUT_OF_MEMORY;
    }
}

int svo_world_create(const svo_chunk_desc *chunks, int n, int w, int h, int d, int chunksize,
                     const int ccm[3], svo_world **out)
{
    if (!out || !chunks || w <= 0 || h <= 0 || d <= 0 || chunksize <= 0 || n != w * h * d) {
        set_error("svo_world_create: bad argument (n must equal w*h*d)");
        return SVO_ERR_INVALID_ARG;
    }
    try {
        svo_world *world = new svo_world();
        world->width = w; world->height = h; world->depth = d; world->chunksize = chunksize;
        for (int i = 0; i < 3; ++i) world->chunkcoordmin[i] = ccm ? ccm[i] : 0;
        world->chunks.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            const svo_chunk_desc &s = chunks[i];
            ChunkPools &c = world->chunks[(size_t)i];
            if (!s.tree || s.trees == 0 || (s.twigs && !s.twig)) { delete world; set_error("svo_world_create: chunk has no pools"); return SVO_ERR_INVALID_ARG; }
            std::memcpy(c.position, s.position, sizeof c.position);
            c.size = s.size; c.depth = s.depth;
            c.tree.assign(s.tree, s.tree + s.trees);
            c.twig.assign(s.twig, s.twig + s.twigs * TWIG_WORDS);
            c.fit_capacity(c.tree.size(), c.twig_count());
            std::string why;
            const int rc = validate_chunk(c, why);
            if (rc != SVO_OK) { delete world; set_error("svo_world_create: chunk " + std::to_string(i) + ": " + why); return rc; }
        }
        classify_world(*world);
        *out = world;
        return SVO_OK;
    } catch (const std::bad_alloc &) {
        set_error("svo_world_create: out of host memory");
        return SVO_ERR_OUT_OF_MEMORY;
    }
}

// World::shift, src/World.cpp:334-378: slide the grid one chunk along one axis.  The whole plane of chunks entering the grid is
// generated (g_pyramid + g_chunk) before any of it is stored at its toroidal index - where the plane leaving on the opposite side
// used to live -, so a failure to generate it changes nothing; then chunkcoordmin moves.
int svo_world_shift(svo_world *w, const int offset[3])
{
    if (!w || !offset) return SVO_ERR_INVALID_ARG;
    if (!w->has_terrain) { set_error("svo_world_shift: world was not made by svo_world_generate (no terrain parameters)"); return SVO_ERR_UNSUPPORTED; }
    int axis = -1;
    for (int a = 0; a < 3; ++a)
        if (offset[a] != 0) { if (axis >= 0 || (offset[a] != 1 && offset[a] != -1)) { set_error("svo_world_shift: offset must be a unit axis step"); return SVO_ERR_INVALID_ARG; } axis = a; }
    if (axis < 0) { set_error("svo_world_shift: offset must be a unit axis step"); return SVO_ERR_INVALID_ARG; }
    const int sign = offset[axis];
    // an uploaded world: the entering plane is generated where the pools live (builder.hip), nothing visits the host
    if (w->device >= 0) return shift_world_resident(*w, axis, sign);
    const TerrainWindow plane = TerrainWindow::whole(w->width, w->height, w->depth, w->chunksize, w->chunkcoordmin).entering(axis, sign);
    try {
        std::vector<ChunkPools> grown;
        if (generate_window(plane, w->terrain, grown) != 0) { set_error("svo_world_shift: out of host memory in a generator thread"); return SVO_ERR_OUT_OF_MEMORY; }
        for (int k = 0; k < plane.size(); ++k) {
            const ChunkPools &c = grown[(size_t)k];
            svo_chunk_desc d;
            std::memcpy(d.position, c.position, sizeof d.position);
            d.size = c.size; d.depth = c.depth; d._pad = 0;
            d.tree = c.tree.data(); d.trees = c.tree.size();
            d.twig = c.twig.data(); d.twigs = c.twig_count();
            const int rc = svo_world_update(w, plane.chunk(k).index, &d, 0, d.trees, 0, d.twigs, 1);
            if (rc < 0) return rc;
        }
    } catch (const std::bad_alloc &) {
        set_error("svo_world_shift: out of host memory");
        return SVO_ERR_OUT_OF_MEMORY;
    }
    w->chunkcoordmin[axis] += sign;
    return SVO_OK;
}

int svo_world_edit_box(svo_world *w, int chunk, int op, const float lo[3], const float hi[3], uint16_t material)
{
    if (!w || !lo || !hi || chunk < 0 || chunk >= (int)w->chunks.size() || op < SVO_EDIT_BUILD || op > SVO_EDIT_REPLACE) { set_error("svo_world_edit_box: bad argument"); return SVO_ERR_INVALID_ARG; }
    for (int a = 0; a < 3; ++a) if (!(lo[a] <= hi[a])) { set_error("svo_world_edit_box: lo must not exceed hi (and neither may be NaN)"); return SVO_ERR_INVALID_ARG; }
    if (w->device < 0) { set_error("svo_world_edit_box: the world is not uploaded (edit the host pools and pass them to svo_world_update instead)"); return SVO_ERR_NOT_UPLOADED; }
    return edit_box_resident(*w, chunk, op, lo, hi, material);
}

int svo_world_edit_cube(svo_world *w, int op, const float bmin[3], float size, uint16_t material, int chunks_out[8], int *nchunks_out)
{   // modify(), src/Main.cpp:321-338
    bool ok = w && bmin && op >= SVO_EDIT_BUILD && op <= SVO_EDIT_REPLACE && size > 0.0f && std::isfinite(size);
    for (int a = 0; ok && a < 3; ++a) ok = std::isfinite(bmin[a]) && std::isfinite(bmin[a] + size);
    if (!ok) { set_error("svo_world_edit_cube: bad argument"); return SVO_ERR_INVALID_ARG; }
    if (w->device < 0) { set_error("svo_world_edit_cube: the world is not uploaded"); return SVO_ERR_NOT_UPLOADED; }
    const float cs = (float)w->chunksize;
    int list[8], n = 0;
    for (int i = 0; i < 8; ++i) {
        const float p[3] = { bmin[0] + ((i & 4) ? 1.0f : 0.0f) * size, bmin[1] + ((i & 2) ? 1.0f : 0.0f) * size, bmin[2] + ((i & 1) ? 1.0f : 0.0f) * size };
        int q[3];
        bool held = true;
        for (int a = 0; a < 3; ++a) {                       // World::index_float, src/World.cpp:323-332
            float f = p[a] / cs;
            if (f < 0.0f) f -= 1.0f;
            if (!(std::fabs(f) < 2147483648.0f)) { held = false; f = 0.0f; }     // beyond every grid an int can place: no chunk holds it
            q[a] = (int)f;
        }
        if (!held) continue;
        const int j = chunk_index(q[0], q[1], q[2], w->width, w->height, w->depth);
        const float *c = w->chunks[(size_t)j].position;
        for (int a = 0; a < 3; ++a) held = held && p[a] >= c[a] && c[a] + cs >= p[a];      // isInsideCube, src/Traverse.cpp:18-23
        if (!held) continue;
        bool seen = false;
        for (int k = 0; k < n; ++k) seen = seen || list[k] == j;
        if (!seen) list[n++] = j;
    }
    if (chunks_out) for (int k = 0; k < n; ++k) chunks_out[k] = list[k];
    if (nchunks_out) *nchunks_out = n;
    const float hi[3] = { bmin[0] + size, bmin[1] + size, bmin[2] + size };
    int status = SVO_OK;
    for (int k = 0; k < n; ++k) {
        const int rc = svo_world_edit_box(w, list[k], op, bmin, hi, material);
        if (rc < 0) return rc;
        if (rc > status) status = rc;
    }
    return status;
}

// svo_world_edit_ball's arguments, settled before anything changes (shared with svo_world_edit_ball_all)
static bool ball_args_ok(const svo_world *w, int op, const float centre[3], float radius)
{
    bool ok = w && centre && op >= SVO_EDIT_BUILD && op <= SVO_EDIT_REPLACE && radius > 0.0f && std::isfinite(radius);
    for (int a = 0; ok && a < 3; ++a) ok = std::isfinite(centre[a]);
    return ok;
}

int svo_world_edit_ball(svo_world *w, int chunk, int op, const float centre[3], float radius, uint16_t material)
{
    if (!ball_args_ok(w, op, centre, radius) || chunk < 0 || chunk >= (int)w->chunks.size()) { set_error("svo_world_edit_ball: bad argument"); return SVO_ERR_INVALID_ARG; }
    if (w->device < 0) { set_error("svo_world_edit_ball: the world is not uploaded"); return SVO_ERR_NOT_UPLOADED; }
    return edit_ball_resident(*w, chunk, op, centre, radius, material);
}

int svo_world_edit_ball_all(svo_world *w, int op, const float centre[3], float radius, uint16_t material, int *chunks_out, int chunks_cap, int *nchunks_out)
{
    if (!ball_args_ok(w, op, centre, radius)) { set_error("svo_world_edit_ball_all: bad argument"); return SVO_ERR_INVALID_ARG; }
    // the ball's touch (builder.hip: BallRegion) on every chunk's box [position, position + chunksize], in float
    const float cs = (float)w->chunksize, r2 = radius * radius;
    std::vector<int> list;
    try { list.reserve(w->chunks.size()); }
    catch (const std::bad_alloc &) { set_error("svo_world_edit_ball_all: out of host memory"); return SVO_ERR_OUT_OF_MEMORY; }
    for (int j = 0; j < (int)w->chunks.size(); ++j) {
        const float *lo = w->chunks[(size_t)j].position;
        float d[3];
        for (int a = 0; a < 3; ++a) {
            const float hi = lo[a] + cs;
            d[a] = lo[a] - centre[a];
            if (!(d[a] > 0.0f)) { d[a] = centre[a] - hi; if (!(d[a] > 0.0f)) d[a] = 0.0f; }
        }
        if (d[0] * d[0] + d[1] * d[1] + d[2] * d[2] <= r2) list.push_back(j);
    }
    const int n = (int)list.size();
    if (nchunks_out) *nchunks_out = n;
    if (chunks_out && n > chunks_cap) { set_error("svo_world_edit_ball_all: the ball touches more chunks than chunks_cap holds"); return SVO_ERR_INVALID_ARG; }
    if (w->device < 0) { set_error("svo_world_edit_ball_all: the world is not uploaded"); return SVO_ERR_NOT_UPLOADED; }
    if (chunks_out) for (int k = 0; k < n; ++k) chunks_out[k] = list[(size_t)k];
    int status = SVO_OK;
    for (int k = 0; k < n; ++k) {
        const int rc = edit_ball_resident(*w, list[(size_t)k], op, centre, radius, material);
        if (rc < 0) return rc;
        if (rc > status) status = rc;
    }
    return status;
}

int svo_world_info_get(const svo_world *w, svo_world_info *o)
{
    if (!w || !o) return SVO_ERR_INVALID_ARG;
    std::memset(o, 0, sizeof *o);
    o->width = w->width; o->height = w->height; o->depth = w->depth; o->chunksize = w->chunksize;
    for (int i = 0; i < 3; ++i) o->chunkcoordmin[i] = w->chunkcoordmin[i];
    o->uploaded_device = w->device;
    for (const ChunkPools &c : w->chunks) { o->total_trees += c.tree_count(); o->total_twigs += c.twig_count(); }
    o->tree_pool_bytes = w->tree_pool_cap * sizeof(uint32_t);
    o->twig_pool_bytes = w->twig_pool_cap * TWIG_WORDS * sizeof(uint16_t);
    o->mask_pool_bytes = w->twig_pool_cap * (sizeof(uint64_t) + sizeof(uint16_t));     // occupancy masks + one material per brick
    o->max_chunk_depth = w->max_levels + (int)TWIG_LEVELS;
    o->exact_geometry = w->exact_geometry ? 1 : 0;
    o->wide_pool_bytes = w->wide_pool_cap * (64 + 9) * sizeof(uint32_t);               // 64 entries + 9 reference block indices per wide node
    o->wide_nodes = w->wide_nodes_used;
    return SVO_OK;
}

int svo_world_chunk(const svo_world *w, int i, svo_chunk_desc *o)
{
    if (!w || !o || i < 0 || i >= (int)w->chunks.size()) return SVO_ERR_INVALID_ARG;
    if (w->chunks[(size_t)i].twigs_on_device || w->chunks[(size_t)i].trees_on_device) {   // built on the device: the host copy is made on first request
        const int rc = fetch_pools(*const_cast<svo_world *>(w), i);
        if (rc != SVO_OK) return rc;
    }
    const ChunkPools &c = w->chunks[(size_t)i];
    std::memcpy(o->position, c.position, sizeof o->position);
    o->size = c.size; o->depth = c.depth; o->_pad = 0;
    o->tree = c.tree.data(); o->trees = c.tree.size();
    o->twig = c.twig.data(); o->twigs = c.twig_count();
    return SVO_OK;
}

void svo_world_destroy(svo_world *w)
{
    if (!w) return;
    release_device(*w);
    delete w;
}

// ---- Ocroot::write / read, src/Octree.cpp:178-201 ----------------------------------------------
namespace {
#pragma pack(push, 1)
struct ChunkFileHeader {            // == the first 64 bytes of Ocroot (TREE_STRUCT_SIZE, src/Octree.cpp:178)
    float    position[3];           // @0
    float    size;                  // @12
    uint32_t depth;                 // @16
    uint32_t pad0;                  // @20
    uint64_t trees, twigs;          // @24, @32
    uint64_t treestoragesize, twigstoragesize;   // @40, @48
    uint8_t  modified;              // @56
    uint8_t  pad1[7];
};
#pragma pack(pop)
static_assert(sizeof(ChunkFileHeader) == 64, "Ocroot file header is 64 bytes");
}

int svo_chunk_write(const char *path, const svo_chunk_desc *c, uint64_t treestoragesize, uint64_t twigstoragesize)
{
    if (!path || !c || !c->tree || c->trees == 0 || (c->twigs && !c->twig)) { set_error("svo_chunk_write: bad argument"); return SVO_ERR_INVALID_ARG; }
    ChunkFileHeader h;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.position, c->position, sizeof h.position);
    h.size = c->size; h.depth = c->depth;
    h.trees = c->trees; h.twigs = c->twigs;
    h.treestoragesize = treestoragesize > c->trees ? treestoragesize : c->trees;
    h.twigstoragesize = twigstoragesize > c->twigs ? twigstoragesize : c->twigs;
    FILE *fp = std::fopen(path, "wb");
    if (!fp) { set_error(std::string("svo_chunk_write: cannot open ") + path); return SVO_ERR_INVALID_ARG; }
    bool ok = std::fwrite(&h, 1, sizeof h, fp) == sizeof h &&
              std::fwrite(c->tree, sizeof(uint32_t), c->trees, fp) == c->trees &&
              (c->twigs == 0 || std::fwrite(c->twig, TWIG_WORDS * sizeof(uint16_t), c->twigs, fp) == c->twigs);
    ok = (std::fclose(fp) == 0) && ok;
    if (!ok) { set_error("svo_chunk_write: short write"); return SVO_ERR_INVALID_ARG; }
    return SVO_OK;
}

int svo_chunk_read(const char *path, svo_chunk_desc *out, uint64_t *treestoragesize, uint64_t *twigstoragesize)
{
    if (!path || !out) { set_error("svo_chunk_read: bad argument"); return SVO_ERR_INVALID_ARG; }
    std::memset(out, 0, sizeof *out);
    FILE *fp = std::fopen(path, "rb");
    if (!fp) { set_error(std::string("svo_chunk_read: cannot open ") + path); return SVO_ERR_INVALID_ARG; }
    ChunkFileHeader h;
    int rc = SVO_OK;
    uint32_t *tree = nullptr;
    uint16_t *twig = nullptr;
    do {
        if (std::fread(&h, 1, sizeof h, fp) != sizeof h) { set_error("svo_chunk_read: truncated header"); rc = SVO_ERR_MALFORMED_TREE; break; }
        std::fseek(fp, 0, SEEK_END);
        const long long len = std::ftell(fp);
        std::fseek(fp, (long)sizeof h, SEEK_SET);
        // the reference trusts the header (src/Octree.cpp:189-201); here sizes are checked against the file
        if (h.trees == 0 || h.trees > (1ull << 31) || h.twigs > (1ull << 31) ||
            (unsigned long long)len != sizeof h + h.trees * 4ull + h.twigs * 128ull) { set_error("svo_chunk_read: header does not match file length"); rc = SVO_ERR_MALFORMED_TREE; break; }
        tree = (uint32_t *)std::malloc(h.trees * sizeof(uint32_t));
        twig = (uint16_t *)std::malloc((h.twigs ? h.twigs : 1) * TWIG_WORDS * sizeof(uint16_t));
        if (!tree || !twig) { set_error("svo_chunk_read: out of memory"); rc = SVO_ERR_OUT_OF_MEMORY; break; }
        if (std::fread(tree, sizeof(uint32_t), h.trees, fp) != h.trees ||
            (h.twigs && std::fread(twig, TWIG_WORDS * sizeof(uint16_t), h.twigs, fp) != h.twigs)) { set_error("svo_chunk_read: short read"); rc = SVO_ERR_MALFORMED_TREE; break; }
    } while (0);
    std::fclose(fp);
    if (rc != SVO_OK) { std::free(tree); std::free(twig); return rc; }
    std::memcpy(out->position, h.position, sizeof out->position);
    out->size = h.size; out->depth = h.depth;
    out->tree = tree; out->trees = h.trees;
    out->twig = twig; out->twigs = h.twigs;
    if (treestoragesize) *treestoragesize = h.treestoragesize;
    if (twigstoragesize) *twigstoragesize = h.twigstoragesize;
    return SVO_OK;
}

void svo_chunk_free(svo_chunk_desc *c)
{
    if (!c) return;
    std::free(const_cast<uint32_t *>(c->tree));
    std::free(const_cast<uint16_t *>(c->twig));
    c->tree = nullptr; c->twig = nullptr; c->trees = c->twigs = 0;
}

int svo_world_index_float(const svo_world *w, const float p[3], int q[3])
{   // src/World.cpp:323-332
    if (!w || !p || !q) return SVO_ERR_INVALID_ARG;
    const float cs = (float)w->chunksize;
    for (int i = 0; i < 3; ++i) {
        float f = p[i] / cs;
        if (f < 0.0f) f -= 1.0f;
        q[i] = (int)f;
    }
    return SVO_OK;
}

int svo_world_index(const svo_world *w, int x, int y, int z)
{   // src/World.cpp:288-293
    if (!w) return SVO_ERR_INVALID_ARG;
    return chunk_index(x, y, z, w->width, w->height, w->depth);
}

} // extern "C"

"""octree-raymarcher_amd — thin ctypes harness over libsvo_amd.so (the C ABI in include/svo.h).

The product is the shared library; this module only exists so that tests/ and bench.py can drive
it.  It mirrors the reference's `World` / `Traverse` surface (src/World.h:44-68, src/Traverse.h:27-30):

    World.generate(w, h, d, chunksize, ...)   <- World::init            src/World.cpp:19-43
    World.upload(device)                      <- World::load_gpu        src/World.cpp:57-94
    World.draw(camera, ...)                   <- World::draw            src/World.cpp:205-266
    World.chunkmarch(origins, dirs)           <- chunkmarch             src/Traverse.cpp:127-171
    World.draw_translucent(camera, m)         <- ParallaxAlpha's march past water   shaders/ParallaxAlpha.Fragment.glsl:141-199,276-335
    World.trace_local_shadows(camera, ...)    <- (none: the reference's three lights share the directional light's shadow term)
    World.trace_lights, shade_lights, Light   <- (none: the reference has three lights)    up to 32 point lights with a reach, one compacted ray list
    World.trace_instances, trace_instance_shadows, Instance   <- (none: the reference's moving object is a rasterised mesh, src/Worm.cpp)   up to 32 placements of a model world
    World.shadowmap_fit / shadowmap_render, shadowmap_apply   <- OrthoCamera, World::draw_shadowmap, computeShadow   src/World.cpp:162-203, shaders/World.Fragment.glsl:140-155
    World.index / index_float                 <- World::index(_float)   src/World.cpp:288-293,323-332
    World.locate / locate_points              <- traverse               src/Traverse.cpp:34-48 (the voxel under each point)
    World.hit_voxels / hit_boxes              <- hit.bmin / hit.size of fragment main   shaders/World.Fragment.glsl:168-172
    hit_uv, shade_textured, Atlas             <- leafUV, texture(Diffuse / Specular, uv)   shaders/World.Fragment.glsl:5-15,178-182
    shade_sky, Sky                            <- Skybox::draw behind the world             src/Skybox.cpp, shaders/Skybox.*.glsl
    frame_rgba8                               <- the RGBA8 colour attachment               src/GBuffer.cpp, shaders/GBuffer.Fragment.glsl:10
    cursor_place, shade_boxes, Box            <- computeTarget, ImaginaryCube / Light::draw   src/Main.cpp:314-319, src/ImaginaryCube.cpp:59-87
    World.edit_cube                           <- modify()                                  src/Main.cpp:321-368
    World.edit_ball / edit_ball_all           <- (none: the reference edits cubes only)    destroyCube / buildCube over a closed ball
    World.hit_ao / ao_image, shade_ao         <- (none: the reference has no ambient occlusion)   the eight lattice cells around each hit's face
    World.trace_reflections / reflect_image, shade_reflections, Mirror   <- (none: the reference has no reflections)   one mirror ray per hit, off its voxel's face
    chunk_from_mesh, World.chunk_from_mesh   <- (none)   the tree of a mesh's shell without the dense grid, to depth 16
    chunk_fill_enclosed, World.chunk_fill_enclosed   <- (none)   the cells a chunk's voxels enclose, filled on the tree, to depth 16
    chunk_combine, World.chunk_combine   <- (none)   two chunks of one depth combined cell by cell on their trees (COMBINE_*), to depth 16
    chunk_stamp, World.chunk_stamp, Placement   <- (none)   a chunk placed into another at a cell offset, in one of 48 orientations, through a COMBINE_* rule
    chunk_extract, World.chunk_extract          <- (none)   the stamp's inverse: a cube of cells copied out of a chunk at a cell offset, in one of 48 orientations
    grid_add_mesh / grid_fill_enclosed, device_grid_add_mesh / device_grid_fill_enclosed, Mesh   <- (none: the reference rasterises its one mesh with GL)   a triangle mesh into a dense grid, its shell filled

There is NO CPU fallback: if libsvo_amd.so is missing the import raises, and every device call
raises SvoError when HIP reports no device.

Import with importlib.import_module("octree-raymarcher_amd") (the hyphen is the project's name).
If torch is used in the same process, import torch BEFORE this module so that both share one HIP
runtime (both resolve the soname libamdhip64.so.7).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Sequence

import numpy as np

from . import partition  # noqa: F401  (host-side image partition helpers)

_HERE = os.path.dirname(os.path.abspath(__file__))
# SVO_AMD_LIB lets kernel A/B experiments point at an alternative build of the same library.
LIB_PATH = os.environ.get("SVO_AMD_LIB") or os.path.join(_HERE, "libsvo_amd.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C {_HERE}` (or __graft_entry__.build()). "
        "There is no CPU fallback for the SVO march.")

lib = C.CDLL(LIB_PATH)

# ---- enums / constants (include/svo.h) -----------------------------------------------------
SVO_OK = 0
OK_LITERAL_ONLY = 1     # svo_world_update / edit_box / compact / coarsen / shift: applied, but the stack kernel's wide trees could not be rebuilt
ERR_NAMES = {0: "SVO_OK", -1: "SVO_ERR_INVALID_ARG", -2: "SVO_ERR_NO_DEVICE", -3: "SVO_ERR_OUT_OF_MEMORY",
             -4: "SVO_ERR_MALFORMED_TREE", -5: "SVO_ERR_NOT_UPLOADED", -6: "SVO_ERR_UNSUPPORTED", -7: "SVO_ERR_HIP"}
EMPTY, LEAF, BRANCH, TWIG = 0, 1, 2, 3
KERNEL_AUTO, KERNEL_LITERAL, KERNEL_STACK = 0, 1, 2
EDIT_BUILD, EDIT_DESTROY, EDIT_REPLACE = 0, 1, 2     # svo_world_edit_box
COMBINE_MAX, COMBINE_UNDER, COMBINE_OVER, COMBINE_SUBTRACT, COMBINE_INTERSECT = 0, 1, 2, 3, 4     # svo_chunk_combine / svo_world_chunk_combine
COMBINE_MIN_DEPTH, COMBINE_MAX_DEPTH = 2, 16
STAMP_MIN_DEPTH, STAMP_MAX_DEPTH, STAMP_ORIENTS, STAMP_OFFSET_LIMIT = 2, 16, 48, 65536      # svo_chunk_stamp / svo_world_chunk_stamp
EXTRACT_MIN_DEPTH, EXTRACT_MAX_DEPTH = 2, 16                # svo_chunk_extract / svo_world_chunk_extract
# the 24 proper orientations (rotations) among orient = perm * 8 + flips: parity(perm) * (-1)^popcount(flips) = +1; perms 1, 2, 5 are odd
ORIENT_ROTATIONS = tuple(o for o in range(48) if ((o >> 3 in (1, 2, 5)) + bin(o & 7).count("1")) % 2 == 0)
HIT_FLAG, SHADOW_TRACED, SHADOWED, FACE_NORMAL, SEE_THROUGH, ERR_FLAG = 1, 2, 4, 8, 16, 1 << 15
LOCAL_SHADOWS, SHADOWED_POINT, SHADOWED_SPOT = 1 << 5, 1 << 6, 1 << 7     # svo_trace_local_shadows
NORMAL_CUBE, NORMAL_FACE = 0, 1
SHADOW_NO_CLEARANCE = 2          # bit of TraceParams.shadow: shadow rays as ever, World.prepare_light's bits ignored
SHADOW_NO_BRICK_CLEARANCE = 4    # bit of TraceParams.shadow: the bits are used, the per-brick flags that settle a lit shadow ray at its hit are not
SHADOW_NO_DARK_BIRTH = 8         # bit of TraceParams.shadow: a shadow ray born in an occupied cell of the hit brick is marched, not settled at the hit
SEMANTICS_CPU, SEMANTICS_GLSL = 0, 1
CELL_NONE = 0xFF
SKY_LINEAR, SKY_NEAREST = 0, 1                           # svo_sky.filter
BOX_SOLID, BOX_CURSOR, BOX_HIDDEN = 0, 1, 1 << 8         # svo_box.style
MAX_BOXES = 64                                           # SVO_MAX_BOXES
MAX_LIGHTS = 32                                          # SVO_MAX_LIGHTS
MAX_INSTANCES = 32                                       # SVO_MAX_INSTANCES
BOX_DTYPE = np.dtype([("bmin", "<f4", (3,)), ("size", "<f4"), ("color", "<f4", (3,)), ("alpha", "<f4"), ("style", "<u4"), ("_pad", "<u4", (3,))])
assert BOX_DTYPE.itemsize == 48

HIT_DTYPE = np.dtype([("t", "<f4"), ("normal", "<f4", (3,)), ("material", "<u2"), ("flags", "<u2"),
                      ("chunk", "<u4"), ("node", "<u4"), ("cell", "<u4")])
assert HIT_DTYPE.itemsize == 32
LOCATE_INSIDE, LOCATE_SOLID = 1, 2                       # svo_voxel.flags (svo_world_locate)
VOXEL_DTYPE = np.dtype([("bmin", "<f4", (3,)), ("size", "<f4"), ("material", "<u2"), ("flags", "<u2"),
                        ("chunk", "<u4"), ("node", "<u4"), ("cell", "<u4")])
assert VOXEL_DTYPE.itemsize == 32


class SvoError(RuntimeError):
    def __init__(self, code: int, where: str):
        self.code = code
        msg = lib.svo_last_error().decode(errors="replace")
        super().__init__(f"{where}: {ERR_NAMES.get(code, code)} ({msg})")


class ChunkDesc(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("size", C.c_float), ("depth", C.c_uint32), ("_pad", C.c_uint32),
                ("tree", C.POINTER(C.c_uint32)), ("trees", C.c_uint64),
                ("twig", C.POINTER(C.c_uint16)), ("twigs", C.c_uint64)]


class Placement(C.Structure):
    """svo_placement: A's cell that B's cube starts at (each offset in [-65536, 65536]) and the orientation 0 .. 47."""
    _fields_ = [("offset", C.c_int32 * 3), ("orient", C.c_uint32)]

    def __init__(self, offset=(0, 0, 0), orient=0):
        super().__init__((C.c_int32 * 3)(*[int(x) for x in offset]), int(orient))


class TerrainParams(C.Structure):
    _fields_ = [("depth", C.c_uint32), ("pyramid_resolution", C.c_uint32), ("amplitude", C.c_float),
                ("yshift", C.c_float), ("seed", C.c_int32), ("water", C.c_int32), ("water_level", C.c_float),
                ("water_material", C.c_uint32), ("threads", C.c_int32), ("coarse_depth", C.c_uint32),
                ("refine_min", C.c_float * 3), ("refine_max", C.c_float * 3), ("build_device_plus1", C.c_int32)]


class Camera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("forward", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3),
                ("tan_half_x", C.c_float), ("tan_half_y", C.c_float), ("width", C.c_int32), ("height", C.c_int32)]


class TraceParams(C.Structure):
    _fields_ = [("eps", C.c_float), ("max_chunk_steps", C.c_int32), ("max_tree_steps", C.c_int32),
                ("max_twig_steps", C.c_int32), ("shadow", C.c_int32), ("light_dir", C.c_float * 3),
                ("kernel", C.c_int32), ("tiles_per_wave", C.c_int32), ("counters_dev", C.c_void_p),
                ("normal_mode", C.c_int32), ("launches_in_flight", C.c_int32),
                ("tile_cost_dev", C.c_void_p), ("tile_order_dev", C.c_void_p), ("semantics", C.c_int32), ("see_through", C.c_uint32)]


class Material(C.Structure):
    _fields_ = [("ambient", C.c_float * 3), ("diffuse", C.c_float * 3), ("specular", C.c_float * 3), ("shininess", C.c_float)]


class _PointLight(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("ambient", C.c_float * 3), ("diffuse", C.c_float * 3), ("specular", C.c_float * 3),
                ("constant", C.c_float), ("linear", C.c_float), ("quadratic", C.c_float)]


class _DirectionalLight(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("direction", C.c_float * 3), ("ambient", C.c_float * 3), ("diffuse", C.c_float * 3),
                ("specular", C.c_float * 3)]


class _Spotlight(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("direction", C.c_float * 3), ("ambient", C.c_float * 3), ("diffuse", C.c_float * 3),
                ("specular", C.c_float * 3), ("cos_phi", C.c_float), ("cos_gamma", C.c_float), ("constant", C.c_float),
                ("linear", C.c_float), ("quadratic", C.c_float)]


class ShadeParams(C.Structure):
    _fields_ = [("point", _PointLight), ("directional", _DirectionalLight), ("spot", _Spotlight), ("materials", Material * 8),
                ("eps", C.c_float), ("gamma", C.c_float), ("near_plane", C.c_float), ("far_plane", C.c_float)]


class Atlas(C.Structure):
    """svo_atlas: RGB8 images on the device, rows tightly packed, row 0 at v = 0; specular_dev None = the diffuse image."""
    _fields_ = [("diffuse_dev", C.c_void_p), ("specular_dev", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


class ShadowMap(C.Structure):
    """svo_shadowmap: the directional light's orthographic view and its depth image (width*height float on the device, row 0 at +up)."""
    _fields_ = [("origin", C.c_float * 3), ("direction", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3),
                ("half_width", C.c_float), ("half_height", C.c_float), ("width", C.c_int32), ("height", C.c_int32), ("depth_dev", C.c_void_p)]


class Sky(C.Structure):
    """svo_sky: six size x size RGB8 cube-map faces on the device (+X, -X, +Y, -Y, +Z, -Z; rows tightly packed, row 0 at t = 0).
    Sky(face_ptrs, size, filter): face_ptrs are six device pointers (None = NULL)."""
    _fields_ = [("faces_dev", C.c_void_p * 6), ("size", C.c_int32), ("filter", C.c_int32)]

    def __init__(self, faces=(None,) * 6, size: int = 0, filter: int = SKY_LINEAR):
        super().__init__()
        for i, ptr in enumerate(faces):
            self.faces_dev[i] = ptr
        self.size, self.filter = int(size), int(filter)


class Mirror(C.Structure):
    """svo_mirror: what svo_shade_reflections blends with.  Mirror(material, f0, fresnel, background, sky): sky a Sky or None; the
    struct keeps a reference to it."""
    _fields_ = [("material", C.c_uint32), ("f0", C.c_float), ("fresnel", C.c_int32), ("background", C.c_float * 3), ("sky", C.POINTER(Sky))]

    def __init__(self, material: int = 0, f0: float = 0.02, fresnel: bool = True, background=(0.0, 0.0, 0.0), sky: Optional[Sky] = None):
        super().__init__()
        self.material, self.f0, self.fresnel = int(material), float(f0), int(bool(fresnel))
        self.background[:] = [float(c) for c in background]
        self._sky = sky                                      # (the pointer below does not keep it alive)
        if sky is not None:
            self.sky = C.pointer(sky)


class Light(C.Structure):
    """svo_light: one point light of a light list (64 bytes).  Light(position, reach, ambient, diffuse, specular, attenuation)."""
    _fields_ = [("position", C.c_float * 3), ("reach", C.c_float), ("ambient", C.c_float * 3), ("constant", C.c_float),
                ("diffuse", C.c_float * 3), ("linear", C.c_float), ("specular", C.c_float * 3), ("quadratic", C.c_float)]

    def __init__(self, position=(0.0, 0.0, 0.0), reach: float = 0.0, ambient=(0.0, 0.0, 0.0), diffuse=(0.0, 0.0, 0.0), specular=(0.0, 0.0, 0.0),
                 attenuation=(1.0, 0.0, 0.0)):
        super().__init__()
        self.position[:], self.reach = [float(c) for c in position], float(reach)
        self.ambient[:], self.diffuse[:], self.specular[:] = ([float(c) for c in v] for v in (ambient, diffuse, specular))
        self.constant, self.linear, self.quadratic = (float(c) for c in attenuation)


class Instance(C.Structure):
    """svo_instance: one placement of a model world (64 bytes): x_world = pos + scale * (R x_model).  Instance(rot, pos, scale), rot a
    3x3 (or 9 floats, row-major), model -> world."""
    _fields_ = [("rot", C.c_float * 9), ("pos", C.c_float * 3), ("scale", C.c_float), ("_pad", C.c_uint32 * 3)]

    def __init__(self, rot=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), pos=(0.0, 0.0, 0.0), scale: float = 1.0):
        super().__init__()
        self.rot[:] = [float(c) for c in np.asarray(rot, np.float64).reshape(9)]
        self.pos[:], self.scale = [float(c) for c in pos], float(scale)


class Mesh(C.Structure):
    """svo_mesh: a triangle mesh and the frame of the grid it is voxelised into (56 bytes).  Mesh(vertices, indices, materials, nvertices,
    ntriangles, origin, cell, material): the three arrays as addresses (host for svo_grid_add_mesh, device for svo_device_grid_add_mesh;
    None = NULL); the struct does not keep them alive."""
    _fields_ = [("vertices", C.c_void_p), ("indices", C.c_void_p), ("materials", C.c_void_p), ("nvertices", C.c_uint32), ("ntriangles", C.c_uint32),
                ("origin", C.c_float * 3), ("cell", C.c_float), ("material", C.c_uint16), ("_pad", C.c_uint16 * 3)]

    def __init__(self, vertices=None, indices=None, materials=None, nvertices: int = 0, ntriangles: int = 0, origin=(0.0, 0.0, 0.0), cell: float = 1.0,
                 material: int = 1):
        super().__init__()
        self.vertices, self.indices, self.materials = vertices, indices, materials
        self.nvertices, self.ntriangles = int(nvertices), int(ntriangles)
        self.origin[:], self.cell, self.material = [float(c) for c in origin], float(cell), int(material)


class Box(C.Structure):
    """svo_box: one overlay cube of svo_shade_boxes (48 bytes; BOX_DTYPE is its numpy twin)."""
    _fields_ = [("bmin", C.c_float * 3), ("size", C.c_float), ("color", C.c_float * 3), ("alpha", C.c_float), ("style", C.c_uint32),
                ("_pad", C.c_uint32 * 3)]


class WorldInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("depth", C.c_int32), ("chunksize", C.c_int32),
                ("chunkcoordmin", C.c_int32 * 3), ("uploaded_device", C.c_int32),
                ("total_trees", C.c_uint64), ("total_twigs", C.c_uint64),
                ("tree_pool_bytes", C.c_uint64), ("twig_pool_bytes", C.c_uint64), ("mask_pool_bytes", C.c_uint64),
                ("max_chunk_depth", C.c_int32), ("exact_geometry", C.c_int32),
                ("wide_pool_bytes", C.c_uint64), ("wide_nodes", C.c_uint64)]


# every symbol include/svo.h declares (tests check that the library exports exactly these)
MAX_FRAMES = 16                     # SVO_MAX_FRAMES

ABI_SYMBOLS = [
    "svo_world_generate", "svo_world_create", "svo_world_info_get", "svo_world_chunk", "svo_world_destroy",
    "svo_world_index_float", "svo_world_index", "svo_world_locate", "svo_hit_voxels", "svo_hit_uv", "svo_shade_textured", "svo_world_upload", "svo_world_update",
    "svo_chunk_from_grid", "svo_world_chunk_from_grid", "svo_world_chunk_to_grid",
    "svo_grid_add_mesh", "svo_device_grid_add_mesh", "svo_grid_fill_enclosed", "svo_device_grid_fill_enclosed",
    "svo_chunk_from_mesh", "svo_world_chunk_from_mesh", "svo_chunk_fill_enclosed", "svo_world_chunk_fill_enclosed",
    "svo_chunk_combine", "svo_world_chunk_combine", "svo_chunk_stamp", "svo_world_chunk_stamp", "svo_chunk_extract", "svo_world_chunk_extract",
    "svo_chunk_write", "svo_chunk_read", "svo_chunk_free", "svo_world_shift", "svo_world_edit_box", "svo_world_edit_cube", "svo_world_edit_ball", "svo_world_edit_ball_all", "svo_world_compact", "svo_world_coarsen", "svo_shade", "svo_shade_packed", "svo_shade_translucent", "svo_shade_sky", "svo_frame_rgba8", "svo_cursor_place", "svo_shade_boxes", "svo_shade_defaults", "svo_gbuffer_pack", "svo_gbuffer_unpack",
    "svo_tile_order", "svo_trace", "svo_trace_rows", "svo_trace_frames", "svo_trace_rows_frames", "svo_trace_rays", "svo_trace_segments", "svo_trace_translucent", "svo_trace_local_shadows", "svo_trace_last_ray_count",
    "svo_shadowmap_fit", "svo_shadowmap_render", "svo_shadowmap_apply", "svo_hit_ao", "svo_shade_ao",
    "svo_trace_reflections", "svo_shade_reflections", "svo_trace_lights", "svo_shade_lights", "svo_trace_instances", "svo_trace_instance_shadows", "svo_world_prepare_light", "svo_world_prepared_light", "svo_world_prepared_bricks",
    "svo_device_count", "svo_device_alloc", "svo_device_free", "svo_device_cache_trim", "svo_memcpy_h2d", "svo_memcpy_d2h",
    "svo_stream_synchronize", "svo_last_error", "svo_abi_version",
]

_P = C.c_void_p
lib.svo_last_error.restype = C.c_char_p
lib.svo_abi_version.restype = C.c_int
lib.svo_world_edit_box.argtypes = [_P, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint16]
lib.svo_world_edit_cube.argtypes = [_P, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_uint16, C.POINTER(C.c_int), C.POINTER(C.c_int)]
lib.svo_world_edit_ball.argtypes = [_P, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_uint16]
lib.svo_world_edit_ball_all.argtypes = [_P, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_uint16, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
lib.svo_world_compact.argtypes = [_P, C.c_int]
lib.svo_world_compact.restype = C.c_int
lib.svo_world_coarsen.argtypes = [_P, C.c_int]
lib.svo_world_coarsen.restype = C.c_int
lib.svo_world_generate.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(TerrainParams), C.POINTER(_P)]
lib.svo_world_create.argtypes = [C.POINTER(ChunkDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(_P)]
lib.svo_world_info_get.argtypes = [_P, C.POINTER(WorldInfo)]
lib.svo_world_chunk.argtypes = [_P, C.c_int, C.POINTER(ChunkDesc)]
lib.svo_world_destroy.argtypes = [_P]
lib.svo_world_destroy.restype = None
lib.svo_world_index_float.argtypes = [_P, C.POINTER(C.c_float), C.POINTER(C.c_int)]
lib.svo_world_index.argtypes = [_P, C.c_int, C.c_int, C.c_int]
lib.svo_chunk_write.argtypes = [C.c_char_p, C.POINTER(ChunkDesc), C.c_uint64, C.c_uint64]
lib.svo_chunk_read.argtypes = [C.c_char_p, C.POINTER(ChunkDesc), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
lib.svo_chunk_free.argtypes = [C.POINTER(ChunkDesc)]
lib.svo_chunk_free.restype = None
lib.svo_world_shift.argtypes = [_P, C.POINTER(C.c_int)]
lib.svo_chunk_from_grid.argtypes = [_P, C.c_uint32, C.POINTER(C.c_float), C.c_float, C.POINTER(ChunkDesc)]
lib.svo_world_chunk_from_grid.argtypes = [_P, C.c_int, _P, C.c_uint32]
lib.svo_world_chunk_to_grid.argtypes = [_P, C.c_int, C.c_uint32, _P, _P]
lib.svo_grid_add_mesh.argtypes = [C.POINTER(Mesh), C.c_uint32, _P]
lib.svo_device_grid_add_mesh.argtypes = [C.POINTER(Mesh), C.c_uint32, _P, _P]
lib.svo_grid_fill_enclosed.argtypes = [_P, C.c_uint32, C.c_uint16, C.POINTER(C.c_uint64)]
lib.svo_device_grid_fill_enclosed.argtypes = [_P, C.c_uint32, C.c_uint16, C.POINTER(C.c_uint64), _P]
lib.svo_chunk_from_mesh.argtypes = [C.POINTER(Mesh), C.c_int, C.c_uint32, C.POINTER(C.c_float), C.c_float, C.POINTER(ChunkDesc)]
lib.svo_world_chunk_from_mesh.argtypes = [_P, C.c_int, C.POINTER(Mesh), C.c_int, C.c_uint32]
lib.svo_chunk_fill_enclosed.argtypes = [C.POINTER(ChunkDesc), C.c_uint16, C.POINTER(ChunkDesc), C.POINTER(C.c_uint64)]
lib.svo_world_chunk_fill_enclosed.argtypes = [_P, C.c_int, C.c_uint16, C.POINTER(C.c_uint64)]
lib.svo_chunk_combine.argtypes = [C.POINTER(ChunkDesc), C.POINTER(ChunkDesc), C.c_int, C.POINTER(ChunkDesc), C.POINTER(C.c_uint64)]
lib.svo_world_chunk_combine.argtypes = [_P, C.c_int, _P, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
lib.svo_chunk_stamp.argtypes = [C.POINTER(ChunkDesc), C.POINTER(ChunkDesc), C.POINTER(Placement), C.c_int, C.POINTER(ChunkDesc), C.POINTER(C.c_uint64)]
lib.svo_world_chunk_stamp.argtypes = [_P, C.c_int, _P, C.c_int, C.POINTER(Placement), C.c_int, C.POINTER(C.c_uint64)]
lib.svo_chunk_extract.argtypes = [C.POINTER(ChunkDesc), C.POINTER(Placement), C.c_uint32, C.POINTER(C.c_float), C.c_float, C.POINTER(ChunkDesc), C.POINTER(C.c_uint64)]
lib.svo_world_chunk_extract.argtypes = [_P, C.c_int, _P, C.c_int, C.POINTER(Placement), C.POINTER(C.c_uint64)]
lib.svo_gbuffer_pack.argtypes = [_P, _P, C.c_int64, _P]
lib.svo_gbuffer_unpack.argtypes = [_P, _P, C.c_int64, _P]
lib.svo_shade_defaults.argtypes = [C.POINTER(ShadeParams)]
lib.svo_shade_defaults.restype = None
lib.svo_shade.argtypes = [C.POINTER(Camera), C.POINTER(ShadeParams), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]
lib.svo_shade_packed.argtypes = [C.POINTER(Camera), C.POINTER(ShadeParams), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]
lib.svo_shade_translucent.argtypes = [C.POINTER(Camera), C.POINTER(ShadeParams), C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]
lib.svo_trace_translucent.argtypes = [_P, C.POINTER(Camera), C.POINTER(TraceParams), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]
lib.svo_trace_local_shadows.argtypes = [_P, C.POINTER(Camera), C.POINTER(TraceParams), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                        C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]
lib.svo_shadowmap_fit.argtypes = [_P, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(ShadowMap)]
lib.svo_shadowmap_render.argtypes = [_P, C.POINTER(ShadowMap), C.POINTER(TraceParams), _P]
lib.svo_shadowmap_apply.argtypes = [C.POINTER(Camera), C.POINTER(ShadowMap), C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]
lib.svo_world_upload.argtypes = [_P, C.c_int]
lib.svo_world_update.argtypes = [_P, C.c_int, C.POINTER(ChunkDesc), C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
lib.svo_trace.argtypes = [_P, C.POINTER(Camera), C.POINTER(TraceParams), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]
lib.svo_trace_rows.argtypes = [_P, C.POINTER(Camera), C.POINTER(TraceParams), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]
lib.svo_trace_frames.argtypes = [_P, C.POINTER(Camera), C.c_int, C.POINTER(TraceParams), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]
lib.svo_trace_rows_frames.argtypes = [_P, C.POINTER(Camera), C.c_int, C.POINTER(TraceParams), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]
lib.svo_tile_order.argtypes = [_P, _P, _P, C.c_int, _P]
lib.svo_trace_rays.argtypes = [_P, _P, _P, C.c_int64, C.POINTER(TraceParams), _P, _P]
lib.svo_trace_segments.argtypes = [_P, _P, _P, _P, C.c_int64, C.POINTER(TraceParams), _P, _P]
lib.svo_world_locate.argtypes = [_P, _P, C.c_int64, C.POINTER(TraceParams), _P, _P]
lib.svo_hit_voxels.argtypes = [_P, _P, C.c_int64, _P, _P]
lib.svo_hit_uv.argtypes = [C.POINTER(Camera), C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]
lib.svo_shade_textured.argtypes = [C.POINTER(Camera), C.POINTER(ShadeParams), C.POINTER(Atlas), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]
lib.svo_hit_ao.argtypes = [_P, C.POINTER(Camera), C.POINTER(TraceParams), C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]
lib.svo_shade_ao.argtypes = [_P, C.c_float, C.c_int64, _P, _P]
lib.svo_trace_reflections.argtypes = [_P, C.POINTER(Camera), C.POINTER(TraceParams), C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]
lib.svo_shade_reflections.argtypes = [C.POINTER(Camera), C.POINTER(ShadeParams), C.POINTER(Mirror), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]
lib.svo_trace_lights.argtypes = [_P, C.POINTER(Camera), C.POINTER(TraceParams), C.POINTER(Light), C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                 _P, _P, _P, _P]
lib.svo_shade_lights.argtypes = [C.POINTER(Camera), C.POINTER(ShadeParams), C.POINTER(Light), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]
lib.svo_trace_instances.argtypes = [_P, _P, C.POINTER(Camera), C.POINTER(TraceParams), C.POINTER(Instance), C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                    _P, _P, _P, _P, _P]
lib.svo_trace_instance_shadows.argtypes = [_P, _P, C.POINTER(Camera), C.POINTER(TraceParams), C.POINTER(Instance), C.c_int, C.c_int64, C.c_float,
                                           C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]
lib.svo_shade_sky.argtypes = [C.POINTER(Camera), C.POINTER(Sky), C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]
lib.svo_frame_rgba8.argtypes = [_P, C.c_int64, _P, _P]
lib.svo_cursor_place.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), _P, C.c_float, _P, _P]
lib.svo_shade_boxes.argtypes = [C.POINTER(Camera), _P, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]
lib.svo_trace_last_ray_count.argtypes = [_P, _P, C.POINTER(C.c_uint64)]
lib.svo_world_prepare_light.argtypes = [_P, C.POINTER(C.c_float), _P]
lib.svo_world_prepared_light.argtypes = [_P, _P, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
lib.svo_world_prepared_bricks.argtypes = [_P, _P, C.POINTER(C.c_uint64)]
lib.svo_device_count.restype = C.c_int
lib.svo_device_alloc.argtypes = [C.c_size_t]
lib.svo_device_alloc.restype = _P
lib.svo_device_free.argtypes = [_P]
lib.svo_device_free.restype = None
lib.svo_device_cache_trim.argtypes = []
lib.svo_device_cache_trim.restype = None
lib.svo_memcpy_h2d.argtypes = [_P, _P, C.c_size_t]
lib.svo_memcpy_d2h.argtypes = [_P, _P, C.c_size_t]
lib.svo_stream_synchronize.argtypes = [_P]


def _check(rc: int, where: str) -> int:
    if rc < 0:
        raise SvoError(rc, where)
    return rc


def device_count() -> int:
    return lib.svo_device_count()


class DeviceBuffer:
    """A caller-owned HBM buffer (svo_device_alloc)."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        self.ptr = lib.svo_device_alloc(self.nbytes)
        if not self.ptr:
            raise SvoError(-3, "svo_device_alloc")

    @classmethod
    def from_numpy(cls, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        buf = cls(max(a.nbytes, 1))
        if a.nbytes:
            _check(lib.svo_memcpy_h2d(buf.ptr, a.ctypes.data, a.nbytes), "svo_memcpy_h2d")
        return buf

    def to_numpy(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            _check(lib.svo_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes), "svo_memcpy_d2h")
        return out

    def free(self):
        if self.ptr:
            lib.svo_device_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _normalize(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def make_camera(eye, forward, up_hint, vfov_deg: float, width: int, height: int) -> Camera:
    """Pinhole camera: orthonormal basis from (forward, up_hint); tangents from the vertical fov."""
    f = _normalize(forward)
    r = _normalize(np.cross(f, np.asarray(up_hint, dtype=np.float64)))
    u = np.cross(r, f)
    cam = Camera()
    cam.eye[:] = [float(np.float32(x)) for x in eye]
    cam.forward[:] = [float(np.float32(x)) for x in f]
    cam.right[:] = [float(np.float32(x)) for x in r]
    cam.up[:] = [float(np.float32(x)) for x in u]
    ty = math.tan(math.radians(vfov_deg) * 0.5)
    cam.tan_half_y = ty
    cam.tan_half_x = ty * width / height
    cam.width, cam.height = int(width), int(height)
    return cam


def default_camera(world_w: int, world_d: int, chunksize: int, width: int, height: int) -> Camera:
    """SURVEY.md §8d bench camera: eye (world_cx, 150, -40), forward normalize(0,-0.5,0.866), vfov 60."""
    cx = world_w * chunksize * 0.5
    return make_camera((cx, 150.0, -40.0), (0.0, -0.5, 0.866), (0.0, 1.0, 0.0), 60.0, width, height)


def c5_scene() -> dict:
    """BASELINE.json configs[4] as tests and bench.py build it: one depth-16 chunk refined to full depth only inside
    the band 62 <= x <= 66 (depth-10 bricks elsewhere; 13.4 M nodes, 2.5 M bricks), seen by a camera hovering 2 units
    over the band's terrain, so that a third of the primary hits are depth-16 voxels (14 branch levels on the path)."""
    return {
        "generate": dict(pyramid_resolution=4096, water=False, coarse_depth=10, refine_box=((62.0, -1e9, -1e9), (66.0, 1e9, 1e9))),
        "camera": lambda w, h: make_camera((64.3, 12.7, 96.5), (0.0, -0.8, 0.6), (0.0, 1.0, 0.0), 60.0, w, h),
    }


def trace_params(shadow: bool = False, kernel: int = KERNEL_AUTO, light_dir=(1.0, -1.0, 0.0), eps: float = 0.0,
                 caps=(0, 0, 0), counters_dev: Optional[int] = None, tiles_per_wave: int = 0, normal_mode: int = 0,
                 tile_cost_dev: Optional[int] = None, tile_order_dev: Optional[int] = None, launches_in_flight: int = 0,
                 semantics: int = 0, see_through: int = 0, light_clearance: bool = True, brick_clearance: bool = True,
                 dark_birth: bool = True) -> TraceParams:
    """semantics: SEMANTICS_CPU (src/Traverse.cpp) / SEMANTICS_GLSL (shaders/Chunkmarch.glsl); eps / caps 0 = that twin's own constants.
    see_through: a material (1..0xFFFF) every ray marches through as if it were empty; 0 = off.
    light_clearance / brick_clearance / dark_birth = False set SHADOW_NO_CLEARANCE / SHADOW_NO_BRICK_CLEARANCE / SHADOW_NO_DARK_BIRTH: the
    same records, more steps (light_clearance=False switches all three short cuts off, brick_clearance=False both that settle a ray at its hit)."""
    p = TraceParams()
    p.semantics = semantics
    p.see_through = see_through
    p.normal_mode = normal_mode
    p.eps = eps
    p.max_chunk_steps, p.max_tree_steps, p.max_twig_steps = caps
    p.shadow = (1 if light_clearance else 1 | SHADOW_NO_CLEARANCE) if shadow else 0    # (light_clearance=False: World.prepare_light's bits are ignored)
    if shadow and not brick_clearance:
        p.shadow |= SHADOW_NO_BRICK_CLEARANCE                                           # (... =False: the bits are used, the brick flags are not)
    if shadow and not dark_birth:
        p.shadow |= SHADOW_NO_DARK_BIRTH                                                # (... =False: a ray born in an occupied cell of the hit brick is marched)
    p.light_dir[:] = [float(x) for x in light_dir]
    p.kernel = kernel
    p.counters_dev = counters_dev
    p.tiles_per_wave = tiles_per_wave
    p.tile_cost_dev = tile_cost_dev
    p.tile_order_dev = tile_order_dev
    p.launches_in_flight = launches_in_flight
    return p


def chunk_write(path: str, chunk: dict, treestoragesize: int = 0, twigstoragesize: int = 0):
    """Ocroot::write (src/Octree.cpp:180-187): chunk = dict(position, size, depth, tree, twig)."""
    tree = np.ascontiguousarray(chunk["tree"], dtype=np.uint32)
    twig = np.ascontiguousarray(chunk["twig"], dtype=np.uint16)
    d = ChunkDesc()
    d.position[:] = [float(x) for x in chunk["position"]]
    d.size, d.depth = float(chunk["size"]), int(chunk["depth"])
    d.tree, d.trees = tree.ctypes.data_as(C.POINTER(C.c_uint32)), tree.size
    d.twig, d.twigs = twig.ctypes.data_as(C.POINTER(C.c_uint16)), twig.size // 64
    _check(lib.svo_chunk_write(path.encode(), C.byref(d), treestoragesize, twigstoragesize), "svo_chunk_write")


def chunk_read(path: str) -> dict:
    """Ocroot::read (src/Octree.cpp:189-201) -> dict(position, size, depth, tree, twig, treestoragesize, twigstoragesize)."""
    d = ChunkDesc()
    ts, ws = C.c_uint64(), C.c_uint64()
    _check(lib.svo_chunk_read(path.encode(), C.byref(d), C.byref(ts), C.byref(ws)), "svo_chunk_read")
    try:
        tree = np.ctypeslib.as_array(d.tree, shape=(d.trees,)).copy()
        twig = np.ctypeslib.as_array(d.twig, shape=(d.twigs * 64,)).copy() if d.twigs else np.zeros(0, np.uint16)
        return {"position": tuple(d.position), "size": d.size, "depth": d.depth, "tree": tree, "twig": twig,
                "treestoragesize": ts.value, "twigstoragesize": ws.value}
    finally:
        lib.svo_chunk_free(C.byref(d))


def _grid_depth(grid: np.ndarray) -> int:
    """depth of a [z, y, x] cube of 2^depth cells per axis (ValueError for any other shape)."""
    n = grid.shape[0] if grid.ndim == 3 else 0
    if n < 1 or grid.shape != (n, n, n) or n & (n - 1):
        raise ValueError("a grid is a [z, y, x] cube of 2^depth cells per axis")
    return n.bit_length() - 1


def chunk_from_grid(grid, position=(0.0, 0.0, 0.0), size: float = 128.0) -> dict:
    """svo_chunk_from_grid: the tree of a [z, y, x] uint16 grid of materials (0 = empty) as a chunk dict (World.create takes it)."""
    g = np.ascontiguousarray(grid, dtype=np.uint16)
    d = ChunkDesc()
    pos = None if position is None else (C.c_float * 3)(*[float(v) for v in position])
    _check(lib.svo_chunk_from_grid(g.ctypes.data, _grid_depth(g), pos, float(size), C.byref(d)), "svo_chunk_from_grid")
    try:
        tree = np.ctypeslib.as_array(d.tree, shape=(d.trees,)).copy()
        twig = np.ctypeslib.as_array(d.twig, shape=(d.twigs * 64,)).copy() if d.twigs else np.zeros(0, np.uint16)
        return {"position": tuple(d.position), "size": d.size, "depth": d.depth, "tree": tree, "twig": twig}
    finally:
        lib.svo_chunk_free(C.byref(d))


def grid_add_mesh(grid: np.ndarray, vertices, indices, origin=(0.0, 0.0, 0.0), cell: float = 1.0, material: int = 1, materials=None) -> np.ndarray:
    """svo_grid_add_mesh on the host: the triangles (vertices [nv, 3] float32, indices [nt, 3] uint32, materials [nt] uint16 or None:
    every triangle carries `material`) raised into `grid`, a C-contiguous [z, y, x] uint16 array, in place.  Returns grid."""
    if not (isinstance(grid, np.ndarray) and grid.dtype == np.uint16 and grid.flags.c_contiguous and grid.flags.writeable):
        raise ValueError("grid_add_mesh writes into a C-contiguous uint16 array")
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    ix = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
    mats = None if materials is None else np.ascontiguousarray(materials, dtype=np.uint16).reshape(ix.shape[0])
    m = Mesh(v.ctypes.data if v.size else None, ix.ctypes.data if ix.size else None, None if mats is None else mats.ctypes.data,
             v.shape[0], ix.shape[0], origin, cell, material)
    _check(lib.svo_grid_add_mesh(C.byref(m), _grid_depth(grid), grid.ctypes.data), "svo_grid_add_mesh")
    return grid


def device_grid_add_mesh(grid_ptr: int, depth: int, vertices_ptr, nvertices: int, indices_ptr, ntriangles: int, origin=(0.0, 0.0, 0.0),
                         cell: float = 1.0, material: int = 1, materials_ptr=None, stream: int = 0):
    """svo_device_grid_add_mesh: the same on device pointers (the grid 16-byte aligned); complete when it returns."""
    m = Mesh(vertices_ptr, indices_ptr, materials_ptr, nvertices, ntriangles, origin, cell, material)
    return _check(lib.svo_device_grid_add_mesh(C.byref(m), int(depth), grid_ptr, stream), "svo_device_grid_add_mesh")


def grid_fill_enclosed(grid: np.ndarray, material: int) -> int:
    """svo_grid_fill_enclosed on the host: the empty cells of the [z, y, x] uint16 array that no path of empty cells connects to the
    grid's faces become `material`, in place.  Returns how many."""
    if not (isinstance(grid, np.ndarray) and grid.dtype == np.uint16 and grid.flags.c_contiguous and grid.flags.writeable):
        raise ValueError("grid_fill_enclosed writes into a C-contiguous uint16 array")
    filled = C.c_uint64(0)
    _check(lib.svo_grid_fill_enclosed(grid.ctypes.data, _grid_depth(grid), int(material), C.byref(filled)), "svo_grid_fill_enclosed")
    return int(filled.value)


def device_grid_fill_enclosed(grid_ptr: int, depth: int, material: int, stream: int = 0) -> int:
    """svo_device_grid_fill_enclosed: the same on a device grid (16-byte aligned); complete when it returns.  Returns how many."""
    filled = C.c_uint64(0)
    _check(lib.svo_device_grid_fill_enclosed(grid_ptr, int(depth), int(material), C.byref(filled), stream), "svo_device_grid_fill_enclosed")
    return int(filled.value)


def _host_meshes(meshes):
    """A list of dict(vertices, indices[, origin, cell, material, materials]) as an svo_mesh array over host arrays, and what keeps
    those arrays alive."""
    arr, keep = (Mesh * max(len(meshes), 1))(), []
    for k, m in enumerate(meshes):
        v = np.ascontiguousarray(m["vertices"], dtype=np.float32).reshape(-1, 3)
        ix = np.ascontiguousarray(m["indices"], dtype=np.uint32).reshape(-1, 3)
        mats = None if m.get("materials") is None else np.ascontiguousarray(m["materials"], dtype=np.uint16).reshape(ix.shape[0])
        keep += [v, ix, mats]
        arr[k].__init__(v.ctypes.data if v.size else None, ix.ctypes.data if ix.size else None, None if mats is None else mats.ctypes.data,
                        v.shape[0], ix.shape[0], m.get("origin", (0.0, 0.0, 0.0)), m.get("cell", 1.0), m.get("material", 1))
    return arr, keep


def chunk_from_mesh(meshes, depth: int, position=(0.0, 0.0, 0.0), size: float = 128.0) -> dict:
    """svo_chunk_from_mesh on the host: the tree of the shell of the meshes - a list of dict(vertices [nv, 3] float32, indices [nt, 3]
    uint32, origin, cell, material, materials [nt] uint16 or None), the keyword arguments of grid_add_mesh - at `depth` (2 .. 16),
    built without the dense grid, as a chunk dict (World.create takes it)."""
    meshes = list(meshes)
    arr, keep = _host_meshes(meshes)
    d = ChunkDesc()
    pos = None if position is None else (C.c_float * 3)(*[float(v) for v in position])
    _check(lib.svo_chunk_from_mesh(arr, len(meshes), int(depth), pos, float(size), C.byref(d)), "svo_chunk_from_mesh")
    try:
        tree = np.ctypeslib.as_array(d.tree, shape=(d.trees,)).copy()
        twig = np.ctypeslib.as_array(d.twig, shape=(d.twigs * 64,)).copy() if d.twigs else np.zeros(0, np.uint16)
        return {"position": tuple(d.position), "size": d.size, "depth": d.depth, "tree": tree, "twig": twig}
    finally:
        lib.svo_chunk_free(C.byref(d))


def chunk_fill_enclosed(chunk: dict, material: int):
    """svo_chunk_fill_enclosed on the host: the chunk dict (position, size, depth, tree, twig) with every empty voxel that no path of
    empty voxels connects to the chunk's six faces turned into `material`, rebuilt minimal and in FIFO order without a dense grid
    (chunk depth 2 .. 16); `chunk` is left as it is.  Returns (the filled chunk dict, how many voxels were filled)."""
    tree = np.ascontiguousarray(chunk["tree"], dtype=np.uint32)
    twig = np.ascontiguousarray(chunk.get("twig", np.zeros(0, np.uint16)), dtype=np.uint16)
    src, d, filled = ChunkDesc(), ChunkDesc(), C.c_uint64(0)
    src.position[:] = [float(x) for x in chunk["position"]]
    src.size, src.depth = float(chunk["size"]), int(chunk["depth"])
    src.tree, src.trees = tree.ctypes.data_as(C.POINTER(C.c_uint32)), tree.size
    src.twig, src.twigs = twig.ctypes.data_as(C.POINTER(C.c_uint16)), twig.size // 64
    _check(lib.svo_chunk_fill_enclosed(C.byref(src), int(material), C.byref(d), C.byref(filled)), "svo_chunk_fill_enclosed")
    try:
        otree = np.ctypeslib.as_array(d.tree, shape=(d.trees,)).copy()
        otwig = np.ctypeslib.as_array(d.twig, shape=(d.twigs * 64,)).copy() if d.twigs else np.zeros(0, np.uint16)
        return {"position": tuple(d.position), "size": d.size, "depth": d.depth, "tree": otree, "twig": otwig}, int(filled.value)
    finally:
        lib.svo_chunk_free(C.byref(d))


def _host_chunk_desc(chunk: dict):
    """A chunk dict as an svo_chunk_desc over host arrays, and what keeps those arrays alive."""
    tree = np.ascontiguousarray(chunk["tree"], dtype=np.uint32)
    twig = np.ascontiguousarray(chunk.get("twig", np.zeros(0, np.uint16)), dtype=np.uint16)
    d = ChunkDesc()
    d.position[:] = [float(x) for x in chunk["position"]]
    d.size, d.depth = float(chunk["size"]), int(chunk["depth"])
    d.tree, d.trees = tree.ctypes.data_as(C.POINTER(C.c_uint32)), tree.size
    d.twig, d.twigs = twig.ctypes.data_as(C.POINTER(C.c_uint16)), twig.size // 64
    return d, (tree, twig)


def chunk_combine(a: dict, b: dict, op: int):
    """svo_chunk_combine on the host: the chunk dicts a and b (one depth, 2 .. 16) combined cell by cell on their trees by COMBINE_* -
    MAX max(a, b), UNDER b where a is empty, OVER b on top, SUBTRACT b's shape carved out of a, INTERSECT a where b is -, rebuilt
    minimal and in FIFO order without a dense grid, in a's frame; a and b are left as they are.  Returns (the combined chunk dict, how
    many voxels differ from a's)."""
    da, keep_a = _host_chunk_desc(a)
    db, keep_b = _host_chunk_desc(b)
    d, changed = ChunkDesc(), C.c_uint64(0)
    _check(lib.svo_chunk_combine(C.byref(da), C.byref(db), int(op), C.byref(d), C.byref(changed)), "svo_chunk_combine")
    try:
        otree = np.ctypeslib.as_array(d.tree, shape=(d.trees,)).copy()
        otwig = np.ctypeslib.as_array(d.twig, shape=(d.twigs * 64,)).copy() if d.twigs else np.zeros(0, np.uint16)
        return {"position": tuple(d.position), "size": d.size, "depth": d.depth, "tree": otree, "twig": otwig}, int(changed.value)
    finally:
        lib.svo_chunk_free(C.byref(d))

def chunk_stamp(a: dict, b: dict, offset, orient: int, op: int):
    """svo_chunk_stamp on the host: chunk dict b (depth <= a's, both 2 .. 16) placed into chunk dict a with its cube starting at a's
    cell `offset` (x, y, z), in orientation `orient` (0 .. 47: perm * 8 + flips, ORIENT_ROTATIONS are the proper ones), through
    COMBINE_* `op` - one cell of b is one cell of a, outside b's cube b is empty -, rebuilt minimal and in FIFO order without a dense
    grid, in a's frame; a and b are left as they are.  Returns (the stamped chunk dict, how many voxels differ from a's)."""
    da, keep_a = _host_chunk_desc(a)
    db, keep_b = _host_chunk_desc(b)
    d, changed, pl = ChunkDesc(), C.c_uint64(0), Placement(offset, orient)
    _check(lib.svo_chunk_stamp(C.byref(da), C.byref(db), C.byref(pl), int(op), C.byref(d), C.byref(changed)), "svo_chunk_stamp")
    try:
        otree = np.ctypeslib.as_array(d.tree, shape=(d.trees,)).copy()
        otwig = np.ctypeslib.as_array(d.twig, shape=(d.twigs * 64,)).copy() if d.twigs else np.zeros(0, np.uint16)
        return {"position": tuple(d.position), "size": d.size, "depth": d.depth, "tree": otree, "twig": otwig}, int(changed.value)
    finally:
        lib.svo_chunk_free(C.byref(d))


def chunk_extract(a: dict, offset, orient: int, depth: int, position=(0.0, 0.0, 0.0), size: float = 128.0):
    """svo_chunk_extract on the host, the stamp's inverse: the cube of (2^depth)^3 cells of chunk dict a (depth <= a's, both 2 .. 16)
    that starts at a's cell `offset` (x, y, z), as a chunk of its own in the frame `position` / `size` - oriented so that stamping it
    back with the same `offset` and `orient` puts every cell where it came from; what lies outside a reads 0.  Rebuilt minimal and in
    FIFO order without a dense grid; a is left as it is.  Returns (the extracted chunk dict, how many of its voxels are not 0)."""
    da, keep_a = _host_chunk_desc(a)
    d, occupied, pl = ChunkDesc(), C.c_uint64(0), Placement(offset, orient)
    _check(lib.svo_chunk_extract(C.byref(da), C.byref(pl), int(depth), (C.c_float * 3)(*position), float(size), C.byref(d), C.byref(occupied)), "svo_chunk_extract")
    try:
        otree = np.ctypeslib.as_array(d.tree, shape=(d.trees,)).copy()
        otwig = np.ctypeslib.as_array(d.twig, shape=(d.twigs * 64,)).copy() if d.twigs else np.zeros(0, np.uint16)
        return {"position": tuple(d.position), "size": d.size, "depth": d.depth, "tree": otree, "twig": otwig}, int(occupied.value)
    finally:
        lib.svo_chunk_free(C.byref(d))


def gbuffer_pack(gbuffer_ptr: int, packed_ptr: int, n: int, stream: int = 0):
    _check(lib.svo_gbuffer_pack(gbuffer_ptr, packed_ptr, n, stream), "svo_gbuffer_pack")


def gbuffer_unpack(packed_ptr: int, gbuffer_ptr: int, n: int, stream: int = 0):
    _check(lib.svo_gbuffer_unpack(packed_ptr, gbuffer_ptr, n, stream), "svo_gbuffer_unpack")


def shade_defaults() -> ShadeParams:
    """The reference's lights (src/Main.cpp:101-131) and material table (shaders/World.Fragment.glsl:63-73)."""
    p = ShadeParams()
    lib.svo_shade_defaults(C.byref(p))
    return p


def shade(cam: Camera, params: ShadeParams, rect, gbuffer_ptr: int, rgba_ptr: int, stream: int = 0):
    x0, y0, w, h = rect
    _check(lib.svo_shade(C.byref(cam), C.byref(params), x0, y0, w, h, gbuffer_ptr, rgba_ptr, stream), "svo_shade")


def shade_packed(cam: Camera, params: ShadeParams, rect, packed_ptr: int, rgba_ptr: int, stream: int = 0):
    """svo_shade over the 8-byte records of gbuffer_pack."""
    x0, y0, w, h = rect
    _check(lib.svo_shade_packed(C.byref(cam), C.byref(params), x0, y0, w, h, packed_ptr, rgba_ptr, stream), "svo_shade_packed")


def shade_translucent(cam: Camera, params: ShadeParams, rect, surface_ptr: int, behind_ptr: int, rgba_ptr: int,
                      absorption: float = 0.0, stream: int = 0):
    """svo_shade_translucent: ParallaxAlpha's blend of the two G-buffers of World.trace_translucent (absorption 0 = 0.5)."""
    x0, y0, w, h = rect
    _check(lib.svo_shade_translucent(C.byref(cam), C.byref(params), absorption, x0, y0, w, h, surface_ptr, behind_ptr, rgba_ptr, stream),
           "svo_shade_translucent")


def hit_uv(cam: Camera, eps: float, rect, gbuffer_ptr: int, voxels_ptr: int, uv_ptr: int, stream: int = 0):
    """svo_hit_uv: the reference's leafUV per pixel ([w*h][2] float) from the G-buffer and World.hit_voxels' records; eps 0 = 1/8192."""
    x0, y0, w, h = rect
    _check(lib.svo_hit_uv(C.byref(cam) if cam is not None else None, eps, x0, y0, w, h, gbuffer_ptr, voxels_ptr, uv_ptr, stream), "svo_hit_uv")


def shade_textured(cam: Camera, params: ShadeParams, atlas: Atlas, rect, gbuffer_ptr: int, voxels_ptr: int, rgba_ptr: int, stream: int = 0):
    """svo_shade_textured: svo_shade with the albedo sampled from the caller's atlas at the hit's leafUV."""
    x0, y0, w, h = rect
    _check(lib.svo_shade_textured(C.byref(cam) if cam is not None else None, C.byref(params) if params is not None else None,
                                  C.byref(atlas) if atlas is not None else None, x0, y0, w, h, gbuffer_ptr, voxels_ptr, rgba_ptr, stream),
           "svo_shade_textured")


def shade_ao(ao_ptr: int, strength: float, n: int, rgba_ptr: int, stream: int = 0):
    """svo_shade_ao: r, g, b of n float4 pixels scaled by 1 - strength * (1 - ao), ao the floats World.hit_ao wrote; behind a shade call,
    before shade_sky, shade_boxes and frame_rgba8."""
    _check(lib.svo_shade_ao(ao_ptr, strength, n, rgba_ptr, stream), "svo_shade_ao")


def shade_sky(cam: Camera, sky: Sky, rect, rgba_ptr: int, gbuffer_ptr: Optional[int] = None, packed_ptr: Optional[int] = None, stream: int = 0):
    """svo_shade_sky: r, g, b of every pixel whose record lacks HIT_FLAG replaced by the cube map's colour along the pixel's ray, over an
    image a shade call has written; the records are given as gbuffer_ptr (32-byte) or packed_ptr (gbuffer_pack's), exactly one of them."""
    x0, y0, w, h = rect
    _check(lib.svo_shade_sky(C.byref(cam) if cam is not None else None, C.byref(sky) if sky is not None else None, x0, y0, w, h,
                             gbuffer_ptr, packed_ptr, rgba_ptr, stream), "svo_shade_sky")


def shade_reflections(cam: Camera, params: ShadeParams, mirror: Mirror, rect, gbuffer_ptr: int, voxels_ptr: int, reflect_ptr: int, rgba_ptr: int,
                      stream: int = 0):
    """svo_shade_reflections: what the mirror rays of World.trace_reflections saw (reflect_ptr), blended by mirror's Fresnel term over
    the image a shade call wrote for the same records; behind shade_ao, before shade_boxes and frame_rgba8.  params.eps is the launch's."""
    x0, y0, w, h = rect
    _check(lib.svo_shade_reflections(C.byref(cam) if cam is not None else None, C.byref(params) if params is not None else None,
                                     C.byref(mirror) if mirror is not None else None, x0, y0, w, h, gbuffer_ptr, voxels_ptr, reflect_ptr, rgba_ptr,
                                     stream), "svo_shade_reflections")


def light_array(lights):
    """A sequence of Light as the contiguous svo_light array the light-list calls take (None stays None); (array, count)."""
    if lights is None:
        return None, 0
    lights = list(lights)
    arr = (Light * max(len(lights), 1))()
    for j, l in enumerate(lights):
        C.memmove(C.byref(arr, j * C.sizeof(Light)), C.byref(l), C.sizeof(Light))
    return arr, len(lights)


def instance_array(instances):
    """A sequence of Instance as the contiguous svo_instance array the instance calls take (None stays None); (array, count)."""
    if instances is None:
        return None, 0
    instances = list(instances)
    arr = (Instance * max(len(instances), 1))()
    for j, i in enumerate(instances):
        C.memmove(C.byref(arr, j * C.sizeof(Instance)), C.byref(i), C.sizeof(Instance))
    return arr, len(instances)


def shade_lights(cam: Camera, params: ShadeParams, rect, gbuffer_ptr: int, lights, rgba_ptr: int, visible_ptr: Optional[int] = None, stream: int = 0):
    """svo_shade_lights: the point lights of `lights` (a sequence of Light), each windowed to its reach, added to the image a shade call
    wrote for the same records; visible_ptr: the words World.trace_lights wrote (None: every light unshadowed).  Before shade_ao."""
    x0, y0, w, h = rect
    arr, n = light_array(lights)
    _check(lib.svo_shade_lights(C.byref(cam) if cam is not None else None, C.byref(params) if params is not None else None, arr, n,
                                x0, y0, w, h, gbuffer_ptr, visible_ptr, rgba_ptr, stream), "svo_shade_lights")


def frame_rgba8(rgba_ptr: int, n: int, out_ptr: int, stream: int = 0):
    """svo_frame_rgba8: n float4 pixels to RGBA8 (4 bytes a pixel, memory order R, G, B, A; alpha 255)."""
    _check(lib.svo_frame_rgba8(rgba_ptr, n, out_ptr, stream), "svo_frame_rgba8")


def cursor_place(origin, direction, record_ptr: int, size: float, box_ptr: int, stream: int = 0):
    """svo_cursor_place: the cursor cube of edge `size` centred on the hit of the ray (origin, direction) whose record the march wrote at
    record_ptr, into the svo_box at box_ptr (bmin, size, BOX_HIDDEN only); a record without a usable hit hides the box."""
    vec = [None if v is None else (C.c_float * 3)(*[float(c) for c in v]) for v in (origin, direction)]
    _check(lib.svo_cursor_place(vec[0], vec[1], record_ptr, size, box_ptr, stream), "svo_cursor_place")


def shade_boxes(cam: Camera, boxes_ptr: int, nboxes: int, rect, rgba_ptr: int, near_plane: float = 0.0, far_plane: float = 0.0, stream: int = 0):
    """svo_shade_boxes: nboxes svo_box records (BOX_DTYPE on the device) blended in list order over the image a shade call (and
    shade_sky) wrote, depth-tested against its depth floats; planes 0 = 0.125 / 8192."""
    x0, y0, w, h = rect
    _check(lib.svo_shade_boxes(C.byref(cam) if cam is not None else None, boxes_ptr, nboxes, near_plane, far_plane, x0, y0, w, h, rgba_ptr, stream),
           "svo_shade_boxes")


def shadowmap_apply(cam: Camera, smap: ShadowMap, eps: float, bias: float, rect, gbuffer_ptr: int, stream: int = 0):
    """svo_shadowmap_apply: SHADOW_TRACED and SHADOWED of every usable hit of the G-buffer svo_trace(cam, rect) filled, from a lookup of
    its sample point in the rendered map; eps is the launch's (0 = 1/8192), bias in world units along the light."""
    x0, y0, w, h = rect
    _check(lib.svo_shadowmap_apply(C.byref(cam) if cam is not None else None, C.byref(smap) if smap is not None else None, eps, bias,
                                   x0, y0, w, h, gbuffer_ptr, stream), "svo_shadowmap_apply")


def see_through_chunk(chunk: dict, material: int) -> dict:
    """The chunk as a see-through march of `material` sees it: LEAF nodes of that material (offset & 0xFFFF) and brick cells
    holding it set to 0, the tree's shape unchanged.  Host numpy; what svo_trace_params.see_through is defined against."""
    tree = np.array(chunk["tree"], dtype=np.uint32, copy=True)
    twig = np.array(chunk["twig"], dtype=np.uint16, copy=True)
    tree[((tree >> 30) == LEAF) & ((tree & 0xFFFF) == material)] = 0
    twig[twig == material] = 0
    out = dict(chunk)
    out["tree"], out["twig"] = tree, twig
    return out


class World:
    """Host handle of a chunk grid; shaped like the reference's `World` (src/World.h:44-68)."""

    def __init__(self, handle):
        self._h = handle

    # -- construction ----------------------------------------------------------------------
    @classmethod
    def generate(cls, w: int, h: int, d: int, chunksize: int = 128, depth: int = 8, chunkcoordmin=(0, 0, 0),
                 pyramid_resolution: int = 0, amplitude: float = 64.0, yshift: float = 16.0, seed: int = 0,
                 water: bool = True, water_level: float = 6.0, water_material: int = 6, threads: int = 0,
                 coarse_depth: int = 0, refine_box=None, build_device: Optional[int] = None) -> "World":
        """coarse_depth / refine_box=((x0,y0,z0),(x1,y1,z1)): sparse refinement (full depth only inside the box)."""
        tp = TerrainParams(depth, pyramid_resolution, amplitude, yshift, seed, 1 if water else 0, water_level,
                           water_material, threads, coarse_depth)
        if refine_box is not None:
            tp.refine_min[:] = [float(v) for v in refine_box[0]]
            tp.refine_max[:] = [float(v) for v in refine_box[1]]
        tp.build_device_plus1 = 0 if build_device is None else int(build_device) + 1     # None: host threads
        ccm = (C.c_int * 3)(*chunkcoordmin)
        out = _P()
        _check(lib.svo_world_generate(w, h, d, chunksize, ccm, C.byref(tp), C.byref(out)), "svo_world_generate")
        return cls(out)

    @classmethod
    def create(cls, chunks: Sequence[dict], w: int, h: int, d: int, chunksize: int, chunkcoordmin=(0, 0, 0)) -> "World":
        """chunks: dicts with position(3), size, depth, tree (uint32 array), twig (uint16 array, 64 per brick)."""
        descs = (ChunkDesc * len(chunks))()
        keep = []
        for i, c in enumerate(chunks):
            tree = np.ascontiguousarray(c["tree"], dtype=np.uint32)
            twig = np.ascontiguousarray(c.get("twig", np.zeros(0, np.uint16)), dtype=np.uint16)
            keep += [tree, twig]
            descs[i].position[:] = [float(x) for x in c["position"]]
            descs[i].size = float(c["size"])
            descs[i].depth = int(c["depth"])
            descs[i].tree = tree.ctypes.data_as(C.POINTER(C.c_uint32))
            descs[i].trees = tree.size
            descs[i].twig = twig.ctypes.data_as(C.POINTER(C.c_uint16))
            descs[i].twigs = twig.size // 64
        ccm = (C.c_int * 3)(*chunkcoordmin)
        out = _P()
        _check(lib.svo_world_create(descs, len(chunks), w, h, d, chunksize, ccm, C.byref(out)), "svo_world_create")
        return cls(out)

    def destroy(self):
        if self._h:
            lib.svo_world_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # -- inspection ------------------------------------------------------------------------
    @property
    def info(self) -> WorldInfo:
        wi = WorldInfo()
        _check(lib.svo_world_info_get(self._h, C.byref(wi)), "svo_world_info_get")
        return wi

    def chunk(self, i: int, copy: bool = True) -> dict:
        """Host pools of chunk i.  copy=False borrows the library's arrays (valid until destroy/update)."""
        d = ChunkDesc()
        _check(lib.svo_world_chunk(self._h, i, C.byref(d)), "svo_world_chunk")
        tree = np.ctypeslib.as_array(d.tree, shape=(d.trees,))
        twig = np.ctypeslib.as_array(d.twig, shape=(d.twigs * 64,)) if d.twigs else np.zeros(0, np.uint16)
        if copy:
            tree, twig = tree.copy(), twig.copy()
        return {"position": tuple(d.position), "size": d.size, "depth": d.depth, "tree": tree, "twig": twig}

    def index_float(self, p) -> tuple:
        pp = (C.c_float * 3)(*[float(x) for x in p])
        q = (C.c_int * 3)()
        _check(lib.svo_world_index_float(self._h, pp, q), "svo_world_index_float")
        return tuple(q)

    def index(self, x: int, y: int, z: int) -> int:
        return _check(lib.svo_world_index(self._h, x, y, z), "svo_world_index")

    # -- device ----------------------------------------------------------------------------
    def upload(self, device: int = 0) -> "World":
        self.upload_status = _check(lib.svo_world_upload(self._h, device), "svo_world_upload")     # SVO_OK or OK_LITERAL_ONLY
        return self

    def update(self, chunk: int, desc: dict, tree_range=(0, 0), twig_range=(0, 0), realloc: bool = False):
        tree = np.ascontiguousarray(desc["tree"], dtype=np.uint32)
        twig = np.ascontiguousarray(desc["twig"], dtype=np.uint16)
        d = ChunkDesc()
        d.position[:] = [float(x) for x in desc["position"]]
        d.size, d.depth = float(desc["size"]), int(desc["depth"])
        d.tree, d.trees = tree.ctypes.data_as(C.POINTER(C.c_uint32)), tree.size
        d.twig, d.twigs = twig.ctypes.data_as(C.POINTER(C.c_uint16)), twig.size // 64
        return _check(lib.svo_world_update(self._h, chunk, C.byref(d), tree_range[0], tree_range[1], twig_range[0], twig_range[1],
                                           1 if realloc else 0), "svo_world_update")

    def edit_box(self, chunk: int, op: int, lo, hi, material: int = 0):
        """Ocroot::build / destroy / replace + World::modify on the device (svo_world_edit_box); op = EDIT_BUILD / EDIT_DESTROY / EDIT_REPLACE."""
        return _check(lib.svo_world_edit_box(self._h, int(chunk), int(op), (C.c_float * 3)(*[float(v) for v in lo]),
                                             (C.c_float * 3)(*[float(v) for v in hi]), C.c_uint16(int(material))), "svo_world_edit_box")

    def edit_cube(self, op: int, bmin, size: float, material: int = 0):
        """svo_world_edit_cube: the reference's modify() - the cube [bmin, bmin + size] to every chunk that holds one of its corners, each
        once.  Returns (status, [chunks edited, in order])."""
        chunks, n = (C.c_int * 8)(), C.c_int(0)
        rc = _check(lib.svo_world_edit_cube(self._h, int(op), None if bmin is None else (C.c_float * 3)(*[float(v) for v in bmin]), float(size),
                                            C.c_uint16(int(material)), chunks, C.byref(n)), "svo_world_edit_cube")
        return rc, list(chunks[:n.value])

    def edit_ball(self, chunk: int, op: int, centre, radius: float, material: int = 0):
        """svo_world_edit_ball: edit_box with the closed ball |p - centre| <= radius as the region; op = EDIT_BUILD / EDIT_DESTROY / EDIT_REPLACE."""
        return _check(lib.svo_world_edit_ball(self._h, int(chunk), int(op), None if centre is None else (C.c_float * 3)(*[float(v) for v in centre]),
                                              float(radius), C.c_uint16(int(material))), "svo_world_edit_ball")

    def edit_ball_all(self, op: int, centre, radius: float, material: int = 0):
        """svo_world_edit_ball_all: the ball to every chunk whose box it touches, in World::index order, each once.  Returns (status,
        [chunks edited, in order])."""
        cap = max(int(self.info.width * self.info.height * self.info.depth), 1)
        chunks, n = (C.c_int * cap)(), C.c_int(0)
        rc = _check(lib.svo_world_edit_ball_all(self._h, int(op), None if centre is None else (C.c_float * 3)(*[float(v) for v in centre]),
                                                float(radius), C.c_uint16(int(material)), chunks, cap, C.byref(n)), "svo_world_edit_ball_all")
        return rc, list(chunks[:n.value])

    def compact(self, chunk: int):
        """Ocroot::defragcopy + World::modify(realloc) (svo_world_compact): chunk rebuilt from its root, uniform bricks and blocks folded."""
        return _check(lib.svo_world_compact(self._h, int(chunk)), "svo_world_compact")

    def coarsen(self, chunk: int):
        """Ocroot::lodmm + World::modify(realloc) (svo_world_coarsen): chunk one level coarser, depth -> depth - 1."""
        return _check(lib.svo_world_coarsen(self._h, int(chunk)), "svo_world_coarsen")

    def chunk_from_grid(self, chunk: int, grid_ptr: int, depth: int):
        """svo_world_chunk_from_grid: chunk replaced by the tree of the (2^depth)^3 uint16 grid at grid_ptr (device memory, x fastest)."""
        return _check(lib.svo_world_chunk_from_grid(self._h, int(chunk), grid_ptr, int(depth)), "svo_world_chunk_from_grid")

    def chunk_from_mesh(self, chunk: int, meshes: Sequence[Mesh], depth: int):
        """svo_world_chunk_from_mesh: chunk replaced by the tree of the shell of the meshes at `depth` (2 .. 16), built on the device
        without the dense grid.  meshes: Mesh structs whose three arrays are device pointers."""
        meshes = list(meshes)
        arr = (Mesh * max(len(meshes), 1))()
        for k, m in enumerate(meshes):
            C.memmove(C.byref(arr[k]), C.byref(m), C.sizeof(Mesh))
        return _check(lib.svo_world_chunk_from_mesh(self._h, int(chunk), arr, len(meshes), int(depth)), "svo_world_chunk_from_mesh")

    def chunk_fill_enclosed(self, chunk: int, material: int) -> int:
        """svo_world_chunk_fill_enclosed: chunk replaced by its filled form - every empty voxel that no path of empty voxels connects to
        the chunk's six faces becomes `material` -, built on the device on the tree (chunk depth 2 .. 16); complete when it returns.
        Returns how many voxels were filled; the status (SVO_OK or SVO_OK_LITERAL_ONLY) is in self.fill_status."""
        filled = C.c_uint64(0)
        self.fill_status = _check(lib.svo_world_chunk_fill_enclosed(self._h, int(chunk), int(material), C.byref(filled)), "svo_world_chunk_fill_enclosed")
        return int(filled.value)

    def chunk_combine(self, chunk: int, src_world: "World", src_chunk: int, op: int) -> int:
        """svo_world_chunk_combine: chunk replaced by its cell-wise combination (COMBINE_*) with chunk src_chunk of src_world - an
        uploaded world on the same device, which may be this one -, built on the device on the two trees (one chunk depth, 2 .. 16);
        complete when it returns.  Returns how many voxels changed; the status (SVO_OK or SVO_OK_LITERAL_ONLY) is in self.combine_status."""
        changed = C.c_uint64(0)
        self.combine_status = _check(lib.svo_world_chunk_combine(self._h, int(chunk), None if src_world is None else src_world._h, int(src_chunk), int(op),
                                                                 C.byref(changed)), "svo_world_chunk_combine")
        return int(changed.value)

    def chunk_stamp(self, chunk: int, src_world: "World", src_chunk: int, offset, orient: int, op: int) -> int:
        """svo_world_chunk_stamp: chunk replaced by itself with chunk src_chunk of src_world - an uploaded world on the same device,
        which may be this one; its depth at most this chunk's - placed at cell `offset` in orientation `orient` through COMBINE_* `op`,
        built on the device on the two trees; complete when it returns.  Returns how many voxels changed; the status (SVO_OK or
        SVO_OK_LITERAL_ONLY) is in self.stamp_status."""
        changed, pl = C.c_uint64(0), Placement(offset, orient)
        self.stamp_status = _check(lib.svo_world_chunk_stamp(self._h, int(chunk), None if src_world is None else src_world._h, int(src_chunk), C.byref(pl), int(op),
                                                             C.byref(changed)), "svo_world_chunk_stamp")
        return int(changed.value)

    def chunk_extract(self, chunk: int, src_world: "World", src_chunk: int, offset, orient: int) -> int:
        """svo_world_chunk_extract, the stamp's inverse: chunk replaced by the cube of its own number of cells that starts at cell
        `offset` of chunk src_chunk of src_world - an uploaded world on the same device, which may be this one, and the chunk may be
        this chunk; its depth at least this chunk's -, oriented so that stamping it back with the same placement puts every cell where
        it came from; built on the device on the tree; complete when it returns.  Returns how many of its voxels are not 0; the status
        (SVO_OK or SVO_OK_LITERAL_ONLY) is in self.extract_status."""
        occupied, pl = C.c_uint64(0), Placement(offset, orient)
        self.extract_status = _check(lib.svo_world_chunk_extract(self._h, int(chunk), None if src_world is None else src_world._h, int(src_chunk), C.byref(pl),
                                                                 C.byref(occupied)), "svo_world_chunk_extract")
        return int(occupied.value)

    def chunk_to_grid(self, chunk: int, depth: int, out_ptr: int, stream: int = 0):
        """svo_world_chunk_to_grid: the chunk's voxels as a (2^depth)^3 uint16 grid at out_ptr (device memory), asynchronous on stream."""
        return _check(lib.svo_world_chunk_to_grid(self._h, int(chunk), int(depth), out_ptr, stream), "svo_world_chunk_to_grid")

    def set_chunk_grid(self, chunk: int, grid):
        """World.chunk_from_grid over a host [z, y, x] uint16 array."""
        g = np.ascontiguousarray(grid, dtype=np.uint16)
        depth = _grid_depth(g)
        gd = DeviceBuffer.from_numpy(g)
        try:
            return self.chunk_from_grid(chunk, gd.ptr, depth)
        finally:
            gd.free()

    def chunk_grid(self, chunk: int, depth: int) -> np.ndarray:
        """World.chunk_to_grid into a host [z, y, x] uint16 array."""
        n = 1 << max(int(depth), 0) if int(depth) <= 10 else 1
        out = DeviceBuffer(max(n ** 3 * 2, 16))
        try:
            self.chunk_to_grid(chunk, depth, out.ptr)
            _check(lib.svo_stream_synchronize(None), "svo_stream_synchronize")
            return out.to_numpy(np.uint16, n ** 3).reshape(n, n, n)
        finally:
            out.free()

    def shift(self, offset):
        """World::shift (src/World.cpp:334-378): slide the grid one chunk along one axis."""
        off = (C.c_int * 3)(*[int(v) for v in offset])
        return _check(lib.svo_world_shift(self._h, off), "svo_world_shift")

    # raw launches on caller-owned device memory (bench.py passes torch tensors' data_ptr())
    def trace(self, cam: Camera, params: TraceParams, rect, out_ptr: int, stream: int = 0):
        x0, y0, w, h = rect
        _check(lib.svo_trace(self._h, C.byref(cam), C.byref(params), x0, y0, w, h, out_ptr, stream), "svo_trace")

    def trace_rows(self, cam: Camera, params: TraceParams, band0: int, band_stride: int, nbands: int, band_height: int,
                   out_ptr: int, stream: int = 0):
        _check(lib.svo_trace_rows(self._h, C.byref(cam), C.byref(params), band0, band_stride, nbands, band_height,
                                  out_ptr, stream), "svo_trace_rows")

    def trace_frames(self, cams, params: TraceParams, rect, out_ptr: int, stream: int = 0):
        """svo_trace_frames: len(cams) frames (<= MAX_FRAMES, one image size) in one launch; out holds the rasters back to back."""
        x0, y0, w, h = rect
        arr = (Camera * len(cams))(*cams)
        _check(lib.svo_trace_frames(self._h, arr, len(cams), C.byref(params), x0, y0, w, h, out_ptr, stream), "svo_trace_frames")

    def trace_rows_frames(self, cams, params: TraceParams, band0: int, band_stride: int, nbands: int, band_height: int,
                          out_ptr: int, stream: int = 0):
        arr = (Camera * len(cams))(*cams)
        _check(lib.svo_trace_rows_frames(self._h, arr, len(cams), C.byref(params), band0, band_stride, nbands, band_height,
                                         out_ptr, stream), "svo_trace_rows_frames")

    def trace_rays(self, origins_ptr: int, dirs_ptr: int, n: int, params: TraceParams, out_ptr: int, stream: int = 0):
        _check(lib.svo_trace_rays(self._h, origins_ptr, dirs_ptr, n, C.byref(params), out_ptr, stream), "svo_trace_rays")

    def trace_segments(self, origins_ptr: int, dirs_ptr: int, tmax_ptr: int, n: int, params: TraceParams, out_ptr: int, stream: int = 0):
        """svo_trace_segments: trace_rays with a far end per ray (tmax_ptr: [n] float on the device); a hit counts only if t < tmax."""
        _check(lib.svo_trace_segments(self._h, origins_ptr, dirs_ptr, tmax_ptr, n, C.byref(params), out_ptr, stream), "svo_trace_segments")

    def locate(self, points_ptr: int, n: int, params: Optional[TraceParams], out_ptr: int, stream: int = 0):
        """svo_world_locate: the voxel under each of n points ([n][3] float on the device) into out_ptr (n VOXEL_DTYPE records).
        Only kernel, semantics and see_through of params are read; None = defaults."""
        _check(lib.svo_world_locate(self._h, points_ptr, n, C.byref(params) if params is not None else None, out_ptr, stream), "svo_world_locate")

    def hit_voxels(self, gbuffer_ptr: int, n: int, out_ptr: int, stream: int = 0):
        """svo_hit_voxels: the voxel box of each of n G-buffer records (HIT_DTYPE on the device) into out_ptr (n VOXEL_DTYPE records);
        all zero for a record without a usable hit or whose (chunk, node, cell) name nothing reachable."""
        _check(lib.svo_hit_voxels(self._h, gbuffer_ptr, n, out_ptr, stream), "svo_hit_voxels")

    def hit_ao(self, cam: Camera, params: Optional[TraceParams], rect, gbuffer_ptr: int, voxels_ptr: int, ao_ptr: int, cell: float = 0.0, stream: int = 0):
        """svo_hit_ao: voxel ambient occlusion (w*h floats in [0, 1], 1 = open) of the G-buffer svo_trace(cam, rect) filled and the
        records hit_voxels wrote for it; cell 0 = the finest voxel of each hit's chunk.  Only eps, semantics, kernel and see_through of
        params are read; None = defaults."""
        x0, y0, w, h = rect
        _check(lib.svo_hit_ao(self._h, C.byref(cam) if cam is not None else None, C.byref(params) if params is not None else None, cell,
                              x0, y0, w, h, gbuffer_ptr, voxels_ptr, ao_ptr, stream), "svo_hit_ao")

    def trace_reflections(self, cam: Camera, params: TraceParams, rect, gbuffer_ptr: int, voxels_ptr: int, reflect_ptr: int, material: int = 0,
                          stream: int = 0):
        """svo_trace_reflections on the G-buffer svo_trace(cam, params, rect) filled and the records hit_voxels wrote for it: the record
        of the mirror ray of every usable hit of `material` (0 = any) into reflect_ptr (w*h HIT_DTYPE records), all zero elsewhere."""
        x0, y0, w, h = rect
        _check(lib.svo_trace_reflections(self._h, C.byref(cam) if cam is not None else None, C.byref(params) if params is not None else None,
                                         material, x0, y0, w, h, gbuffer_ptr, voxels_ptr, reflect_ptr, stream), "svo_trace_reflections")

    def trace_translucent(self, cam: Camera, params: TraceParams, rect, surface_ptr: int, behind_ptr: int, stream: int = 0):
        """svo_trace_translucent: the surface G-buffer and, behind every hit of material params.see_through, the continuation's."""
        x0, y0, w, h = rect
        _check(lib.svo_trace_translucent(self._h, C.byref(cam), C.byref(params), x0, y0, w, h, surface_ptr, behind_ptr, stream),
               "svo_trace_translucent")

    def trace_local_shadows(self, cam: Camera, params: TraceParams, rect, gbuffer_ptr: int, point=None, spot=None, stream: int = 0):
        """svo_trace_local_shadows on the G-buffer svo_trace(cam, params, rect) filled: SHADOWED_POINT / SHADOWED_SPOT from one occlusion
        ray per hit towards `point` / `spot` (positions; None = that light keeps the record's SHADOWED), LOCAL_SHADOWS on every hit."""
        x0, y0, w, h = rect
        vec = [None if v is None else (C.c_float * 3)(*[float(c) for c in v]) for v in (point, spot)]
        _check(lib.svo_trace_local_shadows(self._h, C.byref(cam) if cam is not None else None, C.byref(params) if params is not None else None,
                                           vec[0], vec[1], x0, y0, w, h, gbuffer_ptr, stream), "svo_trace_local_shadows")

    def trace_lights(self, cam: Camera, params: TraceParams, rect, gbuffer_ptr: int, lights, visible_ptr: int, max_rays: int = 0, count_ptr: int = 0,
                     stream: int = 0):
        """svo_trace_lights on the G-buffer svo_trace(cam, params, rect) filled: one word per pixel into visible_ptr, bit j set where
        light j of `lights` (a sequence of Light) reaches the hit unoccluded.  max_rays: the capacity of the compacted ray list (0 = one
        slot per pixel); count_ptr: two uint32 on the device, (pairs, min(pairs, capacity))."""
        x0, y0, w, h = rect
        arr, n = light_array(lights)
        _check(lib.svo_trace_lights(self._h, C.byref(cam) if cam is not None else None, C.byref(params) if params is not None else None, arr, n,
                                    int(max_rays), x0, y0, w, h, gbuffer_ptr, visible_ptr, count_ptr or None, stream), "svo_trace_lights")

    def trace_instances(self, model: "World", cam: Camera, params: TraceParams, rect, gbuffer_ptr: int, instances, merged_ptr: int, owner_ptr: int,
                        max_rays: int = 0, count_ptr: int = 0, stream: int = 0):
        """svo_trace_instances with this world as the scene: up to 32 placements (a sequence of Instance) of the uploaded world `model`
        in front of the G-buffer svo_trace(cam, params, rect) filled.  merged_ptr gets w*h records (it may be gbuffer_ptr), owner_ptr w*h
        uint32 (0: the scene's pixel, j + 1: instance j's, whose ids belong to `model`).  max_rays: the capacity of the compacted ray
        list (0 = one slot per pixel); count_ptr: two uint32 on the device, (pairs, min(pairs, capacity))."""
        x0, y0, w, h = rect
        arr, n = instance_array(instances)
        _check(lib.svo_trace_instances(self._h, model._h if model is not None else None, C.byref(cam) if cam is not None else None,
                                       C.byref(params) if params is not None else None, arr, n, int(max_rays), x0, y0, w, h, gbuffer_ptr, merged_ptr,
                                       owner_ptr, count_ptr or None, stream), "svo_trace_instances")

    def trace_instance_shadows(self, model: "World", cam: Camera, params: TraceParams, rect, instances, merged_ptr: int, owner_ptr: int,
                               max_rays: int = 0, bias: float = 0.0, count_ptr: int = 0, stream: int = 0):
        """svo_trace_instance_shadows on what trace_instances wrote: SHADOW_TRACED, and SHADOWED where the way to the directional light
        is blocked by an instance or (for an instance's pixel) by this world, on every usable record not yet shadowed.  bias: how far
        the shadow ray starts in front of the hit (0 = the march's eps; a rotated instance wants a few eps, 1/256)."""
        x0, y0, w, h = rect
        arr, n = instance_array(instances)
        _check(lib.svo_trace_instance_shadows(self._h, model._h if model is not None else None, C.byref(cam) if cam is not None else None,
                                              C.byref(params) if params is not None else None, arr, n, int(max_rays), float(bias), x0, y0, w, h,
                                              merged_ptr, owner_ptr, count_ptr or None, stream), "svo_trace_instance_shadows")

    def shadowmap_fit(self, direction, width: int, height: int, smap: Optional[ShadowMap] = None) -> ShadowMap:
        """svo_shadowmap_fit: a map of width x height texels that holds the whole world box, seen along `direction`; depth_dev of
        `smap` (a new ShadowMap if None) is left as it is."""
        smap = ShadowMap() if smap is None else smap
        vec = None if direction is None else (C.c_float * 3)(*[float(c) for c in direction])
        _check(lib.svo_shadowmap_fit(self._h, vec, int(width), int(height), C.byref(smap)), "svo_shadowmap_fit")
        return smap

    def shadowmap_render(self, smap: ShadowMap, params: TraceParams, stream: int = 0):
        """svo_shadowmap_render: the world marched once from the light into smap.depth_dev (the march's t, +inf where nothing is hit)."""
        _check(lib.svo_shadowmap_render(self._h, C.byref(smap) if smap is not None else None, C.byref(params) if params is not None else None,
                                        stream), "svo_shadowmap_render")

    def tile_order(self, cost_ptr: int, order_ptr: int, ntiles: int, stream: int = 0):
        """svo_tile_order: tile indices by descending cost (of one frame) into order_ptr."""
        _check(lib.svo_tile_order(self._h, cost_ptr, order_ptr, ntiles, stream), "svo_tile_order")

    def prepare_light(self, light_dir=(1.0, -1.0, 0.0), stream: int = 0):
        """svo_world_prepare_light: decide, for every EMPTY node, whether its way to the light is clear; shadow rays of later camera
        launches with this light_dir end at such a node.  Asynchronous on `stream`; every change to the world drops the bits."""
        _check(lib.svo_world_prepare_light(self._h, (C.c_float * 3)(*[float(v) for v in light_dir]), stream), "svo_world_prepare_light")

    def prepared_light(self, stream: int = 0):
        """svo_world_prepared_light: (shadow direction the bits hold for - (0, 0, 0) if none -, EMPTY nodes found clear)."""
        sdir, n = (C.c_float * 3)(), C.c_uint64()
        _check(lib.svo_world_prepared_light(self._h, stream, sdir, C.byref(n)), "svo_world_prepared_light")
        return tuple(sdir), n.value

    def prepared_bricks(self, stream: int = 0) -> int:
        """svo_world_prepared_bricks: bricks that carry the clear flag (every empty cell has a clear way to the prepared light)."""
        n = C.c_uint64()
        _check(lib.svo_world_prepared_bricks(self._h, stream, C.byref(n)), "svo_world_prepared_bricks")
        return n.value

    def last_ray_count(self, stream: int = 0) -> int:
        n = C.c_uint64()
        _check(lib.svo_trace_last_ray_count(self._h, stream, C.byref(n)), "svo_trace_last_ray_count")
        return n.value

    # -- convenience: World::draw / chunkmarch returning numpy -------------------------------
    def draw(self, cam: Camera, rect=None, shadow: bool = False, kernel: int = KERNEL_AUTO, counters: bool = False,
             light_dir=(1.0, -1.0, 0.0), normal_mode: int = 0, semantics: int = 0, see_through: int = 0, local_shadows=None, shadowmap=None):
        """Trace a rectangle of the camera image; returns the G-buffer (HIT_DTYPE[h, w]) [+ counters].
        local_shadows=(point, spot): positions (or None) handed to trace_local_shadows behind the trace.
        shadowmap=(map, bias): a rendered ShadowMap applied behind the trace (shadowmap_apply) in place of shadow=True."""
        x0, y0, w, h = rect if rect is not None else (0, 0, cam.width, cam.height)
        out = DeviceBuffer(max(w * h, 1) * 32)
        cnt = DeviceBuffer(max(w * h, 1) * 16) if counters else None
        prm = trace_params(shadow=shadow, kernel=kernel, light_dir=light_dir, counters_dev=cnt.ptr if cnt else None, normal_mode=normal_mode,
                           semantics=semantics, see_through=see_through)
        if shadowmap is not None:
            prm.shadow = 0
        self.trace(cam, prm, (x0, y0, w, h), out.ptr)
        if shadowmap is not None:
            shadowmap_apply(cam, shadowmap[0], 1.0 / 4096.0 if semantics == SEMANTICS_GLSL else 0.0, shadowmap[1], (x0, y0, w, h), out.ptr)
        if local_shadows is not None:
            self.trace_local_shadows(cam, prm, (x0, y0, w, h), out.ptr, point=local_shadows[0], spot=local_shadows[1])
        _check(lib.svo_stream_synchronize(None), "svo_stream_synchronize")
        g = out.to_numpy(HIT_DTYPE, w * h).reshape(h, w)
        out.free()
        if counters:
            c = cnt.to_numpy(np.uint32, w * h * 4).reshape(h, w, 4)
            cnt.free()
            return g, c
        return g

    def draw_translucent(self, cam: Camera, see_through: int = 6, rect=None, shadow: bool = False, kernel: int = KERNEL_AUTO,
                         light_dir=(1.0, -1.0, 0.0), normal_mode: int = 0, semantics: int = 0):
        """svo_trace_translucent over a rectangle of the camera image; returns (surface, behind), HIT_DTYPE[h, w] each."""
        x0, y0, w, h = rect if rect is not None else (0, 0, cam.width, cam.height)
        surf, behind = DeviceBuffer(max(w * h, 1) * 32), DeviceBuffer(max(w * h, 1) * 32)
        prm = trace_params(shadow=shadow, kernel=kernel, light_dir=light_dir, normal_mode=normal_mode, semantics=semantics,
                           see_through=see_through)
        self.trace_translucent(cam, prm, (x0, y0, w, h), surf.ptr, behind.ptr)
        _check(lib.svo_stream_synchronize(None), "svo_stream_synchronize")
        s, b = surf.to_numpy(HIT_DTYPE, w * h).reshape(h, w), behind.to_numpy(HIT_DTYPE, w * h).reshape(h, w)
        surf.free()
        behind.free()
        return s, b

    def chunkmarch(self, origins, dirs, shadow: bool = False, kernel: int = KERNEL_AUTO, counters: bool = False,
                   light_dir=(1.0, -1.0, 0.0), eps: float = 0.0, caps=(0, 0, 0), normal_mode: int = 0, semantics: int = 0,
                   see_through: int = 0, tmax=None):
        """chunkmarch over a ray list (src/Traverse.cpp:127-171); returns HIT_DTYPE[n] [+ counters].
        tmax: a far end per ray (a scalar or [n] floats): the rays are marched as segments (svo_trace_segments)."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        od, dd = DeviceBuffer.from_numpy(o), DeviceBuffer.from_numpy(d)
        td = None if tmax is None else DeviceBuffer.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, dtype=np.float32), (n,))))
        out = DeviceBuffer(max(n, 1) * 32)
        cnt = DeviceBuffer(max(n, 1) * 16) if counters else None
        prm = trace_params(shadow=shadow, kernel=kernel, light_dir=light_dir, eps=eps, caps=caps,
                           counters_dev=cnt.ptr if cnt else None, normal_mode=normal_mode, semantics=semantics, see_through=see_through)
        if td is None:
            self.trace_rays(od.ptr, dd.ptr, n, prm, out.ptr)
        else:
            self.trace_segments(od.ptr, dd.ptr, td.ptr, n, prm, out.ptr)
        _check(lib.svo_stream_synchronize(None), "svo_stream_synchronize")
        g = out.to_numpy(HIT_DTYPE, n)
        for b in (od, dd, out) + (() if td is None else (td,)):
            b.free()
        if counters:
            c = cnt.to_numpy(np.uint32, n * 4).reshape(n, 4)
            cnt.free()
            return g, c
        return g

    def locate_points(self, points, kernel: int = KERNEL_AUTO, semantics: int = 0, see_through: int = 0):
        """traverse (src/Traverse.cpp:34-48) and twigmarch's cell lookup over a point list; returns VOXEL_DTYPE[n]."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = p.shape[0]
        pd, out = DeviceBuffer.from_numpy(p), DeviceBuffer(max(n, 1) * 32)
        self.locate(pd.ptr, n, trace_params(kernel=kernel, semantics=semantics, see_through=see_through), out.ptr)
        _check(lib.svo_stream_synchronize(None), "svo_stream_synchronize")
        v = out.to_numpy(VOXEL_DTYPE, n)
        pd.free()
        out.free()
        return v

    def hit_boxes(self, records):
        """World.hit_voxels over host records (HIT_DTYPE, any shape); returns VOXEL_DTYPE[n]."""
        g = np.ascontiguousarray(records, dtype=HIT_DTYPE).reshape(-1)
        n = g.shape[0]
        gd, out = DeviceBuffer.from_numpy(g), DeviceBuffer(max(n, 1) * 32)
        self.hit_voxels(gd.ptr, n, out.ptr)
        _check(lib.svo_stream_synchronize(None), "svo_stream_synchronize")
        v = out.to_numpy(VOXEL_DTYPE, n)
        gd.free()
        out.free()
        return v

    def ao_image(self, cam: Camera, records, rect=None, voxels=None, cell: float = 0.0, kernel: int = KERNEL_AUTO, semantics: int = 0,
                 see_through: int = 0, eps: float = 0.0):
        """World.hit_ao over host records (HIT_DTYPE[h, w], as World.draw(cam, rect) returns them); voxels: their VOXEL_DTYPE records
        (None = hit_voxels').  Returns float32[h, w]."""
        x0, y0, w, h = rect if rect is not None else (0, 0, cam.width, cam.height)
        g = np.ascontiguousarray(records, dtype=HIT_DTYPE).reshape(-1)
        n = w * h
        assert g.shape[0] == n
        gd, vd, out = DeviceBuffer.from_numpy(g), DeviceBuffer(max(n, 1) * 32), DeviceBuffer(max(n, 1) * 4)
        try:
            if voxels is None:
                self.hit_voxels(gd.ptr, n, vd.ptr)
            elif n:
                v = np.ascontiguousarray(voxels, dtype=VOXEL_DTYPE).reshape(-1)
                assert v.shape[0] == n
                _check(lib.svo_memcpy_h2d(vd.ptr, v.ctypes.data, v.nbytes), "svo_memcpy_h2d")
            self.hit_ao(cam, trace_params(kernel=kernel, semantics=semantics, see_through=see_through, eps=eps), (x0, y0, w, h),
                        gd.ptr, vd.ptr, out.ptr, cell=cell)
            _check(lib.svo_stream_synchronize(None), "svo_stream_synchronize")
            return out.to_numpy(np.float32, n).reshape(h, w)
        finally:
            for b in (gd, vd, out):
                b.free()

    def reflect_image(self, cam: Camera, records, rect=None, voxels=None, material: int = 0, shadow: bool = False, kernel: int = KERNEL_AUTO,
                      semantics: int = 0, see_through: int = 0, eps: float = 0.0, light_dir=(1.0, -1.0, 0.0), normal_mode: int = 0):
        """World.trace_reflections over host records (HIT_DTYPE[h, w], as World.draw(cam, rect) returns them); voxels: their VOXEL_DTYPE
        records (None = hit_voxels').  Returns HIT_DTYPE[h, w]."""
        x0, y0, w, h = rect if rect is not None else (0, 0, cam.width, cam.height)
        g = np.ascontiguousarray(records, dtype=HIT_DTYPE).reshape(-1)
        n = w * h
        assert g.shape[0] == n
        gd, vd, out = DeviceBuffer.from_numpy(g), DeviceBuffer(max(n, 1) * 32), DeviceBuffer(max(n, 1) * 32)
        try:
            if voxels is None:
                self.hit_voxels(gd.ptr, n, vd.ptr)
            elif n:
                v = np.ascontiguousarray(voxels, dtype=VOXEL_DTYPE).reshape(-1)
                assert v.shape[0] == n
                _check(lib.svo_memcpy_h2d(vd.ptr, v.ctypes.data, v.nbytes), "svo_memcpy_h2d")
            prm = trace_params(shadow=shadow, kernel=kernel, semantics=semantics, see_through=see_through, eps=eps, light_dir=light_dir,
                               normal_mode=normal_mode)
            self.trace_reflections(cam, prm, (x0, y0, w, h), gd.ptr, vd.ptr, out.ptr, material=material)
            _check(lib.svo_stream_synchronize(None), "svo_stream_synchronize")
            return out.to_numpy(HIT_DTYPE, n).reshape(h, w)
        finally:
            for b in (gd, vd, out):
                b.free()

"""The C-ABI library: exports exactly what include/svo.h declares, validates input, mirrors World::index*,
and fails loudly (error codes, never a CPU fallback) when no HIP device is present.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    text = open(os.path.join(ROOT, "include", "svo.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(svo_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(svo):
    names = header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(svo.lib, n), f"{n} declared in include/svo.h but not exported"
    assert sorted(svo.ABI_SYMBOLS) == names
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" T (svo_[a-z0-9_]+)$", out, flags=re.M)))
    assert exported == names, "exported svo_* symbols differ from the header"
    assert svo.lib.svo_abi_version() == 4


def test_struct_layouts_match_the_header(svo, tmp_path):
    assert C.sizeof(svo.ChunkDesc) == 56 and C.sizeof(svo.Camera) == 64 and C.sizeof(svo.TraceParams) == 80
    assert C.sizeof(svo.TerrainParams) == 68 and svo.HIT_DTYPE.itemsize == 32
    # compile a C translation unit against the header and print the same sizes
    src = r'''#include "svo.h"
#include <stdio.h>
int main(void){printf("%zu %zu %zu %zu %zu %zu\n",sizeof(svo_chunk_desc),sizeof(svo_camera),sizeof(svo_trace_params),sizeof(svo_terrain_params),sizeof(svo_hit),sizeof(svo_world_info));return 0;}'''
    exe = str(tmp_path / "svo_abi_sizes")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src, text=True, check=True)
    sizes = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(svo.ChunkDesc), C.sizeof(svo.Camera), C.sizeof(svo.TraceParams), C.sizeof(svo.TerrainParams), 32, C.sizeof(svo.WorldInfo)]


def _chunk(tree, twig=(), depth=4, pos=(0, 0, 0), size=128.0):
    return dict(position=pos, size=size, depth=depth, tree=np.array(tree, np.uint32), twig=np.array(twig, np.uint16))


B, T, L = 2 << 30, 3 << 30, 1 << 30


@pytest.mark.parametrize("tree,twig,why", [
    ([B | 9], (), "offset outside pool"),
    ([B | 1] + [0] * 8 + [0], (), "pool not 1+8k"),
    ([B | 1] + [B | 1] + [0] * 7, (), "back edge / cycle"),
    ([B | 2] + [0] * 16, (), "child block not at 1+8k"),
    ([T | 0], (), "TWIG without bricks"),
    ([B | 1] + [B | 9] + [0] * 7 + [B | 17] + [0] * 7 + [0] * 8, (), "BRANCH below level depth-2"),
])
def test_malformed_trees_are_rejected(svo, tree, twig, why):
    with pytest.raises(svo.SvoError) as e:
        svo.World.create([_chunk(tree, twig, depth=4)], 1, 1, 1, 128)
    assert e.value.code == -4, why


def test_bad_arguments(svo):
    with pytest.raises(svo.SvoError) as e:
        svo.World.create([_chunk([0])], 2, 1, 1, 128)             # n != w*h*d
    assert e.value.code == -1
    with pytest.raises(svo.SvoError):
        svo.World.generate(1, 1, 1, 128, 1)                         # depth < TWIG_LEVELS
    with pytest.raises(svo.SvoError):
        svo.World.generate(1, 1, 1, 128, 6, pyramid_resolution=48)  # not a power of two


def test_create_roundtrip_and_orphans(svo):
    """Orphaned blocks (left behind by Ocroot::destroy) are tolerated; pools are copied."""
    tree = [B | 1] + [L | 3, 0, 0, 0, 0, 0, 0, 0] + [B | 1] * 8     # second block is unreferenced garbage
    W = svo.World.create([_chunk(tree, depth=4)], 1, 1, 1, 128)
    c = W.chunk(0)
    assert np.array_equal(c["tree"], np.array(tree, np.uint32)) and c["depth"] == 4
    assert W.info.exact_geometry == 1
    W.destroy()
    W = svo.World.create([_chunk([L | 1], size=100.0)], 1, 1, 1, 100)
    assert W.info.exact_geometry == 0                               # 100 is not a power of two
    W.destroy()


def test_index_and_index_float_match_oracle(svo, oracle):
    W = svo.World.generate(3, 2, 2, 128, 3, chunkcoordmin=(-2, -1, 0))
    chunks = [W.chunk(i) for i in range(12)]
    O = oracle.OracleWorld.from_chunks(chunks, 3, 2, 2, 128, (-2, -1, 0))
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.uniform(-700, 700, (500, 3)), rng.integers(-5, 5, (200, 3)) * 128.0]).astype(np.float32)
    q = (C.c_int * 3)()
    for p in pts:
        mine = W.index_float(p)
        oracle.lib.orc_world_index_float(C.byref(O.w), oracle.vec3(p), q)
        assert mine == tuple(q)
        assert W.index(*mine) == oracle.lib.orc_world_index3(C.byref(O.w), *mine)
    # chunk placement: chunk at grid coordinate (cx,cy,cz) sits at index(cx,cy,cz)
    for cx in range(-2, 1):
        for cy in range(-1, 1):
            for cz in range(0, 2):
                c = W.chunk(W.index(cx, cy, cz))
                assert c["position"] == (cx * 128.0, cy * 128.0, cz * 128.0)
    W.destroy()


def test_no_device_means_error_not_fallback(svo):
    """In the CPU container there is no HIP device: every device entry point must fail loudly."""
    if svo.device_count() > 0:
        pytest.skip("a HIP device is present")
    W = svo.World.generate(1, 1, 1, 128, 4)
    with pytest.raises(svo.SvoError) as e:
        W.upload(0)
    assert e.value.code == -2
    cam = svo.default_camera(1, 1, 128, 8, 8)
    with pytest.raises(svo.SvoError) as e:
        W.trace(cam, svo.trace_params(), (0, 0, 8, 8), 0)
    assert e.value.code == -5                                        # not uploaded: nothing was traced on the CPU
    with pytest.raises(svo.SvoError) as e:
        W.edit_box(0, svo.EDIT_BUILD, (0, 0, 0), (8, 8, 8), 5)
    assert e.value.code == -5                                        # ... and nothing is edited on the host behind the caller's back
    with pytest.raises(svo.SvoError) as e:
        svo.World.generate(1, 1, 1, 128, 4, build_device=0)
    assert e.value.code == -2                                        # the device builder does not fall back to the host generator
    W.destroy()


def test_product_does_not_link_the_oracle(svo):
    out = subprocess.run(["ldd", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "oracle" not in out
    syms = subprocess.run(["nm", "-D", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "orc_" not in syms
    pkg = os.path.join(ROOT, "octree-raymarcher_amd")
    for dirpath, _, files in os.walk(pkg):
        if "/build" in dirpath:
            continue
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "oracle_binding" not in text and "svo_oracle" not in text, f"{f} references the oracle"


def test_argument_validation_precedes_any_device_work(svo):
    """Bad arguments are rejected with SVO_ERR_INVALID_ARG before HIP is touched (works without a GPU)."""
    cam = svo.default_camera(1, 1, 128, 16, 16)
    P = svo.shade_defaults()
    with pytest.raises(svo.SvoError) as e:
        svo.shade(cam, P, (0, 0, 16, 16), 0, 0)                      # null buffers
    assert e.value.code == -1
    with pytest.raises(svo.SvoError) as e:
        svo.gbuffer_pack(0, 0, 10)
    assert e.value.code == -1
    svo.gbuffer_pack(0, 0, 0)                                         # n = 0 is a no-op
    with pytest.raises(svo.SvoError) as e:
        svo.gbuffer_unpack(0, 0, -1)
    assert e.value.code == -1
    # a rectangle or a count whose grid of 256-thread blocks does not fit one launch: SVO_ERR_UNSUPPORTED, behind the argument check
    # and before any launch (the dummy pointers are never dereferenced)
    huge, big_n, ptr = (0, 0, 1 << 20, 1 << 20), 1 << 40, 0x1000
    atlas = svo.Atlas(ptr, None, 4, 4)
    shades = {"shade": lambda g, out: svo.shade(cam, P, huge, g, out),
              "shade_packed": lambda g, out: svo.shade_packed(cam, P, huge, g, out),
              "shade_translucent": lambda g, out: svo.shade_translucent(cam, P, huge, g, ptr, out),
              "shade_textured": lambda g, out: svo.shade_textured(cam, P, atlas, huge, g, ptr, out)}
    for name, call in shades.items():
        with pytest.raises(svo.SvoError) as e:
            call(ptr, ptr)
        assert e.value.code == -6, name
        for g, out in ((0, ptr), (ptr, 0)):
            with pytest.raises(svo.SvoError) as e:
                call(g, out)
            assert e.value.code == -1, name
    for call in (svo.gbuffer_pack, svo.gbuffer_unpack):
        with pytest.raises(svo.SvoError) as e:
            call(ptr, ptr, big_n)
        assert e.value.code == -6
        for a, b in ((0, ptr), (ptr, 0)):
            with pytest.raises(svo.SvoError) as e:
                call(a, b, big_n)
            assert e.value.code == -1
    # defaults mirror src/Main.cpp:101-131 and the ML table
    assert tuple(P.point.position) == (50.0, 8.0, 65.0) and abs(P.spot.cos_phi - np.cos(np.radians(25.0))) < 1e-7
    assert P.materials[4].shininess == 10000.0 and tuple(P.materials[6].specular) == (1.0, 1.0, 1.0)
    assert P.eps == np.float32(1 / 8192) and P.near_plane == 0.125 and P.far_plane == 8192.0


def test_stack_kernel_register_budget(tmp_path):
    """The stack kernel is budgeted for six waves per SIMD (+9 %): hipcc must fit every instantiation
    into 80 VGPRs, and the hand-written step (csrc/step_asm.hip.h, one asm statement) must be what it compiles - a change that
    silently drops the kernel to five waves, or the build to the C++ step, fails here, on the CPU (hipcc cross-compiles)."""
    import re
    pkg = os.path.join(ROOT, "octree-raymarcher_amd")
    audit = str(tmp_path / "svo_device_audit.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                        "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", "-o", audit,
                        os.path.join(pkg, "csrc", "device.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.findall(r"Function Name: (\S*k_trace_stack\S*).*?VGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", r.stderr, re.S)
    assert len(blocks) >= 4, "one instantiation per wide-level count"
    for name, vgprs, occ in blocks:
        assert int(vgprs) <= 80 and int(occ) >= 6, (name, vgprs, occ)
    asm = open(audit).read()
    body = asm[asm.index("k_trace_stackILi10E"):]
    assert "v_cmpx_ge_f32" in body and ";;#ASMSTART" in body, "the hand-scheduled step is compiled in"

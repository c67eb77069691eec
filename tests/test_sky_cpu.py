"""svo_shade_sky / svo_frame_rgba8 without a device: the C ABI surface, the argument checks that are settled before any device work,
known answers of the host model (tests/sky_model.py), its float32 statement against a plain float64 cube-map lookup, and - with the
CPU oracle - what the cameras of tests/test_sky.py see.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sky_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ("svo_shade_sky", "svo_frame_rgba8")


def test_new_symbols_are_declared_exported_and_sized(svo, tmp_path):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+svo_shade_sky\s*\(\s*const svo_camera\s*\*\s*cam\s*,\s*const svo_sky\s*\*\s*sky\s*,\s*int x0\s*,\s*int y0\s*,\s*int w\s*,\s*int h\s*,"
                     r"\s*const svo_hit\s*\*\s*gbuffer_dev\s*,\s*const uint64_t\s*\*\s*packed_dev\s*,\s*float\s*\*\s*rgba_dev\s*,\s*void\s*\*\s*stream\s*\)", header)
    assert re.search(r"\bint\s+svo_frame_rgba8\s*\(\s*const float\s*\*\s*rgba_dev\s*,\s*int64_t n\s*,\s*uint32_t\s*\*\s*out_dev\s*,\s*void\s*\*\s*stream\s*\)", header)
    assert re.search(r"typedef struct svo_sky\s*\{\s*const uint8_t\s*\*\s*faces_dev\[6\];\s*int32_t size;\s*int32_t filter;\s*\}\s*svo_sky;", header)
    assert re.search(r"enum\s*\{\s*SVO_SKY_LINEAR = 0\s*,\s*SVO_SKY_NEAREST = 1\s*\}", header)
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in svo.ABI_SYMBOLS and hasattr(svo.lib, name)
        assert re.search(rf" T {name}$", out, flags=re.M)
    # functions added, nothing changed
    assert "#define SVO_ABI_VERSION 4" in header and svo.lib.svo_abi_version() == 4
    src = r'''#include "svo.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %zu %zu %d %d\n",sizeof(svo_sky),offsetof(svo_sky,faces_dev),sizeof(((svo_sky*)0)->faces_dev),
offsetof(svo_sky,size),offsetof(svo_sky,filter),sizeof(svo_hit),(int)SVO_SKY_LINEAR,(int)SVO_SKY_NEAREST);return 0;}'''
    exe = str(tmp_path / "svo_sky_size")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [56, 0, 48, 48, 52, 32, 0, 1]
    assert [C.sizeof(svo.Sky), svo.Sky.faces_dev.offset, svo.Sky.faces_dev.size, svo.Sky.size.offset, svo.Sky.filter.offset] == got[:5]
    assert (svo.SKY_LINEAR, svo.SKY_NEAREST) == (0, 1) == (S.LINEAR, S.NEAREST)


def test_argument_checks_precede_any_device_work(svo):
    fake = 256                                                  # never dereferenced: every call below fails before device work
    cam = svo.default_camera(1, 1, 128, 16, 16)
    rect = (0, 0, 16, 16)
    sky = svo.Sky([fake] * 6, 8, svo.SKY_LINEAR)
    assert list(sky.faces_dev) == [fake] * 6 and sky.size == 8 and sky.filter == 0

    def code(fn, *args, **kw):
        with pytest.raises(svo.SvoError) as e:
            fn(*args, **kw)
        return e.value.code

    assert code(svo.shade_sky, None, sky, rect, fake, gbuffer_ptr=fake) == -1
    assert code(svo.shade_sky, cam, None, rect, fake, gbuffer_ptr=fake) == -1
    assert code(svo.shade_sky, cam, sky, rect, None, gbuffer_ptr=fake) == -1
    for f in range(6):                                          # a NULL face pointer, each of the six
        faces = [fake] * 6
        faces[f] = None
        assert code(svo.shade_sky, cam, svo.Sky(faces, 8), rect, fake, gbuffer_ptr=fake) == -1
    assert code(svo.shade_sky, cam, svo.Sky([fake] * 6, 0), rect, fake, gbuffer_ptr=fake) == -1
    assert code(svo.shade_sky, cam, svo.Sky([fake] * 6, -3), rect, fake, packed_ptr=fake) == -1
    assert code(svo.shade_sky, cam, svo.Sky([fake] * 6, 8, 2), rect, fake, gbuffer_ptr=fake) == -1
    assert code(svo.shade_sky, cam, svo.Sky([fake] * 6, 8, -1), rect, fake, gbuffer_ptr=fake) == -1
    assert code(svo.shade_sky, cam, sky, rect, fake, gbuffer_ptr=fake, packed_ptr=fake) == -1      # both record pointers
    assert code(svo.shade_sky, cam, sky, rect, fake) == -1                                         # neither
    for bad in ((0, 0, -1, 16), (0, 0, 16, -1), (-1, 0, 16, 16), (0, -1, 16, 16)):
        assert code(svo.shade_sky, cam, sky, bad, fake, gbuffer_ptr=fake) == -1
    for wh in ((0, 16), (16, 0), (-4, 16)):
        blind = svo.default_camera(1, 1, 128, 16, 16)
        blind.width, blind.height = wh
        assert code(svo.shade_sky, blind, sky, rect, fake, packed_ptr=fake) == -1
    # a bad argument is refused on an empty rectangle too; a good empty rectangle launches nothing
    assert code(svo.shade_sky, cam, sky, (0, 0, 0, 16), fake) == -1
    svo.shade_sky(cam, sky, (0, 0, 0, 16), fake, gbuffer_ptr=fake)
    svo.shade_sky(cam, svo.Sky([fake] * 6, 8, svo.SKY_NEAREST), (3, 5, 16, 0), fake, packed_ptr=fake)
    # svo_frame_rgba8
    assert code(svo.frame_rgba8, fake, -1, fake) == -1
    assert code(svo.frame_rgba8, None, 8, fake) == -1
    assert code(svo.frame_rgba8, fake, 8, None) == -1
    assert code(svo.frame_rgba8, None, -1, None) == -1
    svo.frame_rgba8(None, 0, None)
    svo.frame_rgba8(fake, 0, fake)


def test_axis_directions_land_on_the_centre_texel_of_their_face():
    d = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F) * F(3.5)
    faces = S.identity_faces(255)                               # odd: texel 127 is the centre one
    face, s, t = S.face_coords(d)
    assert list(face) == [0, 1, 2, 3, 4, 5] and np.all(s == F(0.5)) and np.all(t == F(0.5))
    rgb, _ = S.lookup(d, faces, S.NEAREST)
    assert np.array_equal(np.round(rgb.astype(np.float64) * 255).astype(int), [[127, 127, f] for f in range(6)])
    rgb, _ = S.lookup(d, faces, S.LINEAR)                       # u = 127.0 exactly: the texel's centre, weight 0 for its neighbours
    assert np.array_equal(rgb, (np.array([[127, 127, f] for f in range(6)], F) / F(255)))
    # off the axis the coordinates move as the OpenGL table says: on +X s falls with z and t with y, on +Y t rises with z, ...
    probe = {0: ((1, 0, .5), (.25, .5)), 1: ((-1, .5, 0), (.5, .25)), 2: ((.5, 1, 0), (.75, .5)), 3: ((0, -1, .5), (.5, .25)),
             4: ((.5, .5, 1), (.75, .25)), 5: ((.5, 0, -1), (.25, .5))}
    for f, (direction, want) in probe.items():
        face, s, t = S.face_coords(np.array([direction], F))
        assert (int(face[0]), float(s[0]), float(t[0])) == (f,) + want
    # zero and NaN directions are left alone
    face, _, _ = S.face_coords(np.array([[0, 0, 0], [np.nan, np.nan, np.nan], [-0.0, 0, 0]], F))
    assert list(face) == [-1, -1, -1]


def random_directions(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


@pytest.mark.parametrize("filter", [S.LINEAR, S.NEAREST], ids=["linear", "nearest"])
def test_flat_faces_return_their_byte(filter):
    d = random_directions(10000, 11)
    faces = np.stack([np.full((5, 5, 3), 40 * f + 10, np.uint8) for f in range(6)])
    rgb, face = S.lookup(d, faces, filter)
    assert np.bincount(face, minlength=6).min() > 1000
    want = (F(40) * face.astype(F) + F(10)) / F(255)
    assert np.array_equal(rgb, np.repeat(want[:, None], 3, axis=1))


def test_x_wins_where_the_three_magnitudes_meet():
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                face, _, _ = S.face_coords(np.array([[sx, sy, sz]], F) * F(0.57735026))
                assert face[0] == (0 if sx > 0 else 1)
    face, _, _ = S.face_coords(np.array([[0, 2, 2], [0, -2, 2], [1, 1, 0], [1, 0, -1]], F))
    assert list(face) == [2, 3, 0, 0]                           # Y before Z, X before either


def test_float32_and_float64_lookups_agree():
    """Sizes 1, 2 and 3: s carries at most 2^-24 of rounding, u = s * size one more half ulp of a value below 4 (2^-23 at most), so each
    of the two weights is off by less than 3.1e-7 and the colour, whose texel differences are at most 1, by less than 6.2e-7 plus the
    four roundings of the lerps and the decode (6e-8 each): under the 1e-6 asked for.  The face never differs: both compare the same
    float32 magnitudes."""
    d = random_directions(4000, 12)
    worst = 0.0
    for size in (1, 2, 3):
        faces = S.random_faces(size, 100 + size)
        got, face = S.lookup(d, faces, S.LINEAR)
        want = S.lookup64(d, faces, S.LINEAR)
        assert np.all(face >= 0)
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
    print(f"float32 against float64 lookup: {worst:.3e}")
    assert worst <= 1e-6
    # nearest: the same texel except within rounding of a texel boundary
    faces = S.random_faces(3, 7)
    got, _ = S.lookup(d, faces, S.NEAREST)
    same = np.all(np.abs(got.astype(np.float64) - S.lookup64(d, faces, S.NEAREST)) <= 1e-6, axis=1)
    assert same.mean() > 0.999


def test_rgba8_model_known_answers():
    def one(c):
        return int(S.frame_rgba8(np.array([[c, c, c, 0.5]], F))[0, 0])

    assert [one(c) for c in (np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, 1.0, S.ulp(1.0, 1), S.ulp(1.0, -1), 2.0)] == [0, 255, 0, 0, 0, 0, 255, 255, 255, 255]
    assert np.array_equal(S.frame_rgba8(np.array([[0.2, np.nan, 7.0, -3.0]], F)), [[51, 0, 255, 255]])      # alpha 255 whatever the depth
    # every value against exact rational arithmetic on the float32 operations, done in float64 (c * 255 is exact in float64; the sum
    # is rounded to float32 by one explicit step)
    x = S.rgba8_inputs()
    got = S.frame_rgba8(x)
    assert np.all(got[:, 3] == 255)
    c = x[:, :3].astype(np.float64)
    with np.errstate(all="ignore"):
        prod = (c * 255.0).astype(F).astype(np.float64)
    with np.errstate(all="ignore"):
        want = np.where(np.isnan(c) | (c <= 0), 0, np.where(c >= 1, 255, np.floor((prod + 0.5).astype(F).astype(np.float64))))
    assert np.array_equal(got[:, :3], want.astype(np.uint8))
    for k in range(256):                                        # k / 255 converts back to k, and the half-way point rounds about there
        assert one(F(k) / F(255)) == k
        assert one((F(k) + F(0.5)) / F(255)) in (k, min(k + 1, 255))
    assert len(np.unique(got[:, 0])) == 256


def test_the_cameras_see_what_the_gpu_tests_rest_on(svo, oracle):
    """The all-sky views hit nothing; each cube face is named by at least 50 sky pixels; and at least one of the two mixed views has at
    least 300 hit and 300 miss pixels - all by the CPU oracle."""
    w, h, d, cs, ccm, _, _ = S.WORLDS[S.WORLD]
    import hit_voxels_model as M
    O = oracle.OracleWorld.from_chunks(M.make_chunks(svo, S.WORLD), w, h, d, cs, ccm)
    named = np.zeros(6, np.int64)
    mixed = []
    for name, (cam, all_sky, semantics) in S.all_cameras(svo).items():
        g = O.trace_image(cam, params=oracle.make_params(semantics=semantics))
        g = (g[0] if isinstance(g, tuple) else g).reshape(-1)
        hit = (g["flags"] & 1) != 0
        face, _, _ = S.face_coords(S.camera_dirs(cam))
        assert np.all(face >= 0)
        named += np.bincount(face[~hit], minlength=6)
        print(f"{name}: {int(hit.sum())} hits, {int((~hit).sum())} misses, faces of the misses {np.bincount(face[~hit], minlength=6)}")
        if all_sky:
            assert not hit.any(), f"{name}: an all-sky view hits the world"
        else:
            mixed.append(min(int(hit.sum()), int((~hit).sum())))
    O.close()
    assert named.min() >= 50, named
    assert len(mixed) == 2 and max(mixed) >= 300, mixed
    # the corner view holds the pixels where the major axis changes: three faces, each a third of it
    face, _, _ = S.face_coords(S.camera_dirs(S.sky_cameras(svo)["corner"]))
    assert sorted(np.unique(face)) == [0, 2, 4] and np.bincount(face).max() < 1200

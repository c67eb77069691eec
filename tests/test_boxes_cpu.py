"""svo_cursor_place / svo_shade_boxes / svo_world_edit_cube without a device: the C ABI surface, the argument checks that are settled
before any device work, hand-derived answers of the host model (tests/boxes_model.py), the corner rule against World::index /
index_float of the library, the condition the "once per distinct chunk" rule rests on (a repeated edit leaves the pools as they are,
by the CPU oracle), and what the box placement of tests/test_boxes.py provides.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import boxes_model as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ("svo_cursor_place", "svo_shade_boxes", "svo_world_edit_cube")
UNIT = dict(bmin=(0.0, 0.0, 0.0), size=1.0)
GREY = (0.8, 0.8, 0.8)


def ulp(x, k):
    return (np.array([x], F).view(np.int32) + np.int32(k)).view(F)[0]


def test_new_symbols_are_declared_exported_and_sized(svo, tmp_path):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+svo_cursor_place\s*\(\s*const float origin\[3\]\s*,\s*const float dir\[3\]\s*,\s*const svo_hit\s*\*\s*record_dev\s*,"
                     r"\s*float size\s*,\s*svo_box\s*\*\s*box_dev\s*,\s*void\s*\*\s*stream\s*\)", header)
    assert re.search(r"\bint\s+svo_shade_boxes\s*\(\s*const svo_camera\s*\*\s*cam\s*,\s*const svo_box\s*\*\s*boxes_dev\s*,\s*int nboxes\s*,\s*float near_plane\s*,"
                     r"\s*float far_plane\s*,\s*int x0\s*,\s*int y0\s*,\s*int w\s*,\s*int h\s*,\s*float\s*\*\s*rgba_dev\s*,\s*void\s*\*\s*stream\s*\)", header)
    assert re.search(r"\bint\s+svo_world_edit_cube\s*\(\s*svo_world\s*\*\s*,\s*int op\s*,\s*const float bmin\[3\]\s*,\s*float size\s*,\s*uint16_t material\s*,"
                     r"\s*int chunks_out\[8\]\s*,\s*int\s*\*\s*nchunks_out\s*\)", header)
    assert re.search(r"enum\s*\{\s*SVO_BOX_SOLID = 0\s*,\s*SVO_BOX_CURSOR = 1\s*,\s*SVO_BOX_HIDDEN = 1u << 8\s*\}", header)
    out = subprocess.run(["nm", "-D", "--defined-only", svo.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in svo.ABI_SYMBOLS and hasattr(svo.lib, name)
        assert re.search(rf" T {name}$", out, flags=re.M)
    assert "#define SVO_ABI_VERSION 4" in header and svo.lib.svo_abi_version() == 4      # functions added, nothing changed
    src = r'''#include "svo.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %zu\n",sizeof(svo_box),offsetof(svo_box,bmin),offsetof(svo_box,size),offsetof(svo_box,color),
offsetof(svo_box,alpha),offsetof(svo_box,style),offsetof(svo_box,_pad),(int)SVO_BOX_SOLID,(int)SVO_BOX_CURSOR,(int)SVO_BOX_HIDDEN,(int)SVO_MAX_BOXES,sizeof(svo_hit));return 0;}'''
    exe = str(tmp_path / "svo_box_size")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [48, 0, 12, 16, 28, 32, 36, 0, 1, 256, 64, 32]
    X = svo.Box
    assert [C.sizeof(X), X.bmin.offset, X.size.offset, X.color.offset, X.alpha.offset, X.style.offset, X._pad.offset] == got[:7]
    for dt in (svo.BOX_DTYPE, B.BOX_DTYPE):
        assert [dt.itemsize] + [dt.fields[k][1] for k in ("bmin", "size", "color", "alpha", "style", "_pad")] == got[:7]
    assert (svo.BOX_SOLID, svo.BOX_CURSOR, svo.BOX_HIDDEN, svo.MAX_BOXES) == (0, 1, 256, 64) == (B.SOLID, B.CURSOR, B.HIDDEN, B.MAX_BOXES)


def test_argument_checks_precede_any_device_work(svo):
    fake = 256                                                  # never dereferenced: every call below ends before device work
    cam = svo.default_camera(1, 1, 128, 16, 16)
    rect = (0, 0, 16, 16)

    def code(fn, *args, **kw):
        with pytest.raises(svo.SvoError) as e:
            fn(*args, **kw)
        return e.value.code

    # svo_cursor_place
    o, d = (1.0, 2.0, 3.0), (0.0, 0.0, 1.0)
    assert code(svo.cursor_place, None, d, fake, 4.0, fake) == -1
    assert code(svo.cursor_place, o, None, fake, 4.0, fake) == -1
    assert code(svo.cursor_place, o, d, None, 4.0, fake) == -1
    assert code(svo.cursor_place, o, d, fake, 4.0, None) == -1
    for size in (0.0, -1.0, float("nan")):
        assert code(svo.cursor_place, o, d, fake, size, fake) == -1
    # svo_shade_boxes
    assert code(svo.shade_boxes, None, fake, 1, rect, fake) == -1
    assert code(svo.shade_boxes, cam, fake, 1, rect, None) == -1
    assert code(svo.shade_boxes, cam, None, 1, rect, fake) == -1
    assert code(svo.shade_boxes, cam, fake, -1, rect, fake) == -1
    assert code(svo.shade_boxes, cam, fake, svo.MAX_BOXES + 1, rect, fake) == -1
    for bad in ((0, 0, -1, 16), (0, 0, 16, -1), (-1, 0, 16, 16), (0, -1, 16, 16)):
        assert code(svo.shade_boxes, cam, fake, 1, bad, fake) == -1
    for wh in ((0, 16), (16, 0), (-4, 16)):
        blind = svo.default_camera(1, 1, 128, 16, 16)
        blind.width, blind.height = wh
        assert code(svo.shade_boxes, blind, fake, 1, rect, fake) == -1
    assert code(svo.shade_boxes, cam, fake, 1, rect, fake, near_plane=-0.125) == -1
    assert code(svo.shade_boxes, cam, fake, 1, rect, fake, far_plane=-1.0) == -1
    assert code(svo.shade_boxes, cam, fake, 1, rect, fake, near_plane=float("nan")) == -1
    # a bad argument is refused with nothing to draw too; nothing to draw launches nothing
    assert code(svo.shade_boxes, cam, fake, 0, rect, None) == -1
    assert code(svo.shade_boxes, None, None, 0, (0, 0, 0, 16), fake) == -1
    svo.shade_boxes(cam, None, 0, rect, fake)
    svo.shade_boxes(cam, fake, 0, rect, fake)
    svo.shade_boxes(cam, fake, svo.MAX_BOXES, (0, 0, 0, 16), fake)
    svo.shade_boxes(cam, fake, 3, (3, 5, 16, 0), fake, near_plane=0.5, far_plane=100.0)


def test_edit_cube_argument_checks_leave_their_outputs_alone(svo):
    H = svo.World.generate(1, 1, 1, 128, 4)                     # not uploaded
    chunks, n = (C.c_int * 8)(*[-7] * 8), C.c_int(-7)
    vec = lambda v: (C.c_float * 3)(*v)

    def call(world, op, bmin, size):
        rc = svo.lib.svo_world_edit_cube(world, op, bmin, size, C.c_uint16(5), chunks, C.byref(n))
        assert list(chunks) == [-7] * 8 and n.value == -7, "an output was written"
        return rc

    good = vec((10.0, 10.0, 10.0))
    assert call(None, 0, good, 8.0) == -1
    assert call(H._h, 0, None, 8.0) == -1
    for op in (-1, 3):
        assert call(H._h, op, good, 8.0) == -1
    for size in (0.0, -8.0, float("nan"), float("inf")):
        assert call(H._h, 0, good, size) == -1
    for bad in ((float("nan"), 0.0, 0.0), (0.0, float("nan"), 0.0), (0.0, 0.0, float("nan")), (float("inf"), 0.0, 0.0)):
        assert call(H._h, 1, vec(bad), 8.0) == -1
    for op in (0, 1, 2):
        assert call(H._h, op, good, 8.0) == -5                  # SVO_ERR_NOT_UPLOADED
    assert svo.lib.svo_world_edit_cube(H._h, 0, good, 8.0, C.c_uint16(5), None, None) == -5
    with pytest.raises(svo.SvoError) as e:
        H.edit_cube(svo.EDIT_DESTROY, (10, 10, 10), 8.0)
    assert e.value.code == -5
    before = H.chunk(0)
    assert np.array_equal(before["tree"], svo.World.generate(1, 1, 1, 128, 4).chunk(0)["tree"])
    H.destroy()


# ---- the model on hand-derived cases ----------------------------------------------------------------------------------------------
def depth64(t, near=0.125, far=8192.0):
    return (1.0 / t - 1.0 / near) / (1.0 / far - 1.0 / near)


def one(o, d, box, dst=(0.25, 0.5, 0.75, 1.0), **kw):
    out, st = B.shade_boxes(np.array([dst], F), np.array(o, F), np.array([d], F), box, **kw)
    return out[0], {k: int(v[0]) for k, v in st.items()}


def blend(src, a, dst):
    src, a, dst = np.asarray(src, F), F(a), np.asarray(dst, F)
    return (src * a + dst * (F(1) - a)).astype(F)


def test_axis_parallel_ray_through_a_unit_cube():
    hit, tnear, tfar, fnear, ffar = B.slabs((0.5, 0.5, -2.0), np.array([[0, 0, 1]], F), (0, 0, 0), 1.0)
    assert (bool(hit[0]), float(tnear[0]), float(tfar[0])) == (True, 2.0, 3.0)
    assert (B.FACE_NAMES[fnear[0]], B.FACE_NAMES[ffar[0]]) == ("-Z", "+Z")
    for o, d, faces, ts in (((3.0, 0.5, 0.5), (-1, 0, 0), ("+X", "-X"), (2.0, 3.0)), ((0.5, -1.0, 0.5), (0, 2, 0), ("-Y", "+Y"), (0.5, 1.0))):
        hit, tnear, tfar, fnear, ffar = B.slabs(o, np.array([d], F), (0, 0, 0), 1.0)
        assert hit[0] and (B.FACE_NAMES[fnear[0]], B.FACE_NAMES[ffar[0]]) == faces and (float(tnear[0]), float(tfar[0])) == ts
    f = B.fragment_depth(np.array([2.0, 3.0, 0.125, 8192.0], F))
    assert np.allclose(f[:2].astype(np.float64), [depth64(2.0), depth64(3.0)], rtol=1e-6, atol=0)
    assert f[2] == 0 and f[3] == 1 and f[0] < f[1]               # the planes map to 0 and 1; depth grows with distance
    assert np.allclose(B.fragment_depth(np.array([5.0], F), 0.5, 100.0).astype(np.float64), depth64(5.0, 0.5, 100.0), rtol=1e-6)
    px, st = one((0.5, 0.5, -2.0), (0, 0, 1), B.box(**UNIT, color=(1, 0, 0), alpha=1.0))
    assert list(px[:3]) == [1, 0, 0] and px[3] == f[0] and st == {"passed": 1, "failed": 1, "edge": 0}


def test_ties_go_to_the_first_axis():
    hit, tnear, tfar, fnear, ffar = B.slabs((-1.0, 0.5, -1.0), np.array([[1, 0, 1]], F), (0, 0, 0), 1.0)
    assert hit[0] and float(tnear[0]) == 1.0 and float(tfar[0]) == 2.0
    assert (B.FACE_NAMES[fnear[0]], B.FACE_NAMES[ffar[0]]) == ("-X", "+X")
    hit, _, _, fnear, ffar = B.slabs((0.5, 2.0, 2.0), np.array([[0, -1, -1]], F), (0, 0, 0), 1.0)
    assert hit[0] and (B.FACE_NAMES[fnear[0]], B.FACE_NAMES[ffar[0]]) == ("+Y", "-Y")     # y before z


def test_both_draw_orders():
    """+Y seen from above: the exit face -Y is drawn first (place 4 before 5), passes against the background, then the entry face passes
    in front of it: two layers.  -Z seen from the front: the entry face is drawn first (place 0) and the exit face +Z fails against it."""
    dst = np.array([0.25, 0.5, 0.75, 1.0], F)
    cube = B.box(**UNIT, color=GREY, alpha=0.2)
    px, st = one((0.5, 3.0, 0.5), (0, -1, 0), cube, dst)
    assert st == {"passed": 2, "failed": 0, "edge": 0}
    assert np.array_equal(px[:3], blend(GREY, 0.2, blend(GREY, 0.2, dst[:3]))) and px[3] == B.fragment_depth(np.array([2.0], F))[0]
    px, st = one((0.5, 0.5, -2.0), (0, 0, 1), cube, dst)
    assert st == {"passed": 1, "failed": 1, "edge": 0}
    assert np.array_equal(px[:3], blend(GREY, 0.2, dst[:3])) and px[3] == B.fragment_depth(np.array([2.0], F))[0]
    # the other face pairs: +X from the right is the exit -X first (1 before 3), +Z from behind the exit -Z first (0 before 2)
    assert one((3.0, 0.5, 0.5), (-1, 0, 0), cube)[1]["passed"] == 2 and one((-2.0, 0.5, 0.5), (1, 0, 0), cube)[1]["passed"] == 1
    assert one((0.5, 0.5, 3.0), (0, 0, -1), cube)[1]["passed"] == 2 and one((0.5, -2.0, 0.5), (0, 1, 0), cube)[1]["passed"] == 1


def test_the_cursor_edge_rule_to_the_ulp():
    cursor = B.box(**UNIT, color=GREY, alpha=0.2, style=B.CURSOR)
    dst = np.array([0.25, 0.5, 0.75, 1.0], F)
    lo, hi = F(1) / F(64), F(1) - F(1) / F(64)
    assert (float(lo), float(hi)) == (0.015625, 0.984375)
    cases = [(lo, True), (ulp(lo, 1), False), (ulp(lo, -1), True), (hi, True), (ulp(hi, -1), False), (ulp(hi, 1), True), (F(0.5), False)]
    for x, edge in cases:
        for o, d in (((x, 0.5, -2.0), (0, 0, 1)), ((0.5, x, -2.0), (0, 0, 1)), ((-2.0, x, 0.5), (1, 0, 0)), ((-2.0, 0.5, x), (1, 0, 0)),
                     ((x, -2.0, 0.5), (0, 1, 0)), ((0.5, -2.0, x), (0, 1, 0))):
            px, st = one(o, d, cursor, dst)
            assert st["passed"] == 1 and st["edge"] == int(edge), (x, o)
            assert np.array_equal(px[:3], np.zeros(3, F) if edge else blend(GREY, 0.2, dst[:3])), (x, o)
    # the same box drawn solid has no edges
    px, st = one((lo, 0.5, -2.0), (0, 0, 1), B.box(**UNIT, color=GREY, alpha=0.2, style=B.SOLID), dst)
    assert st["edge"] == 0 and np.array_equal(px[:3], blend(GREY, 0.2, dst[:3]))


def test_a_fragment_at_the_stored_depth_fails():
    f2 = B.fragment_depth(np.array([2.0], F))[0]
    cube = B.box(**UNIT, color=(1, 0, 0), alpha=1.0)
    dst = np.array([0.25, 0.5, 0.75, f2], F)
    px, st = one((0.5, 0.5, -2.0), (0, 0, 1), cube, dst)         # f == D: GL_LESS fails; the exit face is farther still
    assert st == {"passed": 0, "failed": 2, "edge": 0} and np.array_equal(px.view(np.uint32), dst.view(np.uint32))
    dst[3] = ulp(f2, 1)
    px, st = one((0.5, 0.5, -2.0), (0, 0, 1), cube, dst)
    assert st["passed"] == 1 and px[3] == f2
    dst[3] = np.nan                                             # a NaN depth fails every fragment
    px, st = one((0.5, 0.5, -2.0), (0, 0, 1), cube, dst)
    assert st["passed"] == 0 and np.array_equal(px.view(np.uint32), dst.view(np.uint32))


def test_a_zero_direction_component_inside_and_outside_the_slab():
    d = np.array([[0, 0, 1]], F)
    for x, want in ((0.5, True), (0.0, True), (1.0, True), (ulp(1.0, 1), False), (-1e-30, False), (1.5, False)):
        assert bool(B.slabs((x, 0.5, -2.0), d, (0, 0, 0), 1.0)[0][0]) == want, x
    assert bool(B.slabs((0.5, 0.5, -2.0), np.array([[-0.0, 0.0, 1.0]], F), (0, 0, 0), 1.0)[0][0])     # -0 == 0


def test_eye_inside_behind_hidden_and_degenerate_boxes():
    dst = np.array([0.25, 0.5, 0.75, 1.0], F)
    cube = B.box(**UNIT, color=(1, 0, 0), alpha=1.0)
    px, st = one((0.5, 0.5, 0.5), (0, 0, 1), cube, dst)          # inside: tnear = -0.5, the exit face alone
    assert st == {"passed": 1, "failed": 0, "edge": 0} and px[3] == B.fragment_depth(np.array([0.5], F))[0]
    px, st = one((0.5, 0.5, 2.0), (0, 0, 1), cube, dst)          # behind the eye: tnear = -2, tfar = -1
    assert st == {"passed": 0, "failed": 0, "edge": 0} and np.array_equal(px.view(np.uint32), dst.view(np.uint32))
    for bad in (B.box(**UNIT, alpha=1.0, style=B.SOLID | B.HIDDEN), B.box(**UNIT, alpha=1.0, style=B.CURSOR | B.HIDDEN),
                B.box((0, 0, 0), 0.0, alpha=1.0), B.box((0, 0, 0), -1.0, alpha=1.0), B.box((0, 0, 0), np.nan, alpha=1.0)):
        px, st = one((0.5, 0.5, -2.0), (0, 0, 1), bad, dst)
        assert st == {"passed": 0, "failed": 0, "edge": 0} and np.array_equal(px.view(np.uint32), dst.view(np.uint32))
    # the list goes in order and a skipped box does not end it
    px, st = one((0.5, 0.5, -2.0), (0, 0, 1), B.box_list(B.box((0, 0, 0), 0.0), cube), dst)
    assert st["passed"] == 1 and list(px[:3]) == [1, 0, 0]


@pytest.mark.parametrize("alpha", [0.0, 1.0, 0.2])
def test_the_blend(alpha):
    dst = np.array([0.25, 0.5, 0.75, 1.0], F)
    color = (0.9, 0.3, 0.1)
    px, st = one((0.5, 0.5, -2.0), (0, 0, 1), B.box(**UNIT, color=color, alpha=alpha), dst)
    assert st["passed"] == 1 and px[3] == B.fragment_depth(np.array([2.0], F))[0]      # the depth is written whatever the alpha
    if alpha == 0.0:
        assert np.array_equal(px[:3], dst[:3])
    elif alpha == 1.0:
        assert np.array_equal(px[:3], np.array(color, F))
    else:
        want = [float(F(F(c) * F(0.2)) + F(F(q) * F(F(1) - F(0.2)))) for c, q in zip(color, dst[:3])]
        assert [float(v) for v in px[:3]] == want
        assert np.allclose(px[:3], np.array(color) * 0.2 + dst[:3] * 0.8, atol=1e-6)


def test_list_order_matters():
    a, b = B.box(**UNIT, color=(1, 0, 0), alpha=0.5), B.box((0.0, 0.0, -0.5), 1.0, color=(0, 0, 1), alpha=0.5)
    p1, _ = one((0.5, 0.5, -2.0), (0, 0, 1), B.box_list(a, b))
    p2, _ = one((0.5, 0.5, -2.0), (0, 0, 1), B.box_list(b, a))
    assert not np.array_equal(p1[:3], p2[:3]) and p1[3] == p2[3] == B.fragment_depth(np.array([1.5], F))[0]


def test_cursor_place_model():
    rec = np.zeros(1, B.HIT_DTYPE)[0]
    rec["t"], rec["flags"] = 10.0, 1
    start = B.box((1, 2, 3), 9.0, (0.1, 0.2, 0.3), 0.4, B.CURSOR | B.HIDDEN)
    got = B.cursor_place((1.0, 2.0, 3.0), (0.0, 0.6, 0.8), rec, 4.0, start)[0]
    want = np.array([1.0, F(2.0) + F(0.6) * F(10.0), F(3.0) + F(0.8) * F(10.0)], F) - F(2.0)
    assert np.array_equal(got["bmin"], want) and got["size"] == 4.0 and got["style"] == B.CURSOR
    assert np.array_equal(got["color"], start["color"][0]) and got["alpha"] == start["alpha"][0]
    for flags in (0, 1 | (1 << 15), 1 << 15):                    # a miss, an error record
        rec["flags"] = flags
        shown = B.box((1, 2, 3), 9.0, (0.1, 0.2, 0.3), 0.4, B.CURSOR)
        got = B.cursor_place((1.0, 2.0, 3.0), (0.0, 0.6, 0.8), rec, 4.0, shown)[0]
        assert got["style"] == B.CURSOR | B.HIDDEN and np.array_equal(got["bmin"], [1, 2, 3]) and got["size"] == 9.0


# ---- the corner rule ---------------------------------------------------------------------------------------------------------------
GRID = ((2, 1, 2), 128, (0, 0, 0))


def test_corner_rule_on_a_2x1x2_world():
    calls, distinct = B.corner_chunks((10, 10, 10), 8.0, *GRID)
    assert calls == [0] * 8 and distinct == [0]                 # the reference edits chunk 0 eight times
    calls, distinct = B.corner_chunks((124, 10, 124), 8.0, *GRID)
    assert calls == [0, 2, 0, 2, 1, 3, 1, 3] and distinct == [0, 2, 1, 3]      # the seam corner: i & 1 moves z, i & 4 moves x
    for bmin, want in (((-4, 10, 10), [0]), ((252, 10, 10), [1]), ((10, -4, 10), [0]), ((10, 124, 10), [0]), ((10, 10, -4), [0]),
                       ((10, 10, 252), [2]), ((252, 124, 252), [3]), ((-20, 10, 10), []), ((300, 10, 10), []), ((10, 200, 10), [])):
        assert B.corner_chunks(bmin, 8.0, *GRID)[1] == want, bmin
    assert B.corner_chunks((120, 10, 10), 8.0, *GRID)[1] == [0, 1]      # x = 128 exactly belongs to chunk 1 (and lies in its closed box)
    assert B.corner_chunks((248, 10, 10), 8.0, *GRID)[1] == [1]         # x = 256, the world's max face, wraps to chunk 0, which does not hold it
    # the rule's limitation: a cube wider than a chunk skips what lies between its corners (none here: only two chunks a side), and one
    # that spans the world reaches no chunk with the corners outside
    assert B.corner_chunks((-10, 10, 10), 300.0, *GRID)[1] == []


def test_corner_rule_with_negative_chunkcoordmin(svo):
    dims, cs, ccm = (2, 2, 2), 128, (-1, -1, -1)
    assert B.corner_chunks((-4, -4, -4), 8.0, dims, cs, ccm)[1] == [7, 5, 3, 1, 6, 4, 2, 0]
    assert B.corner_chunks((-100, -100, -100), 8.0, dims, cs, ccm)[1] == [7]
    # index_float sends an exact negative multiple one chunk down: x = -128 names chunk x = -2, which wraps to one that does not hold it
    assert B.index_float((-128.0, 0.0, 0.0), cs)[0] == -2
    assert B.corner_chunks((-128, 10, 10), 8.0, dims, cs, ccm)[1] == [1]
    assert B.corner_chunks((-132, 10, 10), 8.0, dims, cs, ccm)[1] == [1]
    # the model's index / index_float / chunk positions are the library's
    W = svo.World.generate(2, 2, 2, cs, 3, chunkcoordmin=ccm)
    pos = B.chunk_positions(dims, cs, ccm)
    for i in range(8):
        assert tuple(pos[i]) == W.chunk(i)["position"]
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(-300, 300, (200, 3)), rng.integers(-3, 3, (50, 3)) * 128.0]).astype(F)
    for p in pts:
        q = B.index_float(p, cs)
        assert tuple(q) == W.index_float(p) and B.world_index(q, dims) == W.index(*q)
    W.destroy()


# ---- what "once per distinct chunk" rests on -------------------------------------------------------------------------------------------
def oracle_edit(oracle, O, chunk, op, lo, hi, material):
    dt, dw = oracle.Delta(), oracle.Delta()
    root = C.byref(O.w.chunk[chunk])
    if op in (1, 2):
        oracle.lib.orc_destroy(root, oracle.vec3(lo), oracle.vec3(hi), C.byref(dt), C.byref(dw))
    if op in (0, 2):
        oracle.lib.orc_build(root, oracle.vec3(lo), oracle.vec3(hi), material, C.byref(dt), C.byref(dw))


IDEMPOTENCE_BOXES = [((20, 60, 20), 50.0),                      # in the air, on the lattice
                     ((100.3, 2.7, 40.1), 50.6),                # across the seam, through the water plane, off the lattice
                     ((120, 0, 60), 16.0),                      # across the seam, on the lattice
                     ((63.99, 5.99, 63.99), 0.02),              # straddles a node corner and the water plane
                     ((97.7, 1.1, 11.3), 33.3)]


@pytest.mark.parametrize("op", [0, 1, 2], ids=["build", "destroy", "replace"])
def test_a_repeated_edit_leaves_the_pools_as_they_are(oracle, op):
    O = oracle.OracleWorld.generate(2, 1, 1, 128, 6)
    changed = 0
    for bmin, size in IDEMPOTENCE_BOXES:
        lo = np.array(bmin, F)
        hi = (lo + F(size)).astype(F)
        for chunk in (0, 1):
            start = O.chunk(chunk)
            oracle_edit(oracle, O, chunk, op, lo, hi, 5)
            once = O.chunk(chunk)
            oracle_edit(oracle, O, chunk, op, lo, hi, 5)
            twice = O.chunk(chunk)
            for k in ("tree", "twig"):
                assert once[k].size == twice[k].size and np.array_equal(once[k], twice[k]), (op, bmin, chunk, k)
            assert (once["treestoragesize"], once["twigstoragesize"]) == (twice["treestoragesize"], twice["twigstoragesize"])
            changed += once["tree"].size != start["tree"].size or not np.array_equal(once["tree"], start["tree"]) or not np.array_equal(once["twig"], start["twig"])
    assert changed >= 4, "the edits changed nothing: the check is empty"
    O.close()


# ---- what the GPU tests rest on -------------------------------------------------------------------------------------------------------
def test_the_placement_provides_every_kind_of_pixel(svo, oracle):
    """By the CPU oracle (records, and its shading for the depths): in each of the two mixed views the seven boxes that do not hold the eye
    give every kind of pixel tests/test_boxes.py asks for, the box behind the terrain shows nowhere, and pixels stay untouched."""
    import hit_voxels_model as M
    (w, h, d), cs, ccm = B.world_spec()
    O = oracle.OracleWorld.from_chunks(M.make_chunks(svo, B.WORLD), w, h, d, cs, ccm)
    P = svo.shade_defaults()
    for name, cam in B.mixed_cameras(svo, B.WORLD).items():
        g = O.trace_image(cam, params=oracle.make_params(shadow=True)).reshape(-1)
        base = oracle.shade_image(cam, P, (0, 0) + B.IMAGE, g).reshape(-1, 4)
        hit = (g["flags"] & 1) != 0
        boxes = B.scene_boxes(cam, g)
        assert boxes.size == 8
        dirs = B.camera_dirs(cam)
        out, st = B.shade_boxes(base, B.eye_of(cam), dirs, B.without_eye_box(boxes))
        got = B.counts(hit, st)
        print(name, got)
        for k, need in B.NEEDED.items():
            assert got[k] >= 2 * need, (name, k, got)           # twice what the GPU test asks: its depths come from the device's shading
        untouched = st["passed"] == 0
        assert untouched.sum() >= 300 and np.array_equal(out[untouched].view(np.uint32), base[untouched].view(np.uint32))
        per_box = [B.shade_boxes(base, B.eye_of(cam), dirs, boxes[i:i + 1])[1] for i in range(8)]
        assert per_box[0]["passed"].sum() > 0 and per_box[1]["passed"].sum() > 0 and per_box[1]["failed"].sum() > 0
        assert per_box[2]["passed"].sum() == 0 and (per_box[2]["failed"] > 0).sum() >= 5, "the box behind the terrain"
        assert (~hit & (per_box[3]["passed"] > 0)).sum() >= 50
        assert np.all(per_box[5]["passed"] == 1) and np.all(per_box[5]["failed"] == 0), "the box that holds the eye: one exit face on every pixel"
        assert per_box[6]["passed"].sum() == 0 and per_box[6]["failed"].sum() == 0 and per_box[7]["passed"].sum() == 0
        a, _ = B.shade_boxes(base, B.eye_of(cam), dirs, B.translucent_pair(boxes))
        b, _ = B.shade_boxes(base, B.eye_of(cam), dirs, B.translucent_pair(boxes)[::-1])
        assert (a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum() >= 20, "the order of the translucent pair does not show"
    O.close()

"""clearance_positions.py — where the clearance tests put their worlds — TEST INFRASTRUCTURE.

The margins of the two proofs are multiples of u, the float32 spacing at the world's largest corner coordinate, and the bits
are used only if eps >= 2u.  A world of 2x1x2 chunks of 128 at the origin has u = 2^-15 and eps = 4u, one chunk layer and an
index that equals the position; the positions below vary each of those.  tests/test_clearance_positions_cpu.py and
tests/test_clearance_positions.py run them on the CPU models and on the device.

    bits  / flags    does the rule of 6t / of 6u hold there (ClearanceModel.enabled / BrickClearanceModel.brick_enabled)
    eps              the launch's eps, 0 = the march's own 1/8192
    sweep_eps        an eps at which the model is enabled on this world: the device sweep never looks at eps, so its counts are
                     those of the model at this eps even where the launch's eps keeps the bits from being used
"""
from __future__ import annotations

import numpy as np

CHUNK = 128
EPS = 1.0 / 8192


def _p(dims, ccm, eps, bits, flags, sweep_eps=None, slab=False):
    return dict(dims=dims, ccm=ccm, eps=eps, bits=bits, flags=flags, sweep_eps=eps if sweep_eps is None else sweep_eps, slab=slab)


POSITIONS = {
    "limit":         _p((2, 1, 2), (2, 0, 2), 0.0, True, True),                 # corner exactly 512: u = 2^-14, eps = 2u (the 4x1x4 headline world)
    "deep":          _p((2, 1, 2), (5, 0, 5), 0.0, True, True),                 # all of it in [512, 1024); odd minimum: toroidal index
    "mixed_u":       _p((2, 1, 2), (3, 0, 5), 0.0, True, True),                 # x below 512, z above; toroidal
    "neg":           _p((2, 1, 2), (-1, 0, -1), 0.0, True, False),              # straddles the origin: node bits on, brick flags all 0
    "neg_far":       _p((2, 1, 2), (-4, 0, -4), 0.0, True, False),              # u = 2^-14 with negative coordinates
    "beyond":        _p((2, 1, 2), (6, 0, 6), 0.0, False, False, sweep_eps=1.0 / 4096),     # corner 1024: u = 2^-13, eps < 2u: prepared, never used
    "beyond_eps":    _p((2, 1, 2), (6, 0, 6), 1.0 / 4096, True, True),          # the same world, an eps that meets the premise again
    "small_eps":     _p((2, 1, 2), (0, 0, 0), 1.0 / 16384, True, True),         # the limit reached from the eps side (u = 2^-15)
    "below_eps":     _p((2, 1, 2), (0, 0, 0), 1.0 / 32768, False, False, sweep_eps=0.0),    # eps < 2u at the origin: never used
    "big_eps":       _p((2, 1, 2), (0, 0, 0), 1.0 / 2048, True, True),          # bits used with an eps the sweep was not told about
    "stacked":       _p((2, 2, 1), (0, 0, 0), 0.0, True, True),                 # a y seam; the upper two chunks are one EMPTY node each
    "stacked_slab":  _p((2, 2, 1), (2, 2, 0), 0.0, True, True, slab=True),      # everything EMPTY but one slab in the upper layer
    "stacked_torus": _p((2, 2, 1), (1, 1, 3), 0.0, True, True, slab=True),      # the same slab with a toroidal index
}

# boxes in the frame of a world at the origin: (lo, hi), none crosses a chunk face
STRUCTURES = [
    ((96.0, 0.0, 32.0), (112.0, 96.0, 48.0)),               # a tower: under the default light it shades x < 96
    ((112.0, 0.0, 80.0), (128.0, 64.0, 96.0)), ((128.0, 0.0, 80.0), (144.0, 64.0, 96.0)),       # an arch over the seam x = 128: legs ...
    ((120.0, 64.0, 80.0), (128.0, 72.0, 96.0)), ((128.0, 64.0, 80.0), (136.0, 72.0, 96.0)),     # ... and lintel
    ((160.0, 40.0, 16.0), (224.0, 44.0, 48.0)),             # a thin roof: bricks with empty cells
    ((112.0, 0.0, 160.0), (128.0, 112.0, 176.0)),           # a tower on the seam x = 128: it shades the chunk beside it only
]
SLAB = [((40.0, 160.0, 40.0), (128.0, 168.0, 90.0)), ((128.0, 160.0, 40.0), (200.0, 168.0, 90.0))]     # across the x seam, in the upper layer

# (eye, forward, up hint) in the same frame; vfov 60
CAMERAS = [((128.3, 120.2, -70.1), (0.0, -0.55, 0.83), (0.0, 1.0, 0.0)), ((200.7, 90.4, 40.2), (-0.5, -0.6, 0.62), (0.0, 1.0, 0.0))]
SLAB_CAMERAS = [((120.3, 60.2, 65.1), (0.1, 1.0, 0.05), (0.0, 0.0, 1.0)),           # from below: the face the `up` light reaches
                ((120.3, 225.2, 10.1), (0.0, -0.7, 0.6), (0.0, 1.0, 0.0))]          # from above


def offset(ccm, chunksize=CHUNK):
    return tuple(float(c * chunksize) for c in ccm)


def translated(boxes, dims, ccm, chunksize=CHUNK):
    """The boxes that lie inside a world of `dims` chunks at the origin, moved to chunkcoordmin `ccm`."""
    off = offset(ccm, chunksize)
    ext = tuple(float(d * chunksize) for d in dims)
    return [(tuple(l + o for l, o in zip(lo, off)), tuple(h + o for h, o in zip(hi, off)))
            for lo, hi in boxes if all(lo[a] >= 0.0 and hi[a] <= ext[a] for a in range(3))]


def boxes_of(pos, chunksize=CHUNK):
    return translated(SLAB if pos["slab"] else STRUCTURES, pos["dims"], pos["ccm"], chunksize)


def centre(lo, hi):
    return tuple(0.5 * (l + h) for l, h in zip(lo, hi))


def oracle_chunk_at(ob, O, p):
    """World::index(index_float(p)) on the oracle: with a minimum that is no multiple of the grid, chunk 0 is not the corner chunk."""
    import ctypes as C
    q = (C.c_int * 3)()
    ob.lib.orc_world_index_float(C.byref(O.w), ob.vec3(p), q)
    return int(ob.lib.orc_world_index3(C.byref(O.w), q[0], q[1], q[2]))


def spacing(dims, ccm, chunksize=CHUNK):
    """u of the proofs, stated on its own: the float32 spacing at the largest |coordinate| of a world corner."""
    m = max(abs(float((ccm[a] + k * dims[a]) * chunksize)) for a in range(3) for k in (0, 1))
    return float(np.spacing(np.float32(max(m, 1.0))))

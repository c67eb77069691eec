"""Which status wins when an entry point that marches or queries an uploaded world is given several faults at once.  The entry
points differ in the order they look at things (svo_trace_rays on a world that is not uploaded answers an unknown kernel id with
SVO_ERR_NOT_UPLOADED, svo_world_locate with SVO_ERR_INVALID_ARG), callers may have come to rely on it, and so the table below pins it:
every entry point, on a world that was never uploaded and on a NULL world, with no further fault, with each further fault that
applies to it and with each pair of them.  The statuses were recorded from the library as it was before the entry points came to share
one params check, one scratch protocol and one launch helper; they are not derived from the code under test.  CPU only: every call
returns before any device work."""
import ctypes as C
import itertools

import numpy as np
import pytest

FAKE = 256                                  # a non-NULL "device pointer": never dereferenced
L = 1 << 30
# the faults beside the world's own (not uploaded / NULL), in the order the table's keys name them
ST, SEM, KER, OUT, NEG, EMPTY = "see_through", "semantics", "kernel", "null_out", "negative", "empty"
PARAMS = (ST, SEM, KER)
ALL = PARAMS + (OUT, NEG, EMPTY)
# entry point -> the faults that apply to it
ENTRIES = {
    "svo_trace": ALL, "svo_trace_rows": ALL, "svo_trace_frames": ALL, "svo_trace_rows_frames": ALL,
    "svo_trace_rays": ALL, "svo_trace_segments": ALL, "svo_trace_translucent": ALL, "svo_trace_local_shadows": ALL,
    "svo_shadowmap_render": PARAMS + (OUT,),                    # (the output is the map's depth image; a map has no count)
    "svo_world_locate": ALL, "svo_hit_ao": ALL,
    "svo_hit_voxels": (OUT, NEG, EMPTY), "svo_tile_order": (OUT, NEG, EMPTY),
    "svo_trace_last_ray_count": (OUT,),
}
OK, INVALID, NOT_UPLOADED = 0, -1, -5

# entry point -> { faults: (status on the world that is not uploaded, status on the NULL world) }
EXPECTED = {
    "svo_trace": {
        "": (-5, -1), "see_through": (-1, -1), "semantics": (-5, -1), "kernel": (-5, -1), "null_out": (-5, -1), "negative": (-5, -1),
        "empty": (-5, -1), "see_through+semantics": (-1, -1), "see_through+kernel": (-1, -1), "see_through+null_out": (-1, -1),
        "see_through+negative": (-1, -1), "see_through+empty": (-1, -1), "semantics+kernel": (-5, -1), "semantics+null_out": (-5, -1),
        "semantics+negative": (-5, -1), "semantics+empty": (-5, -1), "kernel+null_out": (-5, -1), "kernel+negative": (-5, -1),
        "kernel+empty": (-5, -1), "null_out+negative": (-5, -1), "null_out+empty": (-5, -1),
    },
    "svo_trace_rows": {
        "": (-5, -1), "see_through": (-1, -1), "semantics": (-5, -1), "kernel": (-5, -1), "null_out": (-5, -1), "negative": (-5, -1),
        "empty": (-5, -1), "see_through+semantics": (-1, -1), "see_through+kernel": (-1, -1), "see_through+null_out": (-1, -1),
        "see_through+negative": (-1, -1), "see_through+empty": (-1, -1), "semantics+kernel": (-5, -1), "semantics+null_out": (-5, -1),
        "semantics+negative": (-5, -1), "semantics+empty": (-5, -1), "kernel+null_out": (-5, -1), "kernel+negative": (-5, -1),
        "kernel+empty": (-5, -1), "null_out+negative": (-5, -1), "null_out+empty": (-5, -1),
    },
    "svo_trace_frames": {
        "": (-5, -1), "see_through": (-1, -1), "semantics": (-5, -1), "kernel": (-5, -1), "null_out": (-5, -1), "negative": (-5, -1),
        "empty": (-5, -1), "see_through+semantics": (-1, -1), "see_through+kernel": (-1, -1), "see_through+null_out": (-1, -1),
        "see_through+negative": (-1, -1), "see_through+empty": (-1, -1), "semantics+kernel": (-5, -1), "semantics+null_out": (-5, -1),
        "semantics+negative": (-5, -1), "semantics+empty": (-5, -1), "kernel+null_out": (-5, -1), "kernel+negative": (-5, -1),
        "kernel+empty": (-5, -1), "null_out+negative": (-5, -1), "null_out+empty": (-5, -1),
    },
    "svo_trace_rows_frames": {
        "": (-5, -1), "see_through": (-1, -1), "semantics": (-5, -1), "kernel": (-5, -1), "null_out": (-5, -1), "negative": (-5, -1),
        "empty": (-5, -1), "see_through+semantics": (-1, -1), "see_through+kernel": (-1, -1), "see_through+null_out": (-1, -1),
        "see_through+negative": (-1, -1), "see_through+empty": (-1, -1), "semantics+kernel": (-5, -1), "semantics+null_out": (-5, -1),
        "semantics+negative": (-5, -1), "semantics+empty": (-5, -1), "kernel+null_out": (-5, -1), "kernel+negative": (-5, -1),
        "kernel+empty": (-5, -1), "null_out+negative": (-5, -1), "null_out+empty": (-5, -1),
    },
    "svo_trace_rays": {
        "": (-5, -1), "see_through": (-1, -1), "semantics": (-5, -1), "kernel": (-5, -1), "null_out": (-5, -1), "negative": (-5, -1),
        "empty": (-5, -1), "see_through+semantics": (-1, -1), "see_through+kernel": (-1, -1), "see_through+null_out": (-1, -1),
        "see_through+negative": (-1, -1), "see_through+empty": (-1, -1), "semantics+kernel": (-5, -1), "semantics+null_out": (-5, -1),
        "semantics+negative": (-5, -1), "semantics+empty": (-5, -1), "kernel+null_out": (-5, -1), "kernel+negative": (-5, -1),
        "kernel+empty": (-5, -1), "null_out+negative": (-5, -1), "null_out+empty": (-5, -1),
    },
    "svo_trace_segments": {
        "": (-5, -1), "see_through": (-1, -1), "semantics": (-5, -1), "kernel": (-5, -1), "null_out": (-5, -1), "negative": (-5, -1),
        "empty": (-5, -1), "see_through+semantics": (-1, -1), "see_through+kernel": (-1, -1), "see_through+null_out": (-1, -1),
        "see_through+negative": (-1, -1), "see_through+empty": (-1, -1), "semantics+kernel": (-5, -1), "semantics+null_out": (-5, -1),
        "semantics+negative": (-5, -1), "semantics+empty": (-5, -1), "kernel+null_out": (-5, -1), "kernel+negative": (-5, -1),
        "kernel+empty": (-5, -1), "null_out+negative": (-5, -1), "null_out+empty": (-5, -1),
    },
    "svo_trace_translucent": {
        "": (-5, -1), "see_through": (-1, -1), "semantics": (-5, -1), "kernel": (-5, -1), "null_out": (-1, -1), "negative": (-5, -1),
        "empty": (-5, -1), "see_through+semantics": (-1, -1), "see_through+kernel": (-1, -1), "see_through+null_out": (-1, -1),
        "see_through+negative": (-1, -1), "see_through+empty": (-1, -1), "semantics+kernel": (-5, -1), "semantics+null_out": (-1, -1),
        "semantics+negative": (-5, -1), "semantics+empty": (-5, -1), "kernel+null_out": (-1, -1), "kernel+negative": (-5, -1),
        "kernel+empty": (-5, -1), "null_out+negative": (-1, -1), "null_out+empty": (-1, -1),
    },
    "svo_trace_local_shadows": {
        "": (-5, -1), "see_through": (-1, -1), "semantics": (-5, -1), "kernel": (-5, -1), "null_out": (-1, -1), "negative": (-1, -1),
        "empty": (-5, -1), "see_through+semantics": (-1, -1), "see_through+kernel": (-1, -1), "see_through+null_out": (-1, -1),
        "see_through+negative": (-1, -1), "see_through+empty": (-1, -1), "semantics+kernel": (-5, -1), "semantics+null_out": (-1, -1),
        "semantics+negative": (-1, -1), "semantics+empty": (-5, -1), "kernel+null_out": (-1, -1), "kernel+negative": (-1, -1),
        "kernel+empty": (-5, -1), "null_out+negative": (-1, -1), "null_out+empty": (-1, -1),
    },
    "svo_shadowmap_render": {
        "": (-5, -1), "see_through": (-1, -1), "semantics": (-5, -1), "kernel": (-5, -1), "null_out": (-1, -1), "see_through+semantics": (-1, -1),
        "see_through+kernel": (-1, -1), "see_through+null_out": (-1, -1), "semantics+kernel": (-5, -1), "semantics+null_out": (-1, -1),
        "kernel+null_out": (-1, -1),
    },
    "svo_world_locate": {
        "": (-5, -1), "see_through": (-1, -1), "semantics": (-1, -1), "kernel": (-1, -1), "null_out": (-1, -1), "negative": (-1, -1),
        "empty": (-5, -1), "see_through+semantics": (-1, -1), "see_through+kernel": (-1, -1), "see_through+null_out": (-1, -1),
        "see_through+negative": (-1, -1), "see_through+empty": (-1, -1), "semantics+kernel": (-1, -1), "semantics+null_out": (-1, -1),
        "semantics+negative": (-1, -1), "semantics+empty": (-1, -1), "kernel+null_out": (-1, -1), "kernel+negative": (-1, -1),
        "kernel+empty": (-1, -1), "null_out+negative": (-1, -1), "null_out+empty": (-5, -1),
    },
    "svo_hit_ao": {
        "": (-5, -1), "see_through": (-1, -1), "semantics": (-1, -1), "kernel": (-1, -1), "null_out": (-1, -1), "negative": (-1, -1),
        "empty": (-5, -1), "see_through+semantics": (-1, -1), "see_through+kernel": (-1, -1), "see_through+null_out": (-1, -1),
        "see_through+negative": (-1, -1), "see_through+empty": (-1, -1), "semantics+kernel": (-1, -1), "semantics+null_out": (-1, -1),
        "semantics+negative": (-1, -1), "semantics+empty": (-1, -1), "kernel+null_out": (-1, -1), "kernel+negative": (-1, -1),
        "kernel+empty": (-1, -1), "null_out+negative": (-1, -1), "null_out+empty": (-5, -1),
    },
    "svo_hit_voxels": {
        "": (-5, -1), "null_out": (-1, -1), "negative": (-1, -1), "empty": (-5, -1), "null_out+negative": (-1, -1), "null_out+empty": (-5, -1),
    },
    "svo_tile_order": {
        "": (-5, -1), "null_out": (-1, -1), "negative": (-1, -1), "empty": (-5, -1), "null_out+negative": (-1, -1), "null_out+empty": (-1, -1),
    },
    "svo_trace_last_ray_count": {
        "": (-5, -1), "null_out": (-1, -1),
    },
}


def fault_sets(entry):
    """no further fault, each one, each pair (a count is negative or zero, not both)"""
    faults = ENTRIES[entry]
    sets = [()] + [(f,) for f in faults] + [p for p in itertools.combinations(faults, 2) if p != (NEG, EMPTY)]
    return ["+".join(s) for s in sets]


def call(svo, entry, world, key):
    """entry on `world` (a handle or None) with the faults `key` names; every other argument is good"""
    faults = set(key.split("+")) if key else set()
    lib = svo.lib
    prm = svo.trace_params(see_through=0x10000 if ST in faults else 6 if entry == "svo_trace_translucent" else 0,
                           semantics=2 if SEM in faults else 0, kernel=3 if KER in faults else 0)
    out = None if OUT in faults else FAKE
    n = -1 if NEG in faults else 0 if EMPTY in faults else 8            # a count, or a rectangle's width
    cams = (svo.Camera * 2)(svo.default_camera(1, 1, 128, 8, 8), svo.default_camera(1, 1, 128, 8, 8))
    if entry == "svo_trace":
        return lib.svo_trace(world, cams, prm, 0, 0, n, 8, out, None)
    if entry == "svo_trace_rows":
        return lib.svo_trace_rows(world, cams, prm, 0, 1, n, 1, out, None)
    if entry == "svo_trace_frames":
        return lib.svo_trace_frames(world, cams, 2, prm, 0, 0, n, 8, out, None)
    if entry == "svo_trace_rows_frames":
        return lib.svo_trace_rows_frames(world, cams, 2, prm, 0, 1, n, 1, out, None)
    if entry == "svo_trace_rays":
        return lib.svo_trace_rays(world, FAKE, FAKE, n, prm, out, None)
    if entry == "svo_trace_segments":
        return lib.svo_trace_segments(world, FAKE, FAKE, FAKE, n, prm, out, None)
    if entry == "svo_trace_translucent":
        return lib.svo_trace_translucent(world, cams, prm, 0, 0, n, 8, FAKE, out, None)
    if entry == "svo_trace_local_shadows":
        light = (C.c_float * 3)(10.0, 100.0, 10.0)
        return lib.svo_trace_local_shadows(world, cams, prm, light, light, 0, 0, n, 8, out, None)
    if entry == "svo_shadowmap_render":
        m = svo.ShadowMap()
        m.origin[:], m.direction[:], m.right[:], m.up[:] = (64.0, 300.0, 64.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)
        m.half_width = m.half_height = 100.0
        m.width = m.height = 64
        m.depth_dev = out
        return lib.svo_shadowmap_render(world, m, prm, None)
    if entry == "svo_world_locate":
        return lib.svo_world_locate(world, FAKE, n, prm, out, None)
    if entry == "svo_hit_ao":
        return lib.svo_hit_ao(world, cams, prm, 1.0, 0, 0, n, 8, FAKE, FAKE, out, None)
    if entry == "svo_hit_voxels":
        return lib.svo_hit_voxels(world, FAKE, n, out, None)
    if entry == "svo_tile_order":
        return lib.svo_tile_order(world, FAKE, out, n, None)
    if entry == "svo_trace_last_ray_count":
        return lib.svo_trace_last_ray_count(world, None, C.byref(C.c_uint64()) if out else None)
    raise KeyError(entry)


def observed(svo, entry):
    """{ faults: (status on a world that is not uploaded, status on the NULL world) } of the loaded library"""
    W = svo.World.create([dict(position=(0, 0, 0), size=128.0, depth=4, tree=np.array([L | 6], np.uint32), twig=np.zeros(0, np.uint16))], 1, 1, 1, 128)
    try:
        return {key: (call(svo, entry, W._h, key), call(svo, entry, None, key)) for key in fault_sets(entry)}
    finally:
        W.destroy()


def test_the_table_covers_every_entry_point_fault_and_pair():
    assert set(EXPECTED) == set(ENTRIES) and len(ENTRIES) == 14
    for entry, faults in ENTRIES.items():
        assert list(EXPECTED[entry]) == fault_sets(entry), entry
        n = len(faults)
        assert len(EXPECTED[entry]) == 1 + n + n * (n - 1) // 2 - (1 if NEG in faults else 0), entry
        assert all(status in (OK, INVALID, NOT_UPLOADED) for pair in EXPECTED[entry].values() for status in pair), entry
    # the example the table exists for
    assert EXPECTED["svo_trace_rays"][KER][0] == NOT_UPLOADED and EXPECTED["svo_world_locate"][KER][0] == INVALID


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_status_precedence(svo, entry):
    got = observed(svo, entry)
    wrong = {key: (got[key], want) for key, want in EXPECTED[entry].items() if got[key] != want}
    assert not wrong, f"{entry}: {{faults: (got, recorded)}} = {wrong}"

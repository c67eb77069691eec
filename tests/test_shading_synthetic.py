"""The shading stage (csrc/shade.hip) on synthetic G-buffers, against the float64 model of tests/shade_model.py.

The stage reads nothing but records, so no world is built: every buffer is made in numpy (shade_model.all_cases and friends, at
most 5000 records each) to reach what a terrain frame never produces - every material and shininess with a visible highlight, the
seam of the kernel's own power function, the spot cone's edges, points next to the eye, every combination of the shadow bits, and
every bit pattern of the packed record.

Tolerance (shade_model.within): |got - want| <= 1e-6 + 2e-5 |want| + K * 2^-23 * cond, cond = sum over the lights of
shininess * |specular term|.  K is not fitted to the kernel: the C oracle (float32, correctly rounded) needs K_oracle = 1.758 on
these buffers (tests/test_shade_model_cpu.py measures it), and the kernel's three 1-ulp normalisations and 1-ulp log2 / exp2 on the
way to the power make it K = ceil(4 K_oracle) = 8.  Largest |got - want| / tolerance measured on an MI355X with that K:
    svo_shade              0.273
    svo_shade_packed       0.273
    svo_shade_translucent  0.029
Everything else is exact: misses are {0,0,0,1}, NaN sits exactly on the rgb of NaN-normal hits, packed shading equals unpacked
shading bit for bit on cube and NaN normals, pack / unpack equal the integer model, refused calls write nothing."""
import ctypes as C

import numpy as np
import pytest

import shade_model as sm

pytestmark = pytest.mark.gpu
CASES = ["general_default", "general_gamma1", "general_gamma2.4", "highlight_point", "highlight_spot", "highlight_directional_0",
         "highlight_directional_2^-24", "highlight_directional_2^-12", "spot_cone", "near_eye"]
SENTINEL = np.float32(-12345.678)
PAD = 64                                            # float4s / words of sentinel behind every output


@pytest.fixture(scope="module")
def cases(svo):
    return sm.all_cases(svo)


def _shade(svo, cam, P, rect, g, packed=False, behind=None, absorption=0.0):
    """Run one of the three entry points over host records; the output buffer is sentinel-filled and its tail must survive."""
    n = rect[2] * rect[3]
    src = svo.DeviceBuffer.from_numpy(g)
    out = svo.DeviceBuffer.from_numpy(np.full((n + PAD) * 4, SENTINEL, np.float32))
    if behind is not None:
        bb = svo.DeviceBuffer.from_numpy(behind)
        svo.shade_translucent(cam, P, rect, src.ptr, bb.ptr, out.ptr, absorption=absorption)
    elif packed:
        svo.shade_packed(cam, P, rect, src.ptr, out.ptr)
    else:
        svo.shade(cam, P, rect, src.ptr, out.ptr)
    assert svo.lib.svo_stream_synchronize(None) == 0
    got = out.to_numpy(np.float32, (n + PAD) * 4)
    src.free(); out.free()
    if behind is not None:
        bb.free()
    assert np.all(got[n * 4:] == SENTINEL), "wrote past w*h pixels"
    return got[:n * 4].reshape(n, 4)


def _check(got, want, cond, g, what, capsys):
    """NaN exactly where the model has it, misses exactly {0,0,0,1}, everything else within the tolerance at K_GPU."""
    hit = (np.asarray(g).reshape(-1)["flags"] & sm.HIT) != 0
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN elsewhere than the model's"
    assert not np.isnan(want[:, 3]).any()
    assert np.all(got[~hit] == np.array([0.0, 0.0, 0.0, 1.0], np.float32)), f"{what}: a miss is not {{0,0,0,1}}"
    r = sm.within(got, want, cond, sm.K_GPU)
    worst = float(np.nanmax(r)) if r.size else 0.0
    with capsys.disabled():
        print(f"\n  {what:52s} |got - want| / tolerance(K={sm.K_GPU}) <= {worst:.3f}   K needed {sm.needed_K(got, want, cond):.3f}", end="")
    k = np.unravel_index(np.nanargmax(r), r.shape) if r.size else (0, 0)
    assert worst <= 1.0, f"{what}: record {k[0]} component {k[1]} got {got[k]} want {want[k]} cond {cond[k[0]]}"
    return worst


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("name", CASES)
def test_shade_matches_model(svo, cases, name, capsys):
    cam, P, rect, g = cases[name]
    want, cond = sm.shade(cam, P, rect, g)
    got = _shade(svo, cam, P, rect, g)
    _check(got, want, cond, g, f"svo_shade {name}", capsys)
    if name.startswith("highlight"):
        assert (cond > 0).mean() > 0.5


@pytest.mark.parametrize("name", CASES)
def test_shade_packed_matches_unpacked(svo, cases, name, capsys):
    """svo.h: identical colours from the 8-byte record.  Bit for bit wherever the record keeps its normal (the 26 cube normals and
    NaN); any other normal is replaced by the packed form's, and that is compared with the model of the unpacked words."""
    cam, P, rect, g = cases[name]
    words = sm.pack(g)
    got = _shade(svo, cam, P, rect, words, packed=True)
    plain = _shade(svo, cam, P, rect, g)
    keeps = sm.is_cube_or_nan(g) | ((g["flags"] & sm.HIT) == 0)
    assert keeps.mean() > 0.5
    assert np.array_equal(got[keeps].view(np.uint32), plain[keeps].view(np.uint32)), "packed shading differs from unpacked shading"
    back = sm.unpack(words)
    want, cond = sm.shade(cam, P, rect, back)
    _check(got, want, cond, back, f"svo_shade_packed {name}", capsys)


def test_zero_fields_mean_the_defaults(svo, cases):
    cam, P, rect, g = cases["general_default"]
    assert (P.eps, P.gamma, P.near_plane, P.far_plane) == (1.0 / 8192.0, float(np.float32(2.2)), 0.125, 8192.0)
    Z = sm.copy_params(P)
    Z.eps = Z.gamma = Z.near_plane = Z.far_plane = 0.0
    spelled = _shade(svo, cam, P, rect, g)
    assert _bits_equal(_shade(svo, cam, Z, rect, g), spelled)
    assert _bits_equal(_shade(svo, cam, Z, rect, sm.pack(g), packed=True), _shade(svo, cam, P, rect, sm.pack(g), packed=True))
    cam, P, rect, s, b = sm.translucent_case(svo)
    Z = sm.copy_params(P)
    Z.eps = Z.gamma = Z.near_plane = Z.far_plane = 0.0
    assert _bits_equal(_shade(svo, cam, Z, rect, s, behind=b, absorption=0.5), _shade(svo, cam, P, rect, s, behind=b, absorption=0.0))


@pytest.mark.parametrize("rect", [(57, 31, 1, 1), (130, 0, 1, 97), (0, 96, 131, 1)], ids=["1x1", "1xh", "wx1"])
def test_thin_rectangles(svo, cases, rect, capsys):
    """One pixel, one column at the image's right edge, one row at its bottom: k % w and k / w at their extremes."""
    cam, P, _, g = cases["general_gamma2.4"]
    n = rect[2] * rect[3]
    g = g[7:7 + n].copy()
    g["flags"][0] |= sm.HIT
    g["normal"][0] = sm.cube_normals()[4]
    want, cond = sm.shade(cam, P, rect, g)
    _check(_shade(svo, cam, P, rect, g), want, cond, g, f"svo_shade {rect}", capsys)
    back = sm.unpack(sm.pack(g))
    want, cond = sm.shade(cam, P, rect, back)
    _check(_shade(svo, cam, P, rect, sm.pack(g), packed=True), want, cond, back, f"svo_shade_packed {rect}", capsys)
    _check(_shade(svo, cam, P, rect, g, behind=np.zeros(n, sm.HIT_DTYPE)), *sm.shade(cam, P, rect, g), g, f"svo_shade_translucent {rect}", capsys)


@pytest.mark.parametrize("absorption", [0.0, 0.2])
def test_shade_translucent_matches_model(svo, absorption, capsys):
    cam, P, rect, s, b = sm.translucent_case(svo, dict(gamma=2.4))
    a = np.float32(absorption or 0.5)
    see = ((s["flags"] & sm.HIT) != 0) & ((s["flags"] & sm.SEE_THROUGH) != 0)
    bhit = (b["flags"] & sm.HIT) != 0
    x = b["t"] * a
    for part in (see & bhit, see & ~bhit, ~see & bhit & ((s["flags"] & sm.HIT) != 0), see & bhit & (x < 1), see & bhit & (x == 1),
                 see & bhit & (x > 1), see & bhit & ((b["flags"] & (sm.SHADOWED | sm.LOCAL_SHADOWS)) != 0)):
        assert part.sum() >= 20
    want, cond = sm.shade_translucent(cam, P, float(a), rect, s, b)
    got = _shade(svo, cam, P, rect, s, behind=b, absorption=absorption)
    _check(got, want, cond, s, f"svo_shade_translucent absorption {absorption}", capsys)
    plain = _shade(svo, cam, P, rect, s)
    assert np.array_equal(got[~see].view(np.uint32), plain[~see].view(np.uint32)), "a pixel without SVO_SEE_THROUGH is svo_shade's"
    assert np.array_equal(got[see & ~bhit].view(np.uint32), plain[see & ~bhit].view(np.uint32)), "nothing behind: the surface colour"


# ---- pack / unpack: exact ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_pack_and_unpack_equal_the_integer_model(svo, n):
    g = sm.pack_records(n)
    if n == 1:
        g["flags"] |= sm.HIT
    fill64, fill32 = np.uint64(0xA5A5A5A5DEADBEEF), np.uint32(0xDEADBEEF)
    src = svo.DeviceBuffer.from_numpy(g)
    packed = svo.DeviceBuffer.from_numpy(np.full(n + PAD, fill64, np.uint64))
    svo.gbuffer_pack(src.ptr, packed.ptr, n)
    assert svo.lib.svo_stream_synchronize(None) == 0
    words = packed.to_numpy(np.uint64, n + PAD)
    assert np.all(words[n:] == fill64), "svo_gbuffer_pack wrote past n"
    want = sm.pack(g)
    bad = np.nonzero(words[:n] != want)[0]
    assert bad.size == 0, f"record {bad[0]}: {g[bad[0]]} packs to {int(words[bad[0]]):#018x}, model {int(want[bad[0]]):#018x}"
    back = svo.DeviceBuffer.from_numpy(np.full((n + PAD) * 8, fill32, np.uint32))
    svo.gbuffer_unpack(packed.ptr, back.ptr, n)
    assert svo.lib.svo_stream_synchronize(None) == 0
    raw = back.to_numpy(np.uint32, (n + PAD) * 8)
    assert np.all(raw[n * 8:] == fill32), "svo_gbuffer_unpack wrote past n"
    got, model = raw[:n * 8].reshape(n, 8), sm.unpack(want).view(np.uint32).reshape(n, 8)
    bad = np.nonzero((got != model).any(axis=1))[0]
    assert bad.size == 0, f"word {int(want[bad[0]]):#018x} unpacks to {got[bad[0]]}, model {model[bad[0]]}"
    for buf in (src, packed, back):
        buf.free()
    if n >= 255:
        zero = ((g["flags"] & sm.HIT) != 0) & (g["normal"] == 0).all(axis=1)        # a hit with the normal (0,0,0): NaN, pinned
        assert zero.any() and np.all(got[zero][:, 1:4] == 0x7FC00000)
        stale = ((g["flags"] & sm.HIT) == 0) & (g["normal"] != 0).any(axis=1)
        assert stale.any() and not got[stale][:, 1:4].any()


# ---- arguments ---------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(svo, cases):
    """Every SVO_ERR_INVALID_ARG branch of the five entry points, and the empty calls that are SVO_OK.  Every pointer that is
    not NULL is a real buffer large enough for the call as it would run, so nothing here can fault."""
    cam, P, rect, g = cases["general_default"]
    x0, y0, w, h = rect
    n = w * h
    fill = np.full(n * 8, 0xDEADBEEF, np.uint32)                     # n float4 = n/2 records = n words: enough for every role
    src, behind = svo.DeviceBuffer.from_numpy(g), svo.DeviceBuffer.from_numpy(g)
    words = svo.DeviceBuffer.from_numpy(sm.pack(g))
    out = svo.DeviceBuffer.from_numpy(fill)
    INVALID, OK = -1, 0
    lib = svo.lib

    def camera(width=cam.width, height=cam.height):
        c = type(cam)()
        C.memmove(C.byref(c), C.byref(cam), C.sizeof(c))
        c.width, c.height = width, height
        return C.byref(c)
    good = dict(cam=C.byref(cam), P=C.byref(P), x0=x0, y0=y0, w=w, h=h, src=src.ptr, out=out.ptr)
    bad = [dict(cam=None), dict(P=None), dict(src=None), dict(out=None), dict(w=-1), dict(h=-1), dict(x0=-1), dict(y0=-1),
           dict(w=-3, h=-5), dict(cam=camera(width=0)), dict(cam=camera(width=-131)), dict(cam=camera(height=0)), dict(cam=camera(height=-1))]
    calls = []
    for change in bad + [dict(w=0), dict(h=0), dict(w=0, h=0)]:
        a = dict(good, **change)
        want = OK if change in (dict(w=0), dict(h=0), dict(w=0, h=0)) else INVALID
        calls.append((f"svo_shade {change}", want, lambda a=a: lib.svo_shade(a["cam"], a["P"], a["x0"], a["y0"], a["w"], a["h"], a["src"], a["out"], None)))
        a = dict(a, src=words.ptr if a["src"] else None)
        calls.append((f"svo_shade_packed {change}", want, lambda a=a: lib.svo_shade_packed(a["cam"], a["P"], a["x0"], a["y0"], a["w"], a["h"], a["src"], a["out"], None)))
        a = dict(good, **change)
        calls.append((f"svo_shade_translucent {change}", want,
                      lambda a=a: lib.svo_shade_translucent(a["cam"], a["P"], 0.2, a["x0"], a["y0"], a["w"], a["h"], a["src"], behind.ptr, a["out"], None)))
    a = good
    for absorption in (-0.1, -1e-30, float("nan"), float("-inf")):
        calls.append((f"svo_shade_translucent absorption {absorption}", INVALID,
                      lambda x=absorption: lib.svo_shade_translucent(a["cam"], a["P"], x, x0, y0, w, h, src.ptr, behind.ptr, out.ptr, None)))
    calls.append(("svo_shade_translucent behind NULL", INVALID, lambda: lib.svo_shade_translucent(a["cam"], a["P"], 0.2, x0, y0, w, h, src.ptr, None, out.ptr, None)))
    for name, fn, inp in (("svo_gbuffer_pack", lib.svo_gbuffer_pack, src), ("svo_gbuffer_unpack", lib.svo_gbuffer_unpack, words)):
        calls += [(f"{name} n < 0", INVALID, lambda fn=fn, inp=inp: fn(inp.ptr, out.ptr, -1, None)),
                  (f"{name} n = INT64_MIN", INVALID, lambda fn=fn, inp=inp: fn(inp.ptr, out.ptr, -2 ** 63, None)),
                  (f"{name} in NULL", INVALID, lambda fn=fn: fn(None, out.ptr, n // 4, None)),
                  (f"{name} out NULL", INVALID, lambda fn=fn, inp=inp: fn(inp.ptr, None, n // 4, None)),
                  (f"{name} n = 0", OK, lambda fn=fn, inp=inp: fn(inp.ptr, out.ptr, 0, None)),
                  (f"{name} n = 0, NULL", OK, lambda fn=fn: fn(None, None, 0, None))]
    for what, want, call in calls:
        assert call() == want, what
        if want == INVALID:
            assert svo.lib.svo_last_error(), what
    assert svo.lib.svo_stream_synchronize(None) == 0
    assert np.array_equal(out.to_numpy(np.uint32, n * 8), fill), "a refused or empty call wrote to its output"
    for buf in (src, behind, words, out):
        buf.free()

"""The float64 shading model (tests/shade_model.py) and its tolerance, checked on a CPU before the GPU tests lean on them
(tests/test_shading_synthetic.py): pixels worked by hand, the model against the C oracle on every synthetic G-buffer, mutations of
the model that the tolerance must catch, and the integer model of the packed record.

The C oracle is a float32 restatement with correctly rounded divisions and glibc's powf; it has no SVO_LOCAL_SHADOWS rule and no
0 = default substitution, so `oracle_shade` composes the first from three single-light runs and the cases spell the second out."""
import math

import numpy as np
import pytest

import shade_model as sm

F = np.float32
EPS = 1.0 / 8192.0


def _zero(light):
    for f in ("ambient", "diffuse", "specular"):
        getattr(light, f)[:] = [0.0, 0.0, 0.0]


def oracle_shade(oracle, cam, P, rect, g):
    """oracle.shade_image with svo.h's per-light shadow rule: a record with SVO_LOCAL_SHADOWS is the sum of three runs with one
    light each, SVO_SHADOWED replaced by that light's own bit (a light whose colours are all zero contributes exactly 0)."""
    g = np.asarray(g).reshape(-1)
    n = g.shape[0]
    out = oracle.shade_image(cam, P, rect, g).reshape(n, 4).astype(np.float64)
    local = ((g["flags"] & sm.HIT) != 0) & ((g["flags"] & sm.LOCAL_SHADOWS) != 0)
    if local.any():
        total = np.zeros((n, 3))
        for keep, bit in (("point", sm.SHADOWED_POINT), ("directional", sm.SHADOWED), ("spot", sm.SHADOWED_SPOT)):
            Q = sm.copy_params(P)
            for name in ("point", "directional", "spot"):
                if name != keep:
                    _zero(getattr(Q, name))
            h = g.copy()
            h["flags"] = np.where(g["flags"] & bit, g["flags"] | sm.SHADOWED, g["flags"] & ~np.uint16(sm.SHADOWED))
            total += oracle.shade_image(cam, Q, rect, h).reshape(n, 4)[:, :3]
        out[local, :3] = total[local]
    return out


@pytest.fixture(scope="module")
def cases(svo):
    return sm.all_cases(svo)


@pytest.fixture(scope="module")
def results(svo, oracle, cases):
    """name -> (oracle's rgba, model's rgba, cond), computed once."""
    out = {}
    for name, (cam, P, rect, g) in cases.items():
        want, cond = sm.shade(cam, P, rect, g)
        out[name] = (oracle_shade(oracle, cam, P, rect, g), want, cond)
    return out


# ---- pixels worked by hand ---------------------------------------------------------------------------------------
def _one_pixel(svo, flags=sm.HIT, material=1, t=5.0):
    """The 1x1 image looking straight down from (0, 10, 0): the pixel's ray IS the forward axis, the point is (0, 5 + eps, 0),
    the direction to the eye (0, 1, 0); normal +y; stone (diffuse .8, specular .5, shininess 8)."""
    cam = svo.make_camera((0.0, 10.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), 60.0, 1, 1)
    g = np.zeros(1, sm.HIT_DTYPE)
    g["t"], g["normal"], g["material"], g["flags"] = t, (0.0, 1.0, 0.0), material, flags
    return cam, g


def _only(svo, keep):
    P = svo.shade_defaults()
    for name in ("point", "directional", "spot"):
        if name != keep:
            _zero(getattr(P, name))
    return P


GAMMA = float(F(2.2))
DEPTH5 = (1.0 / (5.0 - EPS) - 8.0) / (1.0 / 8192.0 - 8.0)


def _f(v):
    return np.array([float(F(x)) for x in v])


def test_hand_worked_directional_pixel(svo):
    """Light straight down: l = v = h = (0, 1, 0), so the diffuse factor and the specular power are both 1."""
    P = _only(svo, "directional")
    P.directional.direction[:] = [0.0, -1.0, 0.0]
    P.directional.specular[:] = [0.1, 0.2, 0.3]
    cam, g = _one_pixel(svo)
    A, S = float(F(0.8)) ** GAMMA, float(F(0.5)) ** GAMMA
    rgba, cond = sm.shade(cam, P, (0, 0, 1, 1), g)
    want = (_f([0.2, 0.3, 0.4]) + _f([0.3, 0.3, 0.6])) * A + _f([0.1, 0.2, 0.3]) * S
    assert np.allclose(rgba[0, :3], want, rtol=1e-12) and abs(rgba[0, 3] - DEPTH5) < 1e-12
    assert abs(cond[0] - 8.0 * float(F(0.3)) * S) < 1e-12                   # shininess * the largest specular component
    g["flags"] = sm.HIT | sm.SHADOWED
    assert np.allclose(sm.shade(cam, P, (0, 0, 1, 1), g)[0][0, :3], _f([0.2, 0.3, 0.4]) * A, rtol=1e-12)
    g["flags"] = sm.HIT | sm.SHADOWED | sm.LOCAL_SHADOWS                    # the directional light keeps SVO_SHADOWED
    assert np.allclose(sm.shade(cam, P, (0, 0, 1, 1), g)[0][0, :3], _f([0.2, 0.3, 0.4]) * A, rtol=1e-12)
    g["flags"] = sm.SHADOWED | sm.FACE_NORMAL                               # not a hit
    rgba, cond = sm.shade(cam, P, (0, 0, 1, 1), g)
    assert rgba.tolist() == [[0.0, 0.0, 0.0, 1.0]] and cond[0] == 0.0


def _light_at_3_4(light):
    """5 away from the point (0, 5 + eps, 0) in the direction (0.6, 0.8, 0): n.l = 0.8, h = normalize(0.6, 1.8, 0),
    (v.h)^2 = 3.24 / 3.6 = 0.9, so the specular power at shininess 8 is 0.9^4 = 0.6561."""
    light.position[:] = [3.0, 9.0 + EPS, 0.0]


def test_hand_worked_point_pixel(svo):
    P = _only(svo, "point")
    _light_at_3_4(P.point)
    cam, g = _one_pixel(svo)
    A, S = float(F(0.8)) ** GAMMA, float(F(0.5)) ** GAMMA
    att = 1.0 / (1.0 + float(F(0.14)) * 5.0 + float(F(0.09)) * 25.0)
    want = (_f([0.1] * 3) * A + _f([0.5] * 3) * 0.8 * A + 0.6561 * S) * att
    rgba, cond = sm.shade(cam, P, (0, 0, 1, 1), g)
    assert np.allclose(rgba[0, :3], want, rtol=1e-9) and abs(rgba[0, 3] - DEPTH5) < 1e-12
    assert abs(cond[0] - 8.0 * 0.6561 * S * att) < 1e-9
    for flags, lit in ((sm.SHADOWED, 0), (sm.SHADOWED | sm.LOCAL_SHADOWS, 1), (sm.LOCAL_SHADOWS | sm.SHADOWED_POINT, 0),
                       (sm.LOCAL_SHADOWS | sm.SHADOWED_SPOT, 1), (sm.SHADOWED_POINT | sm.SHADOWED_SPOT, 1)):
        g["flags"] = sm.HIT | flags
        want = (_f([0.1] * 3) * A + lit * (_f([0.5] * 3) * 0.8 * A + 0.6561 * S)) * att
        assert np.allclose(sm.shade(cam, P, (0, 0, 1, 1), g)[0][0, :3], want, rtol=1e-9), flags


@pytest.mark.parametrize("cos_gamma, cos_phi, intensity", [(0.8, 0.9, 0.0), (0.7, 0.9, 0.5), (0.6, 0.8, 1.0)])
def test_hand_worked_spot_pixels(svo, cos_gamma, cos_phi, intensity):
    """The same geometry with the spotlight shining straight down: theta = dot(l, (0, 1, 0)) = 0.8, put at cos_gamma, at the
    midpoint and at cos_phi by moving the bounds (float32(0.8) is 1.2e-8 above 0.8: the clamp takes the first, the last is 1 - 6e-8)."""
    P = _only(svo, "spot")
    _light_at_3_4(P.spot)
    P.spot.direction[:] = [0.0, -1.0, 0.0]
    P.spot.cos_gamma, P.spot.cos_phi = cos_gamma, cos_phi
    cam, g = _one_pixel(svo)
    A, S = float(F(0.8)) ** GAMMA, float(F(0.5)) ** GAMMA
    att = 1.0 / (1.0 + float(F(0.045)) * 5.0 + float(F(0.0075)) * 25.0)
    light = _f([0.2, 0.8, 0.3])
    want = (light * A + (light * 0.8 * A + 0.6561 * S) * intensity) * att
    rgba, cond = sm.shade(cam, P, (0, 0, 1, 1), g)
    assert np.allclose(rgba[0, :3], want, rtol=1e-6, atol=1e-9)
    assert abs(cond[0] - 8.0 * 0.6561 * S * intensity * att) < 1e-6
    g["flags"] = sm.HIT | sm.LOCAL_SHADOWS | sm.SHADOWED_SPOT
    assert np.allclose(sm.shade(cam, P, (0, 0, 1, 1), g)[0][0, :3], light * A * att, rtol=1e-9)


def test_hand_worked_translucent_pixel(svo):
    """Water (diffuse .4, specular 1, shininess 100) at t1 = 4 over stone at t2 = 1 behind it, absorption 0.2: s = 0.2, the stone
    is shaded at t = 5, depth is the stone's.  Directional light straight down: every factor is 1."""
    P = _only(svo, "directional")
    P.directional.direction[:] = [0.0, -1.0, 0.0]
    P.directional.specular[:] = [0.1, 0.2, 0.3]
    cam, s = _one_pixel(svo, flags=sm.HIT | sm.SEE_THROUGH, material=6, t=4.0)
    _, b = _one_pixel(svo, material=1, t=1.0)

    def colour(diffuse, specular):
        return (_f([0.2, 0.3, 0.4]) + _f([0.3, 0.3, 0.6])) * float(F(diffuse)) ** GAMMA + _f([0.1, 0.2, 0.3]) * float(F(specular)) ** GAMMA
    water, stone = colour(0.4, 1.0), colour(0.8, 0.5)
    rgba, _ = sm.shade_translucent(cam, P, 0.2, (0, 0, 1, 1), s, b)
    assert np.allclose(rgba[0, :3], stone * (1.0 - float(F(0.2))) + water * float(F(0.2)), rtol=1e-7)
    assert abs(rgba[0, 3] - DEPTH5) < 1e-12
    rgba, _ = sm.shade_translucent(cam, P, 0.0, (0, 0, 1, 1), s, b)                  # 0 means 0.5
    assert np.allclose(rgba[0, :3], 0.5 * stone + 0.5 * water, rtol=1e-12)
    b["t"] = 7.0                                                                    # 7 * 0.2 clamps to 1: the water alone, the stone's depth
    rgba, _ = sm.shade_translucent(cam, P, 0.2, (0, 0, 1, 1), s, b)
    assert np.allclose(rgba[0, :3], water, rtol=1e-12) and abs(rgba[0, 3] - (1.0 / (11.0 - EPS) - 8.0) / (1.0 / 8192.0 - 8.0)) < 1e-12
    depth4 = (1.0 / (4.0 - EPS) - 8.0) / (1.0 / 8192.0 - 8.0)
    for sflags, bflags in ((sm.HIT, sm.HIT), (sm.HIT | sm.SEE_THROUGH, 0)):         # not see-through / nothing behind: the surface
        s["flags"], b["flags"] = sflags, bflags
        rgba, _ = sm.shade_translucent(cam, P, 0.2, (0, 0, 1, 1), s, b)
        assert np.allclose(rgba[0, :3], water, rtol=1e-12) and abs(rgba[0, 3] - depth4) < 1e-12


def test_power_of_zero(svo):
    x, y = np.array([0.0, 0.0, 1.0, 0.25, np.nan]), np.array([0.0, 3.0, 0.0, 0.5, 2.0])
    assert np.array_equal(sm.MODEL.power(x, y)[:4], [1.0, 0.0, 1.0, 0.5]) and np.isnan(sm.MODEL.power(x, y)[4])


def test_zero_means_default(svo):
    cam, P, rect, g = sm.general_case(svo)
    Z = sm.copy_params(P)
    Z.eps = Z.gamma = Z.near_plane = Z.far_plane = 0.0
    a, b = sm.shade(cam, P, rect, g), sm.shade(cam, Z, rect, g)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


# ---- the synthetic buffers are what they claim to be ---------------------------------------------------------
def test_inputs_cover_what_they_are_built_for(svo, cases):
    cam, P, rect, g = cases["general_default"]
    hit = (g["flags"] & sm.HIT) != 0
    assert 0.05 < 1.0 - hit.mean() < 0.15 and g.shape[0] == 3015 and g.shape[0] % 256 != 0
    assert set(np.unique(g["material"][hit])) == {0, 1, 2, 3, 4, 5, 6, 7, 8, 255, 0xFFFF}
    shadow_bits = sm.SHADOWED | sm.LOCAL_SHADOWS | sm.SHADOWED_POINT | sm.SHADOWED_SPOT
    assert set(np.unique(g["flags"][hit] & shadow_bits)) == set(sm.SHADOW_FLAG_SETS)
    codes = set(np.unique(sm.pack(g[hit]) >> np.uint64(56) & np.uint64(0x7F)))
    assert len(codes) == 27 and 0x15 not in codes                                   # 26 sign triples and the NaN code
    for light in ("point", "spot", "directional_0", "directional_2^-24", "directional_2^-12"):
        cam, P, rect, g = cases["highlight_" + light]
        T = sm.terms(cam, P, rect, g)
        name = light.split("_")[0]
        d = 1.0 - T["x_" + name]
        assert d.max() > 0.1
        if light == "directional_2^-12":                        # the aimed pixel itself
            assert np.min(np.abs(d / 2.0 ** -12 - 1.0)) < 1e-3
        else:
            assert d.min() < 2.0 ** -23
        assert np.sum((d > 1 / 64 - 1 / 512) & (d < 1 / 64)) > 20 and np.sum((d >= 1 / 64) & (d < 1 / 64 + 1 / 512)) > 20
        if name != "directional":
            for want in (2.0 ** -24, 2.0 ** -12, 1 / 64, 0.125):
                assert np.min(np.abs(d / want - 1.0)) < 1e-3, (light, want)
        bright = np.abs(T["spec_" + name]).max(axis=1) > 1e-3
        assert bright.mean() >= 0.2, (light, bright.mean())
        assert set(np.unique(T["shininess"][bright])) == set(sm.CUSTOM_SHININESS)
    cam, P, rect, g = cases["spot_cone"]
    theta, cg, cp = sm.terms(cam, P, rect, g)["theta"], float(P.spot.cos_gamma), float(P.spot.cos_phi)
    for part in (theta < cg - 1e-3, (theta > cg + 1e-3) & (theta < cp - 1e-3), theta > cp + 1e-3,
                 (np.abs(theta - cg) < 1e-6) & (theta < cg), (np.abs(theta - cg) < 1e-6) & (theta > cg),
                 (np.abs(theta - cp) < 1e-6) & (theta < cp), (np.abs(theta - cp) < 1e-6) & (theta > cp)):
        assert part.mean() > 0.05
    cam, P, rect, g = cases["near_eye"]
    s = g["t"] - F(P.eps)
    assert np.all(s != 0) and (s < 0).sum() >= 10 and np.all(s <= F(2.001e-3))
    assert (s == F(1e-3)).any() and ((s > F(0.9e-3)) & (s < F(1e-3))).sum() > 100 and ((s > F(1e-3)) & (s < F(1.1e-3))).sum() > 100


# ---- the model against the C oracle ------------------------------------------------------------------------------
def test_model_matches_oracle_with_K2(results, capsys):
    """Every component of every case within 1e-6 + 2e-5 |want| + 2 * 2^-23 * cond of the float64 model; NaN exactly on the rgb of
    the hits with a NaN normal.  K_oracle, the smallest K the oracle needs anywhere, is what the GPU tests' K = 4 K_oracle rests on."""
    k_oracle = 0.0
    for name, (got, want, cond) in results.items():
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        r = sm.within(got, want, cond, 2.0)
        k = sm.needed_K(got, want, cond)
        k_oracle = max(k_oracle, k)
        with capsys.disabled():
            print(f"\n  {name:28s} largest |oracle - model| / tolerance(K=2) {np.nanmax(r):.3f}   K needed {k:.3f}", end="")
        assert np.nanmax(r) <= 1.0, (name, np.nanmax(r))
    with capsys.disabled():
        print(f"\n  K_oracle = {k_oracle:.3f} (recorded {sm.K_ORACLE}); the GPU tests use K = {sm.K_GPU}")
    assert k_oracle <= 2.0
    assert k_oracle <= sm.K_ORACLE, "shade_model.K_ORACLE must be re-measured"
    assert sm.K_GPU == math.ceil(4.0 * sm.K_ORACLE)


def test_fixed_tolerance_alone_is_not_enough(results):
    """The point of the cond term: on the highlights the correctly rounded float32 oracle itself misses 2e-5 relative."""
    got, want, cond = results["highlight_point"]
    assert np.nanmax(sm.within(got, want, cond, 0.0)) > 2.0


# ---- the tolerance has teeth: a wrong model must fail against the oracle --------------------------------------------
class SwappedLocalShadows(sm.ShadeModel):
    def lit(self, flags):
        p, d, s = super().lit(flags)
        return s, d, p


class SpotUnclampedAbove(sm.ShadeModel):
    def spot_intensity(self, x):
        return np.where(x < 0.0, 0.0, x)


class Shinier(sm.ShadeModel):
    def shininess(self, table, mi):
        return table[mi] * 1.01


class NextMaterial(sm.ShadeModel):
    def material_index(self, material):
        return (super().material_index(material) + 1) % 8


class Gamma2(sm.ShadeModel):
    def gamma(self, g):
        return 2.0


class PointAtT(sm.ShadeModel):
    def sample_distance(self, t, eps):
        return t


class DepthAtT(sm.ShadeModel):
    def depth_distance(self, p, eye, t, eps):
        return np.abs(t)


class SeriesWithoutCubicTerm(sm.ShadeModel):
    def log2(self, x):
        d = 1.0 - x
        return np.where(d < 1 / 64, -(d + d * d / 2.0) / math.log(2.0), np.log2(x))


MUTATIONS = [(SwappedLocalShadows, "general_default", slice(0, 3)), (SpotUnclampedAbove, "spot_cone", slice(0, 3)),
             (Shinier, "highlight_point", slice(0, 3)), (NextMaterial, "general_default", slice(0, 3)),
             (Gamma2, "general_default", slice(0, 3)), (PointAtT, "near_eye", slice(0, 3)), (DepthAtT, "near_eye", slice(3, 4)),
             (SeriesWithoutCubicTerm, "highlight_point", slice(0, 3))]


@pytest.mark.parametrize("mutant, case, components", MUTATIONS, ids=[m[0].__name__ for m in MUTATIONS])
def test_tolerance_catches(cases, results, mutant, case, components):
    cam, P, rect, g = cases[case]
    want, cond = mutant().shade(cam, P, rect, g)
    r = sm.within(results[case][0], want, cond, 2.0)[:, components]
    caught = np.nan_to_num(r, nan=0.0).max(axis=1) > 1.0
    assert caught.mean() >= 0.01, f"{mutant.__name__}: {caught.sum()} of {caught.size} records beyond the tolerance"


# ---- the packed record -------------------------------------------------------------------------------------------
def test_pack_layout():
    g = np.zeros(4, sm.HIT_DTYPE)
    g["t"] = [1.5, 2.0, -0.0, np.nan]
    g["normal"] = [(-1.0, 0.0, 1.0), (np.nan, 1.0, 0.0), (0.0, -0.0, -2.5), (0.0, 0.0, 0.0)]
    g["material"] = [0x1234, 0xFFFF, 0, 1]
    g["flags"] = [0x7F01, 0x80FF, 0x00A5, 0x8001]
    w = sm.pack(g)
    assert (w & np.uint64(0xFFFFFFFF)).tolist() == [0x3FC00000, 0x40000000, 0x80000000, 0x7FC00000]
    #            material | low flag byte << 16 | code << 24 | error << 31
    assert (w >> np.uint64(32)).tolist() == [0x1234 | 0x01 << 16 | (0 | 1 << 2 | 2 << 4) << 24,
                                              0xFFFF | 0xFF << 16 | 1 << 30 | 1 << 31,
                                              0 | 0xA5 << 16 | (1 | 1 << 2 | 0 << 4) << 24,
                                              1 | 0x01 << 16 | (1 | 1 << 2 | 1 << 4) << 24 | 1 << 31]
    u = sm.unpack(w)
    assert u["flags"].tolist() == [0x0001, 0x80FF, 0x00A5, 0x8001] and u["material"].tolist() == [0x1234, 0xFFFF, 0, 1]
    assert u["normal"][0].view(np.uint32).tolist() == [0xBF3504F3, 0, 0x3F3504F3]
    assert np.isnan(u["normal"][1]).all() and u["normal"][2].view(np.uint32).tolist() == [0, 0, 0xBF800000]
    assert np.isnan(u["normal"][3]).all()                               # a hit with the normal (0,0,0) does not round-trip
    assert not u["chunk"].any() and not u["node"].any() and not u["cell"].any()


def test_pack_unpack_round_trip():
    g = sm.pack_records(5000)
    u = sm.unpack(sm.pack(g))
    assert np.array_equal(u["t"].view(np.uint32), g["t"].view(np.uint32)) and np.array_equal(u["material"], g["material"])
    assert np.array_equal(u["flags"], g["flags"] & (0xFF | sm.ERR))
    hit = (g["flags"] & sm.HIT) != 0
    assert not u["normal"][~hit].view(np.uint32).any()
    keeps = hit & sm.is_cube_or_nan(g)
    nan = np.isnan(g["normal"]).any(axis=1)
    assert (keeps & ~nan).sum() > 500 and (keeps & nan).sum() > 100 and (hit & ~keeps).sum() > 500
    assert np.isnan(u["normal"][keeps & nan]).all()
    assert np.array_equal(u["normal"][keeps & ~nan].view(np.uint32), g["normal"][keeps & ~nan].view(np.uint32))
    cube = np.zeros(27, sm.HIT_DTYPE)                                   # the 26 vectors and NaN, as hits: the identity
    cube["normal"][:26], cube["normal"][26], cube["flags"] = sm.cube_normals(), np.nan, sm.HIT
    assert sm.is_cube_or_nan(cube).all() and len(set(sm.pack(cube).tolist())) == 27
    back = sm.unpack(sm.pack(cube))["normal"]
    assert np.array_equal(back[:26].view(np.uint32), cube["normal"][:26].view(np.uint32)) and np.isnan(back[26]).all()

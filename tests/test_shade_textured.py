"""svo_hit_uv and svo_shade_textured on the GPU: the reference's leafUV bit for bit against the host model
(tests/hit_voxels_model.py) under both semantics, the texel the kernel samples (an atlas whose texels encode their own coordinates),
exact equality with svo_shade on a flat atlas, the float64 shading model (tests/shade_model.py) fed the decoded texels as albedo -
judged by that file's own `within` at the K svo_shade is held to -, and specular_dev == NULL.  Atlases are made with numpy."""
import numpy as np
import pytest

import hit_voxels_model as M
import shade_model as sm

pytestmark = pytest.mark.gpu
F = np.float32
EPS = {0: F(1.0 / 8192.0), 1: F(1.0 / 4096.0)}
RECT = (0, 0) + M.IMAGE
N = M.IMAGE[0] * M.IMAGE[1]


class Frame:
    """One traced frame kept on the device: its records, their boxes, and host copies of both."""

    def __init__(self, svo, W, cam, **kw):
        self.svo, self.cam = svo, cam
        self.gbuffer, self.voxels = svo.DeviceBuffer(N * 32), svo.DeviceBuffer(N * 32)
        W.trace(cam, svo.trace_params(**kw), RECT, self.gbuffer.ptr)
        W.hit_voxels(self.gbuffer.ptr, N, self.voxels.ptr)
        assert svo.lib.svo_stream_synchronize(None) == 0
        self.g, self.v = self.gbuffer.to_numpy(svo.HIT_DTYPE, N), self.voxels.to_numpy(svo.VOXEL_DTYPE, N)
        self.hit = (self.v["flags"] & M.INSIDE) != 0
        assert self.hit.sum() >= 300 and np.array_equal(self.hit, (self.g["flags"] & 1) != 0)

    def uv(self, eps):
        out = self.svo.DeviceBuffer.from_numpy(np.full(N * 2 + 16, -7.0, F))
        self.svo.hit_uv(self.cam, float(eps), RECT, self.gbuffer.ptr, self.voxels.ptr, out.ptr)
        assert self.svo.lib.svo_stream_synchronize(None) == 0
        got = out.to_numpy(F, N * 2 + 16)
        out.free()
        assert np.all(got[N * 2:] == F(-7.0)), "wrote past w*h pixels"
        return got[:N * 2].reshape(N, 2)

    def model_uv(self, eps):
        return M.hit_uv(np.array(self.cam.eye, F)[None], M.camera_dirs(self.cam), self.g, self.v, eps)

    def shade(self, P, atlas=None):
        out = self.svo.DeviceBuffer.from_numpy(np.full((N + 16) * 4, -7.0, F))
        if atlas is None:
            self.svo.shade(self.cam, P, RECT, self.gbuffer.ptr, out.ptr)
        else:
            self.svo.shade_textured(self.cam, P, atlas, RECT, self.gbuffer.ptr, self.voxels.ptr, out.ptr)
        assert self.svo.lib.svo_stream_synchronize(None) == 0
        got = out.to_numpy(F, (N + 16) * 4)
        out.free()
        assert np.all(got[N * 4:] == F(-7.0)), "wrote past w*h pixels"
        return got[:N * 4].reshape(N, 4)

    def free(self):
        self.gbuffer.free()
        self.voxels.free()


@pytest.fixture(scope="module")
def worlds(svo):
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    out = {}
    for name, (w, h, d, cs, ccm, _, _) in M.WORLDS.items():
        out[name] = svo.World.create(M.make_chunks(svo, name), w, h, d, cs, ccm)
        out[name].upload(0)
    yield out
    for W in out.values():
        W.destroy()


def upload_atlas(svo, diffuse, specular=None):
    """-> (svo.Atlas, the device buffers to free); images are uint8 [height][width][3], row 0 at v = 0."""
    bufs = [svo.DeviceBuffer.from_numpy(np.ascontiguousarray(diffuse, np.uint8))]
    if specular is not None:
        bufs.append(svo.DeviceBuffer.from_numpy(np.ascontiguousarray(specular, np.uint8)))
    return svo.Atlas(bufs[0].ptr, bufs[1].ptr if specular is not None else None, diffuse.shape[1], diffuse.shape[0]), bufs


@pytest.mark.parametrize("semantics", [0, 1])
@pytest.mark.parametrize("name", sorted(M.WORLDS))
def test_uv_equals_the_model(svo, worlds, name, semantics):
    for view, cam in M.cameras(svo, name).items():
        f = Frame(svo, worlds[name], cam, semantics=semantics, kernel=svo.KERNEL_LITERAL)
        got, want = f.uv(EPS[semantics]), f.model_uv(EPS[semantics])
        bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, f"{name}/{view}/semantics {semantics}: {bad.size} UVs differ, first {bad[:4]}: got {got[bad[:4]]} want {want[bad[:4]]}"
        assert not got[~f.hit].any()
        # the hits lie on a face of their box: the tile coordinate is not the nudged zero everywhere
        iuv = want[f.hit] * F(256) - np.floor(want[f.hit] * F(256))
        assert (iuv.max(axis=1) > 0.01).mean() > 0.9
        if semantics == 0:                                      # eps == 0 means 1/8192
            assert np.array_equal(f.uv(0.0).view(np.uint32), got.view(np.uint32))
        f.free()


def ambient_only(svo):
    """gamma 1 and nothing lit but the point light's ambient term, unattenuated: rgb is the decoded diffuse texel."""
    P = svo.shade_defaults()
    for light in (P.point, P.directional, P.spot):
        for term in ("ambient", "diffuse", "specular"):
            getattr(light, term)[:] = [0.0, 0.0, 0.0]
    P.point.ambient[:] = [1.0, 1.0, 1.0]
    for light in (P.point, P.spot):
        light.constant, light.linear, light.quadratic = 1.0, 0.0, 0.0
    P.gamma = 1.0
    return P


@pytest.mark.parametrize("name", ["grid_2x1x2_d6", "inexact_100_d5"])
def test_identity_atlas_recovers_the_models_texel(svo, worlds, name):
    """Texel (x, y) of a 1024 x 512 atlas holds (x & 255, y & 255, x >> 8 | (y >> 8) << 4).  SVO_NORMAL_FACE records: no NaN normal
    reaches a zeroed term.  round(rgb * 255) then names exactly the model's texel for every hit pixel."""
    width, height = 1024, 512
    y, x = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    image = np.stack([x & 255, y & 255, (x >> 8) | ((y >> 8) << 4)], axis=2).astype(np.uint8)
    atlas, bufs = upload_atlas(svo, image)
    P = ambient_only(svo)
    for view, cam in M.cameras(svo, name).items():
        f = Frame(svo, worlds[name], cam, normal_mode=svo.NORMAL_FACE, shadow=True, kernel=svo.KERNEL_LITERAL)
        rgba = f.shade(P, atlas)
        assert np.all(rgba[~f.hit] == np.array([0, 0, 0, 1], F))
        code = np.round(rgba[f.hit, :3].astype(np.float64) * 255.0).astype(np.int64)
        assert np.all(np.abs(rgba[f.hit, :3].astype(np.float64) * 255.0 - code) < 1e-3)
        gx, gy = code[:, 0] | ((code[:, 2] & 15) << 8), code[:, 1] | ((code[:, 2] >> 4) << 8)
        wx, wy = M.texel_index(f.model_uv(EPS[0])[f.hit], width, height)
        bad = np.nonzero((gx != wx) | (gy != wy))[0]
        assert bad.size == 0, f"{name}/{view}: {bad.size} texels differ, first got {gx[bad[:4]], gy[bad[:4]]} want {wx[bad[:4]], wy[bad[:4]]}"
        assert np.unique(wx * height + wy).size >= 8, "the frame samples a handful of texels only"
        f.free()
    for b in bufs:
        b.free()


@pytest.mark.parametrize("byte", [137, 0, 255])
def test_flat_atlas_equals_svo_shade(svo, worlds, byte):
    """A flat atlas of byte value b gives, bit for bit, svo_shade's image with every material's diffuse and specular at b / 255.0f."""
    atlas, bufs = upload_atlas(svo, np.full((24, 40, 3), byte, np.uint8))
    P = svo.shade_defaults()
    Q = sm.copy_params(P)
    for m in Q.materials:
        m.diffuse[:] = [float(F(byte) / F(255.0))] * 3
        m.specular[:] = [float(F(byte) / F(255.0))] * 3
    for view, cam in M.cameras(svo, "grid_2x1x2_d6").items():
        f = Frame(svo, worlds["grid_2x1x2_d6"], cam, shadow=True)
        got, want = f.shade(P, atlas), f.shade(Q)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        assert np.all((got.view(np.uint32) == want.view(np.uint32)) | nan), f"{view}: textured shading of a flat atlas differs from svo_shade"
        assert (~nan[f.hit]).all(axis=1).sum() > 200
        f.free()
    bufs[0].free()


def test_general_atlas_matches_the_float64_model(svo, worlds, capsys):
    """Random diffuse and specular atlases, the reference's lights, shadows and local shadow bits as traced.  The model is
    shade_model.ShadeModel unchanged: per sampled texel it shades the frame with every material's colours set to that texel's
    bytes / 255 (the kernel decodes pow(byte / 255.0f, gamma) in float), and the texel's pixels are taken from that image."""
    rng = np.random.default_rng(77)
    width, height = 1024, 512
    diffuse, specular = rng.integers(0, 256, (height, width, 3), np.uint8), rng.integers(0, 256, (height, width, 3), np.uint8)
    atlas, bufs = upload_atlas(svo, diffuse, specular)
    P = svo.shade_defaults()
    worst = 0.0
    for view, cam in M.cameras(svo, "grid_2x1x2_d6").items():
        f = Frame(svo, worlds["grid_2x1x2_d6"], cam, normal_mode=svo.NORMAL_FACE, shadow=True)
        got = f.shade(P, atlas)
        tx, ty = M.texel_index(f.model_uv(EPS[0]), width, height)
        want, cond = sm.shade(cam, P, RECT, f.g)                 # (misses; every hit is overwritten below)
        texels = np.unique(np.stack([tx[f.hit], ty[f.hit]], axis=1), axis=0)
        assert 8 <= texels.shape[0] <= 64
        for x, y in texels:
            Q = sm.copy_params(P)
            for m in Q.materials:
                m.diffuse[:] = [float(F(b) / F(255.0)) for b in diffuse[y, x]]
                m.specular[:] = [float(F(b) / F(255.0)) for b in specular[y, x]]
            w1, c1 = sm.shade(cam, Q, RECT, f.g)
            rows = f.hit & (tx == x) & (ty == y)
            want[rows], cond[rows] = w1[rows], c1[rows]
        assert not np.isnan(want).any() and np.all(got[~f.hit] == np.array([0, 0, 0, 1], F))
        r = sm.within(got, want, cond, sm.K_GPU)
        k = np.unravel_index(np.argmax(r), r.shape)
        worst = max(worst, float(r.max()))
        assert r.max() <= 1.0, f"{view}: pixel {k[0]} component {k[1]} got {got[k]} want {want[k]} cond {cond[k[0]]}"
        f.free()
    with capsys.disabled():
        print(f"\n  svo_shade_textured: |got - want| / tolerance(K={sm.K_GPU}) <= {worst:.3f}", end="")
    for b in bufs:
        b.free()


def test_null_specular_means_the_diffuse_image(svo, worlds):
    rng = np.random.default_rng(5)
    image = rng.integers(0, 256, (300, 700, 3), np.uint8)       # (no power of two: the row pitch is width * 3 bytes)
    once, bufs1 = upload_atlas(svo, image)
    twice, bufs2 = upload_atlas(svo, image, image)
    P = svo.shade_defaults()
    cam = M.cameras(svo, "grid_neg_2x2x2_d5")["above"]
    f = Frame(svo, worlds["grid_neg_2x2x2_d5"], cam, normal_mode=svo.NORMAL_FACE, shadow=True)
    a, b = f.shade(P, once), f.shade(P, twice)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and not np.isnan(a).any()
    inverted, bufs3 = upload_atlas(svo, image, 255 - image)
    assert not np.array_equal(f.shade(P, inverted), a)          # the specular image is read when it is given
    f.free()
    for buf in bufs1 + bufs2 + bufs3:
        buf.free()

"""svo_shade_sky and svo_frame_rgba8 on the GPU, held bit for bit to the host model (tests/sky_model.py): the texel the nearest filter
names (faces whose texels encode their own coordinates), the linear filter on random faces of size 37, 2 and 1, flat faces, what is
NOT written (hit pixels, every depth, everything behind w*h pixels), packed records, a sub-rectangle, the RGBA8 conversion on crafted
values and on a frame, and trace -> shade -> sky -> rgba8 end to end.  64 x 48 images of one small world; cameras from sky_model."""
import numpy as np
import pytest

import sky_model as S

pytestmark = pytest.mark.gpu
F = np.float32
W_, H_ = S.IMAGE
N = W_ * H_
FULL = (0, 0, W_, H_)
SENTINEL = F(-7.0)
PAD = 16                                                        # pixels of sentinel behind the image


def sync(svo):
    assert svo.lib.svo_stream_synchronize(None) == 0


class Frame:
    """One traced rectangle kept on the device: its records (both forms), host copies, the model's directions, and svo_shade's image."""

    def __init__(self, svo, world, cam, semantics, rect=FULL):
        self.svo, self.cam, self.rect = svo, cam, rect
        self.n = rect[2] * rect[3]
        self.gbuffer, self.packed = svo.DeviceBuffer(self.n * 32), svo.DeviceBuffer(self.n * 8)
        world.trace(cam, svo.trace_params(shadow=True, semantics=semantics), rect, self.gbuffer.ptr)
        svo.gbuffer_pack(self.gbuffer.ptr, self.packed.ptr, self.n)
        sync(svo)
        self.g = self.gbuffer.to_numpy(svo.HIT_DTYPE, self.n)
        self.hit = (self.g["flags"] & 1) != 0
        self.dirs = S.camera_dirs(cam, rect)
        self.P = svo.shade_defaults()
        self.base = self.shaded()

    def shaded(self, sky=None, packed=False):
        """svo_shade into a buffer with a sentinel behind the image, then (sky given) svo_shade_sky over it.  With a sky, asserts what
        must NOT have been written: hit pixels byte for byte, the depth of every pixel, the sentinel."""
        svo = self.svo
        out = svo.DeviceBuffer.from_numpy(np.full((self.n + PAD) * 4, SENTINEL, F))
        svo.shade(self.cam, self.P, self.rect, self.gbuffer.ptr, out.ptr)
        if sky is not None:
            svo.shade_sky(self.cam, sky, self.rect, out.ptr, gbuffer_ptr=None if packed else self.gbuffer.ptr, packed_ptr=self.packed.ptr if packed else None)
        sync(svo)
        got = out.to_numpy(F, (self.n + PAD) * 4)
        out.free()
        assert np.all(got[self.n * 4:] == SENTINEL), "wrote past w*h pixels"
        got = got[:self.n * 4].reshape(self.n, 4)
        if sky is None:
            assert np.all(got[~self.hit] == np.array([0, 0, 0, 1], F))
        else:
            assert np.array_equal(got[self.hit].view(np.uint32), self.base[self.hit].view(np.uint32)), "a hit pixel was written"
            assert np.all(got[~self.hit, 3] == F(1.0)), "the depth of a sky pixel was written"
        return got

    def free(self):
        self.gbuffer.free()
        self.packed.free()


class DeviceSky:
    def __init__(self, svo, faces):
        self.faces = np.ascontiguousarray(faces, np.uint8)
        self.size = self.faces.shape[1]
        self.buf = svo.DeviceBuffer.from_numpy(self.faces)
        self.svo = svo

    def sky(self, filter):
        step = self.size * self.size * 3
        return self.svo.Sky([self.buf.ptr + f * step for f in range(6)], self.size, filter)

    def free(self):
        self.buf.free()


@pytest.fixture(scope="module")
def world(svo):
    import hit_voxels_model as M
    if svo.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests need the MI355X")
    w, h, d, cs, ccm, _, _ = S.WORLDS[S.WORLD]
    W = svo.World.create(M.make_chunks(svo, S.WORLD), w, h, d, cs, ccm)
    W.upload(0)
    yield W
    W.destroy()


@pytest.fixture(scope="module")
def frames(svo, world):
    out = {}
    for name, (cam, all_sky, semantics) in S.all_cameras(svo).items():
        out[name] = Frame(svo, world, cam, semantics)
        if all_sky:
            assert not out[name].hit.any(), f"{name}: an all-sky view hits the world"
    yield out
    for f in out.values():
        f.free()


def mixed_view(frames):
    """The mixed view the tests of both kinds of pixel run on: at least 300 hit and 300 miss pixels."""
    ok = [k for k in ("above", "front") if frames[k].hit.sum() >= 300 and (~frames[k].hit).sum() >= 300]
    assert ok, {k: int(frames[k].hit.sum()) for k in ("above", "front")}
    return frames[ok[0]]


def test_every_face_is_named(frames):
    named = np.zeros(6, np.int64)
    for f in frames.values():
        face, _, _ = S.face_coords(f.dirs)
        assert np.all(face >= 0)
        named += np.bincount(face[~f.hit], minlength=6)
    assert named.min() >= 50, named
    mixed_view(frames)


def test_nearest_filter_names_the_models_texel(svo, frames):
    """Texel (x, y) of face f holds (x, y, f): round(rgb * 255) of every sky pixel of every camera is exactly the model's."""
    faces = S.identity_faces(256)
    D = DeviceSky(svo, faces)
    for name, f in frames.items():
        got = f.shaded(D.sky(svo.SKY_NEAREST))
        sky = ~f.hit
        scaled = got[sky, :3].astype(np.float64) * 255.0
        code = np.round(scaled).astype(np.int64)
        assert np.all(np.abs(scaled - code) < 1e-3)
        face, s, t = S.face_coords(f.dirs[sky])
        x, y = S.nearest_index(s, t, 256)
        bad = np.nonzero((code[:, 0] != x) | (code[:, 1] != y) | (code[:, 2] != face))[0]
        assert bad.size == 0, f"{name}: {bad.size} texels differ, first got {code[bad[:4]]} want {x[bad[:4]], y[bad[:4]], face[bad[:4]]}"
        want = S.shade_sky(f.base, f.g, f.dirs, faces, S.NEAREST)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.unique(np.concatenate([S.face_coords(f.dirs[~f.hit])[0] for f in frames.values()])).size == 6
    D.free()


@pytest.mark.parametrize("size", [37, 2, 1])
def test_linear_filter_equals_the_model_bit_for_bit(svo, frames, size):
    faces = S.random_faces(size, 500 + size)
    D = DeviceSky(svo, faces)
    for name, f in frames.items():
        got = f.shaded(D.sky(svo.SKY_LINEAR))
        want = S.shade_sky(f.base, f.g, f.dirs, faces, S.LINEAR)
        sky = ~f.hit
        bad = np.nonzero((got[sky].view(np.uint32) != want[sky].view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, f"{name}, size {size}: {bad.size} of {int(sky.sum())} sky pixels differ, first got {got[sky][bad[:3]]} want {want[sky][bad[:3]]}"
        assert not np.isnan(got[sky]).any()
        if size > 1:
            assert np.unique(got[sky, 0]).size > 20, "the frame samples a handful of colours only"
    D.free()


@pytest.mark.parametrize("filter", [S.LINEAR, S.NEAREST], ids=["linear", "nearest"])
@pytest.mark.parametrize("byte", [137, 255, 0])
def test_flat_sky_is_exactly_its_byte(svo, frames, byte, filter):
    D = DeviceSky(svo, S.flat_faces(5, byte))
    want = F(byte) / F(255)
    for name in ("corner", "+Y", "above", "front"):
        f = frames[name]
        got = f.shaded(D.sky(filter))
        assert np.all(got[~f.hit, :3].view(np.uint32) == np.array([want], F).view(np.uint32)[0]), name
    D.free()


def test_what_is_not_written(svo, frames):
    """Frame.shaded asserts it on every call; here on the mixed view, with the counts that keep it from passing vacuously."""
    f = mixed_view(frames)
    D = DeviceSky(svo, S.random_faces(8, 3))
    before = f.base
    after = f.shaded(D.sky(svo.SKY_LINEAR))
    hit, sky = f.hit, ~f.hit
    assert hit.sum() >= 300 and sky.sum() >= 300
    assert np.array_equal(after[hit].view(np.uint8), before[hit].view(np.uint8))
    assert np.all(before[sky] == np.array([0, 0, 0, 1], F)) and np.all(after[sky, 3] == F(1.0))
    assert (after[sky, :3] != 0).any(axis=1).mean() > 0.99, "the sky pixels were not written"
    D.free()


@pytest.mark.parametrize("filter", [S.LINEAR, S.NEAREST], ids=["linear", "nearest"])
def test_packed_records_give_the_same_image(svo, frames, filter):
    D = DeviceSky(svo, S.random_faces(37, 9))
    for name in ("above", "front", "corner"):
        f = frames[name]
        a, b = f.shaded(D.sky(filter)), f.shaded(D.sky(filter), packed=True)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    D.free()


def test_a_sub_rectangle_equals_the_crop(svo, world, frames):
    x0, y0, w, h = rect = (5, 7, 40, 30)
    D = DeviceSky(svo, S.random_faces(37, 21))
    for name in ("above", "front", "corner", "-X"):
        cam, _, semantics = S.all_cameras(svo)[name]
        full = frames[name].shaded(D.sky(svo.SKY_LINEAR)).reshape(H_, W_, 4)
        part = Frame(svo, world, cam, semantics, rect)
        got = part.shaded(D.sky(svo.SKY_LINEAR)).reshape(h, w, 4)
        assert np.array_equal(part.hit.reshape(h, w), frames[name].hit.reshape(H_, W_)[y0:y0 + h, x0:x0 + w])
        assert np.array_equal(got.view(np.uint32), full[y0:y0 + h, x0:x0 + w].view(np.uint32)), name
        part.free()
    D.free()


def rgba8(svo, rgba):
    """svo_frame_rgba8 of float32 [n][4] -> uint8 [n][4]; asserts that nothing is written past n."""
    rgba = np.ascontiguousarray(rgba, F).reshape(-1, 4)
    n = rgba.shape[0]
    src = svo.DeviceBuffer.from_numpy(rgba)
    out = svo.DeviceBuffer.from_numpy(np.full(n + PAD, 0xDEADBEEF, np.uint32))
    svo.frame_rgba8(src.ptr, n, out.ptr)
    sync(svo)
    got = out.to_numpy(np.uint32, n + PAD)
    src.free()
    out.free()
    assert np.all(got[n:] == 0xDEADBEEF), "wrote past n pixels"
    return got[:n].view(np.uint8).reshape(n, 4)                 # memory order R, G, B, A


def test_rgba8_equals_the_model(svo, frames):
    x = S.rgba8_inputs()
    got = rgba8(svo, x)
    assert np.array_equal(got, S.frame_rgba8(x))
    assert np.all(got[:, 3] == 255) and np.unique(got[:, 0]).size == 256
    D = DeviceSky(svo, S.random_faces(37, 33))
    f = mixed_view(frames)
    image = f.shaded(D.sky(svo.SKY_LINEAR))
    got = rgba8(svo, image)
    assert np.array_equal(got, S.frame_rgba8(image)) and np.all(got[:, 3] == 255)
    assert np.unique(got[:, :3]).size > 100
    D.free()


def test_trace_shade_sky_rgba8_end_to_end(svo, world, frames):
    """One stream, no host step in between: the four calls of a frame.  Sky pixels equal the model pipeline (lookup, then RGBA8), hit
    pixels the RGBA8 model of svo_shade's own output."""
    f = mixed_view(frames)
    name = [k for k, v in frames.items() if v is f][0]
    cam, _, semantics = S.all_cameras(svo)[name]
    faces = S.random_faces(37, 41)
    D = DeviceSky(svo, faces)
    gbuffer, rgba = svo.DeviceBuffer(N * 32), svo.DeviceBuffer(N * 16)
    out = svo.DeviceBuffer.from_numpy(np.full(N + PAD, 0xDEADBEEF, np.uint32))
    world.trace(cam, svo.trace_params(shadow=True, semantics=semantics), FULL, gbuffer.ptr)
    svo.shade(cam, f.P, FULL, gbuffer.ptr, rgba.ptr)
    svo.shade_sky(cam, D.sky(svo.SKY_LINEAR), FULL, rgba.ptr, gbuffer_ptr=gbuffer.ptr)
    svo.frame_rgba8(rgba.ptr, N, out.ptr)
    sync(svo)
    got = out.to_numpy(np.uint32, N + PAD)
    assert np.all(got[N:] == 0xDEADBEEF)
    got = got[:N].view(np.uint8).reshape(N, 4)
    hit, sky = f.hit, ~f.hit
    colour, face = S.lookup(f.dirs, faces, S.LINEAR)
    assert np.all(face >= 0)
    want_sky = S.frame_rgba8(np.concatenate([colour, np.ones((N, 1), F)], axis=1))
    assert np.array_equal(got[sky], want_sky[sky])
    assert np.array_equal(got[hit], S.frame_rgba8(f.base)[hit])
    assert np.all(got[:, 3] == 255) and hit.sum() >= 300 and sky.sum() >= 300
    for b in (gbuffer, rgba, out):
        b.free()
    D.free()

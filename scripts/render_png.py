"""Render one shaded frame (svo_trace + svo_shade) to a PNG — a human-readable sanity check of the whole path.
    python scripts/render_png.py out.png [depth] [width] [height] [--ao STRENGTH] [--reflect]
--ao STRENGTH (0..1): a ball of radius 12 is carved out of the terrain under the image's centre and the frame gets voxel ambient occlusion
(svo_hit_ao + svo_shade_ao) at that strength: the ball reads as a hole, creases and the foot of walls darken.
--reflect: the lake (material 6) mirrors the terrain and the picture's sky colour (svo_trace_reflections + svo_shade_reflections,
f0 = 0.02 with the Fresnel term).
"""
import importlib, os, struct, sys, zlib
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
svo = importlib.import_module("octree-raymarcher_amd")


def write_png(path, rgb):
    h, w, _ = rgb.shape
    raw = b"".join(b"\x00" + rgb[y].tobytes() for y in range(h))
    def chunk(t, d):
        c = struct.pack(">I", len(d)) + t + d
        return c + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    open(path, "wb").write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                           chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


ao = None
if "--ao" in sys.argv:
    i = sys.argv.index("--ao")
    ao = float(sys.argv[i + 1])
    del sys.argv[i:i + 2]
reflect = "--reflect" in sys.argv
if reflect:
    sys.argv.remove("--reflect")
out = sys.argv[1] if len(sys.argv) > 1 else "frame.png"
depth = int(sys.argv[2]) if len(sys.argv) > 2 else 9
w = int(sys.argv[3]) if len(sys.argv) > 3 else 960
h = int(sys.argv[4]) if len(sys.argv) > 4 else 540
W = svo.World.generate(4, 1, 4, 128, depth, build_device=0); W.upload(0)
cam = svo.make_camera((256.3, 150.0, -40.0), (0.0, -0.5, 0.866), (0.0, 1.0, 0.0), 60.0, w, h)
g = W.draw(cam, shadow=True)
if ao is not None:
    c = g[h // 2, w // 2]
    assert c["flags"] & 1, "the image's centre sees no terrain"
    fwd = np.array(cam.forward, np.float64)
    W.edit_ball_all(svo.EDIT_DESTROY, np.array(cam.eye, np.float64) + fwd * float(c["t"]), 12.0)
    g = W.draw(cam, shadow=True)
P = svo.shade_defaults()
# the reference's lights sit near the origin of a 4x4x4 world; for a picture, put a stronger sun-like term in
P.directional.diffuse[:] = [0.9, 0.85, 0.7]; P.directional.ambient[:] = [0.25, 0.3, 0.4]
gb = svo.DeviceBuffer.from_numpy(g); rgba = svo.DeviceBuffer(w * h * 16)
svo.shade(cam, P, (0, 0, w, h), gb.ptr, rgba.ptr)
if ao is not None:
    vox, aod = svo.DeviceBuffer(w * h * 32), svo.DeviceBuffer(w * h * 4)
    W.hit_voxels(gb.ptr, w * h, vox.ptr)
    W.hit_ao(cam, None, (0, 0, w, h), gb.ptr, vox.ptr, aod.ptr)
    svo.shade_ao(aod.ptr, ao, w * h, rgba.ptr)
SKY = (0.45, 0.65, 0.9)
if reflect:
    vox, refl = svo.DeviceBuffer(w * h * 32), svo.DeviceBuffer(w * h * 32)
    W.hit_voxels(gb.ptr, w * h, vox.ptr)
    W.trace_reflections(cam, svo.trace_params(shadow=True), (0, 0, w, h), gb.ptr, vox.ptr, refl.ptr, material=6)
    svo.shade_reflections(cam, P, svo.Mirror(6, 0.02, True, SKY), (0, 0, w, h), gb.ptr, vox.ptr, refl.ptr, rgba.ptr)
svo.lib.svo_stream_synchronize(None)
img = rgba.to_numpy(np.float32, w * h * 4).reshape(h, w, 4)
rgb = np.nan_to_num(img[..., :3], nan=0.0)
hit = (g["flags"] & 1) != 0
sky = np.array(SKY, np.float32)
rgb = np.where(hit[..., None], rgb, sky)
rgb = np.clip(rgb, 0, 1) ** (1 / 2.2)
write_png(out, (rgb * 255 + 0.5).astype(np.uint8))
print(out, "hits %.1f%%" % (100 * hit.mean()), "shadowed %.1f%%" % (100 * ((g["flags"] & 4) != 0).mean()), "materials", np.unique(g["material"][hit]))

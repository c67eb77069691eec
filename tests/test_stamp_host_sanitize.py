"""csrc/stamp.cpp (svo_chunk_stamp) under AddressSanitizer and UndefinedBehaviorSanitizer: compiled with g++ together with
csrc/grid.cpp, csrc/sparse_mesh.cpp, csrc/mesh.cpp, csrc/sparse_fill.cpp and the stand-alone host/stamp_check.cpp and run as a program
of its own, which compares the five ops with a dense loop for D_A <= 5, D_B <= D_A, offsets in [-N_B, N_A] and all 48 orientations,
stamps a depth-8 LEAF into the depth-12 and depth-16 cubes and tries the refusals.  CPU only; nothing is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "octree-raymarcher_amd")


def test_stamp_is_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "stamp_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(PKG, "csrc", "stamp.cpp"), os.path.join(PKG, "csrc", "grid.cpp"), os.path.join(PKG, "csrc", "sparse_mesh.cpp"),
                    os.path.join(PKG, "csrc", "mesh.cpp"), os.path.join(PKG, "csrc", "sparse_fill.cpp"), os.path.join(PKG, "host", "stamp_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": ok") == 13 and "WRONG" not in r.stdout and "runtime error" not in r.stderr

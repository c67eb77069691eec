"""csrc/extract.cpp (svo_chunk_extract) under AddressSanitizer and UndefinedBehaviorSanitizer: compiled with g++ together with
csrc/stamp.cpp, csrc/grid.cpp, csrc/sparse_mesh.cpp, csrc/mesh.cpp, csrc/sparse_fill.cpp and the stand-alone host/extract_check.cpp and
run as a program of its own, which compares pools and count with a dense loop of the header's rule for D_A <= 5, D_C <= D_A, offsets
in [-N_C, N_A] and all 48 orientations, takes windows of depth 8, 10 and 2 out of the depth-12 and depth-16 cubes, stamps one back and
tries the refusals.  extract.cpp holds its arrays in std::vector and calls malloc nowhere, so the stamp's g++ line carries over with
every warning an error.  CPU only; nothing is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "octree-raymarcher_amd")


def test_extract_is_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "extract_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(PKG, "csrc", "extract.cpp"), os.path.join(PKG, "csrc", "stamp.cpp"), os.path.join(PKG, "csrc", "grid.cpp"),
                    os.path.join(PKG, "csrc", "sparse_mesh.cpp"), os.path.join(PKG, "csrc", "mesh.cpp"), os.path.join(PKG, "csrc", "sparse_fill.cpp"),
                    os.path.join(PKG, "host", "extract_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": ok") == 13 and "WRONG" not in r.stdout and "runtime error" not in r.stderr

"""csrc/mesh.cpp (svo_grid_add_mesh, svo_grid_fill_enclosed) under AddressSanitizer and UndefinedBehaviorSanitizer: compiled with g++
together with the stand-alone host/mesh_check.cpp and run as a program of its own.  CPU only; nothing is loaded into python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "octree-raymarcher_amd")


def test_mesh_voxeliser_and_fill_are_clean_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "mesh_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(PKG, "csrc", "mesh.cpp"), os.path.join(PKG, "host", "mesh_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": ok") == 7 and "WRONG" not in r.stdout and "runtime error" not in r.stderr

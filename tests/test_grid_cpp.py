"""svo::World::chunk_from_grid / chunk_to_grid of the C++ adaptor (octree-raymarcher_amd/host/svo_world.hpp), called once from
host/example_grid.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "octree-raymarcher_amd", "host")
EXE = os.path.join(HOST, "example_grid")


def build():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I.", "example_grid.cpp", "-L..", "-lsvo_amd",
                    "-Wl,-rpath,$ORIGIN/..", "-o", "example_grid"], cwd=HOST, check=True)


def test_grid_example_compiles(svo):
    build()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
def test_grid_example_on_gpu(svo):
    build()
    r = subprocess.run([EXE, "5"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 cells differ" in r.stdout and "host pools equal" in r.stdout

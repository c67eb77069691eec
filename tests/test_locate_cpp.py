"""svo::World::locate of the C++ adaptor (octree-raymarcher_amd/host/svo_world.hpp), called once from host/example_locate.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "octree-raymarcher_amd", "host")
EXE = os.path.join(HOST, "example_locate")


def build():
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I.", "example_locate.cpp", "-L..", "-lsvo_amd",
                    "-Wl,-rpath,$ORIGIN/..", "-o", "example_locate"], cwd=HOST, check=True)


def test_locate_example_compiles(svo):
    build()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
def test_locate_example_on_gpu(svo):
    build()
    r = subprocess.run([EXE, "6"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 bad" in r.stdout and "located 34 points: 33 inside" in r.stdout

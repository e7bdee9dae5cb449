"""The three-dword form of a tile order (csrc/tnn_tile_order.h: pack_tile_order / unpack_tile_order), checked on the host:
tests/tile_order_packed_check.cpp is compiled with g++ and run.  No GPU.  The program compares tile_coords on the unpacked words
with tile_coords on the TileOrder they were packed from — every grid up to 64 x 64 tiles under every cut, pm = 1 / 2 / 65,535
over the largest grids the latency kernels take — and checks that the packer refuses what the words cannot hold."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "tile_order_packed_check.cpp")


def test_packed_tile_order_reads_the_same_tiles(tmp_path):
    exe = os.path.join(str(tmp_path), "tile_order_packed_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tinynn-autograd_amd", "csrc"), SOURCE, "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().startswith("packed tile order ok"), run.stdout

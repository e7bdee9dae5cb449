"""The division-free tile order of the latency kernels (csrc/tnn_tile_order.h), checked on the host: tests/tile_order_check.cpp
is compiled with g++ and run.  No GPU: the header is plain C++17 on the host side, and the program compares tile_coords with the
`/` and `%` formulas it replaced for every grid up to 64 x 64 tiles under every cut, the reciprocal at its extremes, and the head
launch's dW / dx orders (see the program's head comment)."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "tile_order_check.cpp")


def test_tile_order_matches_the_division_formulas(tmp_path):
    exe = os.path.join(str(tmp_path), "tile_order_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tinynn-autograd_amd", "csrc"), SOURCE, "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().startswith("tile order ok"), run.stdout

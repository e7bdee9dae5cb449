"""The runtime (dtype, vec) -> compile-time (T, VECTOR) selection that the float32 / float64 kernel families share
(csrc/tnn_dispatch.h), checked on the host: tests/float_dispatch_check.cpp is compiled with g++ and run.  No GPU: the header
is plain C++17, and a swapped arm is invisible to the numeric GPU tests (see the program's head comment)."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "float_dispatch_check.cpp")


def test_float_dispatch_reaches_every_arm(tmp_path):
    exe = os.path.join(str(tmp_path), "float_dispatch_check")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tinynn-autograd_amd", "csrc"), SOURCE, "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip() == "float dispatch ok", run.stdout

"""The host stage of the block-tridiagonal QP engine (trajopt_amd/csrc/tmx_csc_order.h: pattern of K, reverse Cuthill-McKee, uniform
blocks, the AUTO cost model) as a stand-alone C++ program, tests/cpp/csc_order_test.cpp - once as it is and once under
AddressSanitizer / UndefinedBehaviorSanitizer (plain host code with its own main)."""
import os
import subprocess

import pytest

from test_cpp_host_api import BUILD, ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "csc_order_test.cpp")
HDR = os.path.join(ROOT, "trajopt_amd", "csrc", "tmx_csc_order.h")


def _build(tag, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "csc_order_test_" + tag)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.dirname(HDR), SRC, "-o", exe] + extra)
    return exe


@pytest.mark.parametrize("tag,extra", [("plain", []), ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_csc_ordering_and_partition(tag, extra):
    p = subprocess.run([_build(tag, extra)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), f"rc={p.returncode}\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"

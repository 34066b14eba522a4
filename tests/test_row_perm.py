"""build_row_perm (trajopt_amd/csrc/tmx_row_perm.h): the row -> thread assignment of the register-resident ADMM bursts, built at upload.

tests/cpp/row_perm_test.cpp is a stand-alone program over the header alone, built with the address and undefined-behaviour sanitizers.
For every row count 1 .. 512 and seeded slack-count vectors with entries in {0, 1, 2} - R <= 256, heavy-majority rows and R within
8 of 512 among them - it checks: every row slot is placed exactly once and every other entry is -1; second rows sit only on the last
max(0, R - 256) threads; no thread carries two two-slack rows while a one-slack row sits on a single-row thread of a lower wave."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "cpp", "_build")
SRC = os.path.join(HERE, "cpp", "row_perm_test.cpp")
CSRC = os.path.join(ROOT, "trajopt_amd", "csrc")


def test_row_perm_properties_under_sanitizers():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "row_perm_test")
    newest = max(os.path.getmtime(p) for p in (SRC, os.path.join(CSRC, "tmx_row_perm.h")))
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-I" + CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr

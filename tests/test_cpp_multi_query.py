"""The multi-query operations of the C++ host layer (include/tmx_trajopt.hpp: setQueries / setQueryTargets / bestPerQuery) against the
Python layer (runtime.BatchedTrustRegionSQP with queries) on the same problem: configuration 0 at 6 waypoints, two queries that differ
in the goal, three seeds each.  The best trajectory of every query must be the Python result's bytes.

CPU tier: tests/cpp/multi_query_test.cpp linked against the kernel sources built for the host.  GPU tier: libtrajopt_mi355x.so."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_host_api import BUILD, HDRS, PRODUCT_LIB, ROOT, _fmt, _robot_block
from trajopt_amd import configs, runtime
from trajopt_amd.problem import pr2_right_arm

SRC = os.path.join(ROOT, "tests", "cpp", "multi_query_test.cpp")
Q, S, T = 2, 3, 6


def _build(lib_path, tag):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "multi_query_test_" + tag + "_" + os.path.splitext(os.path.basename(lib_path))[0])
    newest = max(os.path.getmtime(p) for p in [SRC, lib_path] + HDRS)
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        libdir, libname = os.path.dirname(lib_path), os.path.basename(lib_path)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                               "-o", exe, "-L" + libdir, "-l:" + libname, "-Wl,-rpath," + libdir, "-fopenmp"])
    return exe


def _case(tmp_path):
    pci, s, g = configs.config0(T)
    goals = np.stack([g, g + np.array([0.1, -0.1, 0.1, 0.1, 0.1, 0.1, -0.1])])
    x0 = np.concatenate([configs.seeds_for(0, pci, s, goals[q], S, sigma=0.1, first=q * S) for q in range(Q)])
    lines = _robot_block("pr2_right_arm", pr2_right_arm(), "r_gripper_tool_frame")
    for name, v in (("start", s), ("goals", goals), ("seeds", x0)):
        lines.append(f"vector {name} {np.asarray(v).size} {_fmt(v)}")
    path = tmp_path / "input.txt"
    path.write_text("\n".join(lines) + "\n")
    return pci, goals, x0, str(path)


def _check(exe, lib_path, tmp_path):
    pci, goals, x0, path = _case(tmp_path)
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    cpp = {}
    for ln in p.stdout.splitlines():
        tok = ln.split()
        if tok and tok[0] == "BEST":
            cpp[int(tok[1])] = (int(tok[2]), int(tok[3]), float.fromhex(tok[4]), np.array([float.fromhex(t) for t in tok[5:]]))
    opt = runtime.BatchedTrustRegionSQP(pci, lib_path=lib_path, queries=[[], [(pci.cnt_infos[0], goals[1])]])
    try:
        opt.initialize(x0)
        status, best = opt.optimize()
    finally:
        opt.ctx.close()
    assert sorted(cpp) == list(range(Q)) and best["found"].all()
    for q in range(Q):
        index, found, cost, x = cpp[q]
        assert (index, bool(found)) == (int(best["index"][q]), True) and q * S <= index < (q + 1) * S
        assert cost == best["total_cost"][q]
        assert x.tobytes() == best["x"][q].reshape(-1).tobytes()
    # the two queries reach their own goals
    assert np.abs(best["x"][:, -1, :] - goals).max() < 1e-4


def test_cpp_multi_query_equals_python_on_host_build(hostemu_lib, tmp_path):
    _check(_build(hostemu_lib, "hostemu"), hostemu_lib, tmp_path)


@pytest.mark.gpu
def test_cpp_multi_query_equals_python_on_device(tmp_path):
    assert os.path.exists(PRODUCT_LIB), "libtrajopt_mi355x.so missing: run __graft_entry__.build()"
    _check(_build(PRODUCT_LIB, "product"), None, tmp_path)

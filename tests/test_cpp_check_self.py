"""The self-collision side of the trajectory check in the C++ host layer (include/tmx_trajopt.hpp: setSelfCollisionPairs by link name,
checkSelfTrajectories, bestPerQuery(cfg)) against the Python layer on the same problem: configuration 0 at 6 waypoints without an
obstacle, a goal that folds the PR2 arm at the elbow and the wrist, four seeds.  The self check of the seeds before optimize(), of the
iterates after it (the class uploads the problem again in between: the pairs must survive) and the best seed that is free of itself
must be the Python result's bytes; an unknown link name throws.

CPU tier: tests/cpp/check_self_test.cpp linked against the kernel sources built for the host.  GPU tier: libtrajopt_mi355x.so."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_host_api import BUILD, HDRS, PRODUCT_LIB, ROOT, _fmt, _robot_block
from trajopt_amd import abi, configs, runtime
from trajopt_amd.problem import pr2_right_arm

SRC = os.path.join(ROOT, "tests", "cpp", "check_self_test.cpp")
S, T = 4, 6
PAIRS = [(6, 2), (4, 2)]


def _build(lib_path, tag):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "check_self_test_" + tag + "_" + os.path.splitext(os.path.basename(lib_path))[0])
    newest = max(os.path.getmtime(p) for p in [SRC, lib_path] + HDRS)
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        libdir, libname = os.path.dirname(lib_path), os.path.basename(lib_path)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                               "-o", exe, "-L" + libdir, "-l:" + libname, "-Wl,-rpath," + libdir, "-fopenmp"])
    return exe


def _case(tmp_path):
    pci, s, g = configs.config0(T)
    g = g.copy()
    g[3], g[5] = -2.0, -1.7      # elbow and wrist flexed: the gripper comes back towards the upper arm
    pci.cnt_infos[0].targets = list(g)
    x0 = configs.seeds_for(0, pci, s, g, S, sigma=0.1, first=0)
    cfg = abi.default_check_config(4, 0.05, 0.1, 5)
    lines = _robot_block("pr2_right_arm", pr2_right_arm(), "r_gripper_tool_frame")
    for name, v in (("start", s), ("goal", g), ("seeds", x0), ("cfg", [cfg.evaluator_type, cfg.max_substates, cfg.margin, cfg.longest_valid_segment_length])):
        lines.append(f"vector {name} {np.asarray(v).size} {_fmt(v)}")
    path = tmp_path / "input.txt"
    path.write_text("\n".join(lines) + "\n")
    return pci, x0, cfg, str(path)


def _check(exe, lib_path, tmp_path):
    pci, x0, cfg, path = _case(tmp_path)
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    got, best = {"SELF": {}, "AFTER": {}}, None
    for ln in p.stdout.splitlines():
        tok = ln.split()
        if tok and tok[0] in got:
            vals = np.array([float.fromhex(t) for t in tok[7:]])
            got[tok[0]][int(tok[1])] = (int(tok[2]), tuple(int(t) for t in tok[3:7]), vals[0], vals[1:1 + T], vals[1 + T:])
        if tok and tok[0] == "BEST":
            best = (int(tok[1]), int(tok[2]), float.fromhex(tok[3]), float.fromhex(tok[4]), np.array([float.fromhex(t) for t in tok[5:]]))
    opt = runtime.BatchedTrustRegionSQP(pci, lib_path=lib_path)
    try:
        opt.check_set_link_pairs(PAIRS)
        want = {"SELF": opt.check_self_trajectories(cfg, x=x0)}
        opt.initialize(x0)
        opt.optimize()
        want["AFTER"] = opt.check_self_trajectories(cfg)
        wbest = opt.best_per_query(check=cfg)
    finally:
        opt.ctx.close()
    # the case is not vacuous: the pairs produce contacts, and the folded end of the trajectories is closer than the margin
    assert (want["SELF"]["min_distance"][:, :T - 1] < 1e299).all() and (want["SELF"]["penetration"] > 0).any() and not want["SELF"]["free"].all()
    for tag in ("SELF", "AFTER"):
        assert sorted(got[tag]) == list(range(S))
        for b in range(S):
            free, worst, wmin, md, pen = got[tag][b]
            w = want[tag]["worst"][b]
            assert bool(free) == bool(want[tag]["free"][b]) and wmin == w["min_distance"]
            assert worst == (w["step"], w["primitive_a"], w["primitive_b"], w["substate"])
            assert md.tobytes() == want[tag]["min_distance"][b].tobytes() and pen.tobytes() == want[tag]["penetration"][b].tobytes()
    index, found, cost, clear, x = best
    assert (index, bool(found)) == (int(wbest["index"][0]), bool(wbest["found"][0]))
    assert cost == wbest["total_cost"][0] and clear == wbest["min_distance"][0] and x.tobytes() == wbest["x"][0].reshape(-1).tobytes()


def test_cpp_self_check_equals_python_on_host_build(hostemu_lib, tmp_path):
    _check(_build(hostemu_lib, "hostemu"), hostemu_lib, tmp_path)


@pytest.mark.gpu
def test_cpp_self_check_equals_python_on_device(tmp_path):
    assert os.path.exists(PRODUCT_LIB), "libtrajopt_mi355x.so missing: run __graft_entry__.build()"
    _check(_build(PRODUCT_LIB, "product"), None, tmp_path)

"""The trajectory collision check of the C++ host layer (include/tmx_trajopt.hpp: CollisionCheckConfig, checkTrajectories,
bestPerQuery(cfg)) against the Python layer on the same problem: configuration 0 at 6 waypoints next to one sphere obstacle, two
queries that differ in the goal, three seeds each.  The check of the seeds before optimize() and the best collision-free trajectory of
every query after it must be the Python result's bytes.

CPU tier: tests/cpp/check_trajectories_test.cpp linked against the kernel sources built for the host.  GPU tier: libtrajopt_mi355x.so."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_host_api import BUILD, HDRS, PRODUCT_LIB, ROOT, _fmt, _robot_block
from trajopt_amd import abi, configs, runtime
from trajopt_amd.problem import pr2_right_arm

SRC = os.path.join(ROOT, "tests", "cpp", "check_trajectories_test.cpp")
Q, S, T = 2, 3, 6


def _build(lib_path, tag):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "check_trajectories_test_" + tag + "_" + os.path.splitext(os.path.basename(lib_path))[0])
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
    pmid = pci.robot.fk_tool(0.5 * (s + g))[:3, 3]
    obstacle = (float(pmid[0]) + 0.02, float(pmid[1]), float(pmid[2]) - 0.3), 0.15
    pci.obstacles.append(obstacle)
    cfg = abi.default_check_config(4, 0.02, 0.1, 5)
    lines = _robot_block("pr2_right_arm", pr2_right_arm(), "r_gripper_tool_frame")
    for name, v in (("start", s), ("goals", goals), ("seeds", x0), ("obstacle", list(obstacle[0]) + [obstacle[1]]),
                    ("cfg", [cfg.evaluator_type, cfg.max_substates, cfg.margin, cfg.longest_valid_segment_length])):
        lines.append(f"vector {name} {np.asarray(v).size} {_fmt(v)}")
    path = tmp_path / "input.txt"
    path.write_text("\n".join(lines) + "\n")
    return pci, goals, x0, cfg, str(path)


def _check(exe, lib_path, tmp_path):
    pci, goals, x0, cfg, path = _case(tmp_path)
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"rc={p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    chk, best = {}, {}
    for ln in p.stdout.splitlines():
        tok = ln.split()
        if tok and tok[0] == "CHECK":
            vals = np.array([float.fromhex(t) for t in tok[7:]])
            chk[int(tok[1])] = (int(tok[2]), tuple(int(t) for t in tok[3:7]), vals[0], vals[1:1 + T], vals[1 + T:])
        if tok and tok[0] == "BEST":
            best[int(tok[1])] = (int(tok[2]), int(tok[3]), float.fromhex(tok[4]), float.fromhex(tok[5]), np.array([float.fromhex(t) for t in tok[6:]]))
    opt = runtime.BatchedTrustRegionSQP(pci, lib_path=lib_path, queries=[[], [(pci.cnt_infos[0], goals[1])]])
    try:
        before = opt.check_trajectories(cfg, x=x0)
        opt.initialize(x0)
        opt.optimize()
        want = opt.best_per_query(check=cfg)
    finally:
        opt.ctx.close()
    assert sorted(chk) == list(range(Q * S)) and sorted(best) == list(range(Q))
    assert not before["free"].all() and (before["penetration"] > 0).any()     # the obstacle is in the way of some seed
    for b in range(Q * S):
        free, worst, wmin, md, pen = chk[b]
        w = before["worst"][b]
        assert bool(free) == bool(before["free"][b]) and worst == (w["step"], w["primitive"], w["obstacle"], w["substate"]) and wmin == w["min_distance"]
        assert md.tobytes() == before["min_distance"][b].tobytes() and pen.tobytes() == before["penetration"][b].tobytes()
    for q in range(Q):
        index, found, cost, clear, x = best[q]
        assert (index, bool(found)) == (int(want["index"][q]), bool(want["found"][q]))
        assert cost == want["total_cost"][q] and clear == want["min_distance"][q]
        assert x.tobytes() == want["x"][q].reshape(-1).tobytes()


def test_cpp_check_equals_python_on_host_build(hostemu_lib, tmp_path):
    _check(_build(hostemu_lib, "hostemu"), hostemu_lib, tmp_path)


@pytest.mark.gpu
def test_cpp_check_equals_python_on_device(tmp_path):
    assert os.path.exists(PRODUCT_LIB), "libtrajopt_mi355x.so missing: run __graft_entry__.build()"
    _check(_build(PRODUCT_LIB, "product"), None, tmp_path)

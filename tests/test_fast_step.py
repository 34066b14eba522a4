"""The specialised SQP shell around the QP solve (trajopt_amd/csrc/tmx_step.h: qp_structure_fast - prefix counts by wave ballots, one
thread per primary column with a non-zero mask, column pointers by wave scans) against the generic code of the SAME library
(DevProblem::dbg_flags bit 3, set through tmx_debug_set_flags).  The two must agree in every bit: results(), state() and step_log()
after every bounded run(1) step, and every integer of every QP record - n, m, nnzP, nnzA, hashP, hashA and warm_started are the
structure pass's own output (the warm start is decided from the hashes of two consecutive QPs), the rest shows that the solve saw
the same QP.  Every test first asserts the upload's verdict (tmx_debug_step_fast) and that the compared run did something.

Which kernels run: a bounded tmx_sqp_run(max_steps = 1) launches k_sqp_fused, a whole optimize() (run(0)) launches k_sqp_pool; both
execute sqp_step_block at TMX_QP_NT threads, where the switch is read.  convexify() + export_csc() launch k_convexify and k_export_csc:
piecewise kernels that call the generic qp_structure whatever the switch says, so the comparison of their integer arrays
(test_export_csc_after_convexify) shows that the switch leaves them alone, not that the new code agrees with them.

CPU tier: libtmx_simt.so (tests/test_simt_emulation.py) - the device branches on cooperative fibers with real barriers and poisoned LDS.
GPU tier: the product library.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import parity_checks as pc
from conftest import ROOT
from test_simt_emulation import simt, simt_lib  # noqa: F401  (fixtures)
from trajopt_amd import configs

GENERIC_STEP = 8  # DevProblem::dbg_flags bit 3


def _set_flags(ctx, flags):
    fn = ctx.lib.tmx_debug_set_flags
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], C.c_int
    assert fn(ctx.h, flags) == 0


def _verdict(ctx):
    """the upload's verdict (DevProblem::step_fast)"""
    fn = ctx.lib.tmx_debug_step_fast
    fn.argtypes, fn.restype = [C.c_void_p], C.c_int
    return fn(ctx.h)


def _rec_ints(ctx, cap=64):
    recs, cnt = ctx.qp_records(cap)
    return [[recs[b * cap + k].key() for k in range(min(int(cnt[b]), cap))] for b in range(len(cnt))]


def _snapshot(ctx):
    """everything a step leaves behind, as bytes / integers"""
    r = ctx.results()
    st = ctx.state()
    logs = ctx.step_log()
    return (tuple(r[k].tobytes() for k in ("x", "status", "total_cost", "n_func_evals", "n_qp_solves")),
            tuple(st[k].tobytes() for k in ("sqp_iter", "merit_increases", "trust_box_size", "done")),
            tuple(tuple(np.asarray(v).tobytes() for _, v in sorted(lg.items())) for lg in logs))


def _steps(ctx, x0, flags, max_steps):
    """run(1) up to max_steps times (0: until every problem is done); the snapshot after every step, the record integers at the end
    and the step logs of every step (for the conditions on the inputs)"""
    _set_flags(ctx, flags)
    try:
        ctx.set_x0(x0)
        snaps, logs = [], []
        while max_steps == 0 or len(snaps) < max_steps:
            na = ctx.run(1)
            snaps.append(_snapshot(ctx))
            logs.append(ctx.step_log())
            if na == 0:
                break
            assert len(snaps) < 200
        return snaps, _rec_ints(ctx), logs
    finally:
        _set_flags(ctx, 0)


def _first_step_both_ways(ctx, x0):
    a = _steps(ctx, x0, 0, 1)
    b = _steps(ctx, x0, GENERIC_STEP, 1)
    return a, b


def _assert_one_step_ran(recs):
    # one QP record per problem, each of a QP with slack variables (n > NX is checked by the caller where it knows NX)
    assert all(len(per) == 1 for per in recs)


def test_first_step_of_baseline_config1(simt):
    """config 1 at T = 30 (R = 304 > 256 threads: 48 threads carry two slots; the 17-row goal waypoint; n = 572 > 2 x 256: three passes
    of the column-pointer scan; rows with two slack variables), two seeds, the first trust-region evaluation"""
    pci, s, g = pc.cfg(1)
    x0 = configs.seeds_for(1, pci, s, g, 2, sigma=0.05)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _verdict(simt) == 1
    a, b = _first_step_both_ways(simt, x0)
    _assert_one_step_ran(a[1])
    assert all(per[0][0] > 2 * 256 for per in a[1])  # n: three column-pointer passes
    assert a[1] == b[1]
    assert a[0] == b[0]


def test_whole_optimize_of_config1_short_horizon_stepped(simt):
    """config 1 with T = 8, seeds 2 and 3 at sigma 0.05, stepped to the end with run(1) (25 steps).  Conditions on the inputs, checked
    on the generic path: the steps hold an accepted and a rejected evaluation, two consecutive QPs of a problem differ in m or nnzA
    (the active set changed), and a warm start was both taken and refused.  (Seeds 0 and 1, the ones of tests/test_fast_polish.py,
    never reject a step.)"""
    pci, s, g = pc.cfg(1, T=8)
    x0 = configs.seeds_for(1, pci, s, g, 2, sigma=0.05, first=2)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _verdict(simt) == 1
    b = _steps(simt, x0, GENERIC_STEP, 0)
    recs = b[1]
    ratios = [(lg["exact_merit_improve"], lg["merit_improve_ratio"]) for step in b[2] for lg in step if lg["valid"]]
    assert any(e >= 0 and r >= 0.25 for e, r in ratios) and any(e < 0 or r < 0.25 for e, r in ratios)
    assert any(per[k][1] != per[k + 1][1] or per[k][3] != per[k + 1][3] for per in recs for k in range(len(per) - 1))
    warm = [k[4] for per in recs for k in per[1:]]
    assert any(w == 1 for w in warm) and any(w == 0 for w in warm)
    a = _steps(simt, x0, 0, 0)
    assert a[1] == b[1]
    assert a[0] == b[0]


@pytest.mark.parametrize("cid,verdict", [(0, 1), (9, 1), (10, 0), (11, 1), (14, 1)])
def test_first_step_of_smaller_shapes(simt, cid, verdict):
    """configs 0 and 9: D < 7; 11: collision rows as constraints; 14: constant rows at a fixed waypoint.  Config 10 (JointPos costs and
    inequality slots) has waypoints with more than TMX_SETUP_COL rows: setup_fast does not hold, so the upload does not qualify and
    both ways run the generic code"""
    pci, s, g = pc.cfg(cid)
    x0 = configs.seeds_for(cid, pci, s, g, 2)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _verdict(simt) == verdict
    a, b = _first_step_both_ways(simt, x0)
    _assert_one_step_ran(a[1])
    assert a[1] == b[1]
    assert a[0] == b[0]


def test_first_step_with_joint_position_costs(simt):
    """the problem of config 10 without its JointPos band constraint (configs.config_mini(with_pos_costs=True, with_joint_band=False)):
    JointPosEqCost (velocity kind 1) and JointPosIneqCost slots (two rows per joint and waypoint) next to collision costs, the cart-pose
    and the goal JointPos constraints, at most TMX_SETUP_COL rows per waypoint - the upload qualifies, so these slot kinds go through
    the new structure pass and decision.  (Config 9 already brings JointPos inequality and equality CONSTRAINT slots.)"""
    pci, s, g = configs.config_mini(with_pos_costs=True, with_joint_band=False)
    x0 = configs.seeds_for(10, pci, s, g, 2)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _verdict(simt) == 1
    a, b = _first_step_both_ways(simt, x0)
    _assert_one_step_ran(a[1])
    assert a[1] == b[1]
    assert a[0] == b[0]


def test_export_csc_after_convexify(simt):
    """export_csc() integer arrays after convexify(), both ways, config 1 at T = 30: k_convexify / k_export_csc run the generic
    structure code under either flag (module docstring) - equal arrays, and the dimensions are those of the first step's QP record"""
    pci, s, g = pc.cfg(1)
    x0 = configs.seeds_for(1, pci, s, g, 2, sigma=0.05)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _verdict(simt) == 1
    out = []
    try:
        for flags in (0, GENERIC_STEP):
            _set_flags(simt, flags)
            simt.set_x0(x0)
            simt.convexify()
            qs = [simt.export_csc(b) for b in range(2)]
            out.append([(q["n"], q["m"]) + tuple(q[k].tobytes() for k in ("P_p", "P_i", "A_p", "A_i")) for q in qs])
    finally:
        _set_flags(simt, 0)
    assert out[0] == out[1]
    a = _steps(simt, x0, 0, 1)
    assert [(per[0][0], per[0][1]) for per in a[1]] == [(q[0], q[1]) for q in out[0]]
    assert all(len(q[4]) // 8 == q[0] + 1 for q in out[0])  # A_p: n + 1 column pointers


@pytest.mark.parametrize("cid", [15, 16])
def test_a_problem_outside_the_predicate_is_untouched(simt, cid):
    """config 15 (no row slot) and config 16 (rows on two waypoints): the upload does not qualify and the switch changes nothing"""
    pci, s, g = pc.cfg(cid)
    x0 = configs.seeds_for(cid, pci, s, g, 2)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _verdict(simt) == 0
    a, b = _first_step_both_ways(simt, x0)
    assert a[1] == b[1]
    assert a[0] == b[0]


def test_capsule_links_either_way(simt):
    """config 20 (capsule primitives): the structure pass does not depend on the geometry, so the upload qualifies; equal bytes both ways"""
    pci, s, g = pc.cfg(20)
    x0 = configs.seeds_for(20, pci, s, g, 2)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _verdict(simt) == 1
    a, b = _first_step_both_ways(simt, x0)
    assert a[1] == b[1]
    assert a[0] == b[0]


def test_the_thread_order_changes_no_bit(simt_lib):
    """the first case with the threads executed in descending order between two barriers (a fresh process per order: the order is
    read once): a missing barrier around the exchanges of the structure pass would show here"""
    code = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import parity_checks as pc
from trajopt_amd import configs, runtime
ctx = runtime.Context(0, %r)
pci, s, g = pc.cfg(1)
x0 = configs.seeds_for(1, pci, s, g, 2, sigma=0.05)
pc.make_ctx_inputs(ctx, pci, x0)
fn = ctx.lib.tmx_debug_step_fast
fn.argtypes, fn.restype = [C.c_void_p], C.c_int
assert fn(ctx.h) == 1
ctx.run(1)
recs, cnt = ctx.qp_records(4)
assert (cnt == 1).all()
ints = np.array([[v %% (1 << 63) for v in recs[b * 4].key()] for b in range(len(cnt))], dtype=np.uint64)
x = ctx.results()["x"]
ctx.close()
np.save(sys.argv[1], np.concatenate([ints.ravel().view(np.float64), x.ravel()]))
""" % (ROOT, os.path.join(ROOT, "tests"), simt_lib)
    res = {}
    with tempfile.TemporaryDirectory() as d:
        for o in ("0", "1"):
            env = dict(os.environ, TMX_SIMT_ORDER=o)
            path = os.path.join(d, f"x{o}.npy")
            subprocess.check_call([sys.executable, "-c", code, path], env=env)
            res[o] = np.load(path)
    assert res["0"].tobytes() == res["1"].tobytes()


@pytest.fixture()
def gpu(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_gpu_whole_optimize_of_config1(gpu):
    """BASELINE config 1, 16 seeds, whole optimize() both ways on one context: results and record integers byte for byte"""
    pci, s, g = pc.cfg(1)
    x0 = configs.seeds_for(1, pci, s, g, 16)
    pc.make_ctx_inputs(gpu, pci, x0)
    assert _verdict(gpu) == 1
    out = []
    try:
        for flags in (0, GENERIC_STEP):
            _set_flags(gpu, flags)
            gpu.set_x0(x0)
            gpu.run(0)
            r = gpu.results()
            out.append((tuple(r[k].tobytes() for k in ("x", "status", "total_cost", "n_func_evals", "n_qp_solves")), _rec_ints(gpu)))
    finally:
        _set_flags(gpu, 0)
    assert all(len(per) > 1 for per in out[0][1])
    assert out[0] == out[1]


@pytest.mark.gpu
def test_gpu_first_step_of_config0(gpu):
    """config 0 (D < 7), 16 seeds, the first trust-region evaluation both ways"""
    pci, s, g = pc.cfg(0)
    x0 = configs.seeds_for(0, pci, s, g, 16)
    pc.make_ctx_inputs(gpu, pci, x0)
    assert _verdict(gpu) == 1
    a, b = _first_step_both_ways(gpu, x0)
    _assert_one_step_ran(a[1])
    assert a[1] == b[1]
    assert a[0] == b[0]

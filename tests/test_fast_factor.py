"""The ADMM factorisation of the dense fast path (trajopt_amd/csrc/tmx_factor.h: the interior inverses of the nested dissection inside one
wave, the pivot row exchanged behind a wave-level sync) - against the generic factorisation of the SAME library (kkt_invert: dpart_factor /
gj_rows with a workgroup barrier per elimination step; DevProblem::dbg_flags bit 5, set through tmx_debug_set_flags).  The two must agree
in every bit: solutions byte for byte, every integer of the QP records equal.  Every test first asserts the upload's verdict
(tmx_debug_factor_fast), so the comparison cannot hold trivially.

CPU tier: libtmx_simt.so (tests/test_simt_emulation.py) - the device branches on cooperative fibers with real barriers and poisoned LDS.
GPU tier: the product library.  The emulation models neither the rounding of v_rcp_f64 nor the accumulation order inside an MFMA: the
three GPU cases are the check of those.
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
from trajopt_amd import abi, configs, runtime

GENERIC_FACTOR = 32


def _set_flags(ctx, flags):
    fn = ctx.lib.tmx_debug_set_flags
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], C.c_int
    assert fn(ctx.h, flags) == 0


def _qualifies(ctx):
    """the upload's verdict (DevProblem::factor_fast)"""
    fn = ctx.lib.tmx_debug_factor_fast
    fn.argtypes, fn.restype = [C.c_void_p], C.c_int
    return fn(ctx.h) == 1


def _ints(rec):
    return [(r.osqp_status, r.osqp_iter, r.rho_updates, r.polish_status, r.hash_active) for r in rec]


def _first_qp_both_ways(ctx, x0):
    """the first Model::optimize() of the uploaded problem with the in-wave factorisation (flags 0) and the generic one (flags 32)"""
    out = []
    try:
        for flags in (0, GENERIC_FACTOR):
            _set_flags(ctx, flags)
            ctx.set_x0(x0)
            ctx.convexify()
            xq, cvx, rec = ctx.qp_solve()
            out.append((np.asarray(xq).tobytes(), _ints(rec)))
    finally:
        _set_flags(ctx, 0)
    return out


def _full_run_both_ways(ctx, x0):
    """whole optimize() both ways: the results and the integers of every QP record of the run (tmx_sqp_qp_records)"""
    out = []
    try:
        for flags in (0, GENERIC_FACTOR):
            _set_flags(ctx, flags)
            ctx.set_x0(x0)
            ctx.run(0)
            r = ctx.results()
            recs, cnt = ctx.qp_records(64)
            ints = [_ints([recs[b * 64 + k] for k in range(min(int(cnt[b]), 64))]) for b in range(len(cnt))]
            out.append((r["status"].tobytes(), r["n_qp_solves"].tobytes(), r["x"].tobytes(), ints))
    finally:
        _set_flags(ctx, 0)
    return out


def _a_rho_update_happened(ints):
    """the factorisation behind an adaptive-rho update (the call from qp_check_nl), not only the setup's"""
    return any(i[2] > 0 for i in ints)


def test_first_qp_of_baseline_config1(simt):
    """config 1 at its real size (7 x 30), two seeds: P = 8 interiors of 3,3,3,3,3,3,3,2 blocks - two matrices per wave on all four
    waves, a 14-row matrix next to a 21-row one in the last wave, the unrolled 21-step instantiation; ns = 49, Zst = 56"""
    pci, s, g = pc.cfg(1)
    x0 = configs.seeds_for(1, pci, s, g, 2, sigma=0.05)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _qualifies(simt)
    a, b = _first_qp_both_ways(simt, x0)
    assert a[1] == b[1]
    assert a[0] == b[0]


def test_whole_optimize_of_config1_short_horizon(simt):
    """config 1 with T = 8, two seeds, the whole optimize(): P = 2, interiors of 4 and 3 blocks (the widest row instantiation, one matrix
    per wave on two waves, two waves without one), one separator (ns = 7).  At least one QP record has rho_updates > 0: the call behind
    the rho update is exercised."""
    pci, s, g = pc.cfg(1, T=8)
    x0 = configs.seeds_for(1, pci, s, g, 2, sigma=0.05)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _qualifies(simt)
    a, b = _full_run_both_ways(simt, x0)
    assert _a_rho_update_happened([i for per_problem in a[3] for i in per_problem])
    assert a == b
    assert (np.frombuffer(a[1], dtype=np.int32) > 1).all()


def test_first_qp_of_config1_with_fourteen_waypoints(simt):
    """config 1 with T = 14, two seeds: P = 4 (one matrix per wave on every wave), ns = 21, Zst = 24: the small separator instantiation"""
    pci, s, g = pc.cfg(1, T=14)
    x0 = configs.seeds_for(1, pci, s, g, 2, sigma=0.05)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _qualifies(simt)
    a, b = _first_qp_both_ways(simt, x0)
    assert a[1] == b[1]
    assert a[0] == b[0]


@pytest.mark.parametrize("cid", [0, 9])
def test_first_qp_with_fewer_than_seven_joints(simt, cid):
    """D < 7: pad joints in the rows of G, matrices of other sizes on the lanes of a wave (the run-time step loop)"""
    pci, s, g = pc.cfg(cid)
    x0 = configs.seeds_for(cid, pci, s, g, 2)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _qualifies(simt)
    a, b = _first_qp_both_ways(simt, x0)
    assert a[1] == b[1]
    assert a[0] == b[0]


def test_a_problem_outside_the_fast_path_is_untouched(simt, orc):
    """config 16 (segment collision rows on two waypoints: never on the dense fast path, the upload does not qualify): the switch
    changes nothing, and the solve is still the oracle's"""
    pci, s, g = pc.cfg(16)
    x0 = configs.seeds_for(16, pci, s, g, 2)
    desc = pc.make_ctx_inputs(simt, pci, x0)
    assert not _qualifies(simt)
    a, b = _first_qp_both_ways(simt, x0)
    assert a == b
    simt.set_x0(x0)
    res = pc.check_first_qp_solve(simt, orc, desc, x0)
    assert all(same for same, _ in res)


def test_first_qp_of_config1_under_another_rho_interval(simt):
    """config 1 under adaptive_rho_interval = 13 (a row of tests/test_osqp_settings.py): factorisations at iterations that are not check
    iterations; at least one rho update happens"""
    pci, s, g = pc.cfg(1)
    x0 = configs.seeds_for(1, pci, s, g, 2, sigma=0.05)
    st = abi.default_osqp_settings()
    st.adaptive_rho_interval = 13
    pc.make_ctx_inputs(simt, pci, x0, osqp=st)
    assert _qualifies(simt)
    a, b = _first_qp_both_ways(simt, x0)
    assert _a_rho_update_happened(a[1])
    assert a[1] == b[1]
    assert a[0] == b[0]


def test_the_thread_order_changes_no_bit(simt_lib):
    """the first case with the threads executed in descending order between two synchronisation points (a fresh process per order: the
    order is read once): a missing wave sync or barrier around the exchange of the pivot row would show here"""
    code = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import parity_checks as pc
from trajopt_amd import configs, runtime
ctx = runtime.Context(0, %r)
pci, s, g = pc.cfg(1)
x0 = configs.seeds_for(1, pci, s, g, 2, sigma=0.05)
pc.make_ctx_inputs(ctx, pci, x0)
fn = ctx.lib.tmx_debug_factor_fast
fn.argtypes, fn.restype = [C.c_void_p], C.c_int
assert fn(ctx.h) == 1
ctx.convexify()
xq, cvx, rec = ctx.qp_solve()
ctx.close()
np.save(sys.argv[1], np.asarray(xq).ravel())
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
    """BASELINE config 1, 16 seeds, whole optimize() both ways on one context: status, QP counts, trajectories and the integers of
    every QP record"""
    pci, s, g = pc.cfg(1)
    x0 = configs.seeds_for(1, pci, s, g, 16)
    pc.make_ctx_inputs(gpu, pci, x0)
    assert _qualifies(gpu)
    a, b = _full_run_both_ways(gpu, x0)
    assert _a_rho_update_happened([i for per_problem in a[3] for i in per_problem])
    assert a == b


@pytest.mark.gpu
def test_gpu_whole_optimize_of_config1_short_horizon(gpu):
    """config 1 with T = 8 (the run-time step loop on the widest rows), 16 seeds, whole optimize() both ways"""
    pci, s, g = pc.cfg(1, T=8)
    x0 = configs.seeds_for(1, pci, s, g, 16)
    pc.make_ctx_inputs(gpu, pci, x0)
    assert _qualifies(gpu)
    a, b = _full_run_both_ways(gpu, x0)
    assert a == b


@pytest.mark.gpu
def test_gpu_first_qp_of_config0(gpu):
    """config 0 (D < 7), 16 seeds, the first Model::optimize() both ways"""
    pci, s, g = pc.cfg(0)
    x0 = configs.seeds_for(0, pci, s, g, 16)
    pc.make_ctx_inputs(gpu, pci, x0)
    assert _qualifies(gpu)
    a, b = _first_qp_both_ways(gpu, x0)
    assert a[1] == b[1]
    assert a[0] == b[0]

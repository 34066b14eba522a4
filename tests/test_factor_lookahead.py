"""Two pivot rows per barrier in the ADMM factorisation of the dense fast path (trajopt_amd/csrc/tmx_factor.h, gj_sep_rows: the owners
of two rows of the separator Schur complement publish them together, every lane advances a private copy of the second row by the first
step and the workgroup barrier is paid once per two elimination steps) - against the per-step forms of the SAME library
(DevProblem::dbg_flags bit 6: gj_rows for the separator inverse) and against the whole generic factorisation (bit 5).  The three must
agree in every bit: solutions byte for byte, every integer of the QP records equal.  Every test first asserts the upload's verdict
(tmx_debug_factor_fast), so the comparison cannot hold trivially.

CPU tier: libtmx_simt.so (tests/test_simt_emulation.py) - the device branches on cooperative fibers with real barriers and poisoned LDS.
GPU tier: the product library - v_rcp_f64 evaluated redundantly in every lane must give the bits of the owner of the row.
"""
import ctypes as C

import numpy as np
import pytest

import parity_checks as pc
from test_simt_emulation import simt, simt_lib  # noqa: F401  (fixtures)
from trajopt_amd import configs

PER_STEP = 64  # DevProblem::dbg_flags bit 6: one elimination step per barrier
GENERIC_FACTOR = 32  # bit 5: the whole generic factorisation
WAYS = (0, PER_STEP, GENERIC_FACTOR)


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


def _first_qp_three_ways(ctx, x0):
    """the first Model::optimize() of the uploaded problem under flags 0, bit 6 and bit 5"""
    out = []
    try:
        for flags in WAYS:
            _set_flags(ctx, flags)
            ctx.set_x0(x0)
            ctx.convexify()
            xq, cvx, rec = ctx.qp_solve()
            out.append((np.asarray(xq).tobytes(), _ints(rec)))
    finally:
        _set_flags(ctx, 0)
    return out


def _full_run_three_ways(ctx, x0):
    """whole optimize() three ways: the results and the integers of every QP record of the run (tmx_sqp_qp_records)"""
    out = []
    try:
        for flags in WAYS:
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


def _assert_first_qp_equal(res):
    a, b, c = res
    assert a[1] == b[1] and a[1] == c[1]
    assert a[0] == b[0]
    assert a[0] == c[0]


def _a_rho_update_happened(ints):
    """the factorisation behind an adaptive-rho update (the call from qp_check_nl), not only the setup's"""
    return any(i[2] > 0 for i in ints)


def _separator_rows(T, D):
    """(number of interiors, rows of the separator system) of the dense nested dissection (dpart_make, tmx_qp.h)"""
    P = min(max((T + 2) // 4, 2), 8)
    if T < 2 * P - 1:
        P = 1
    return P, (P - 1) * D


def test_first_qp_of_baseline_config1(simt):
    """config 1 at its real size (7 x 30), two seeds: ns = 49 = 24 x 2 + 1 and Zst = 56 - the last group is short; interiors of 21 and
    14 rows share the last wave"""
    assert _separator_rows(30, 7) == (8, 49)
    pci, s, g = pc.cfg(1)
    x0 = configs.seeds_for(1, pci, s, g, 2, sigma=0.05)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _qualifies(simt)
    _assert_first_qp_equal(_first_qp_three_ways(simt, x0))


def test_first_qp_of_config1_with_fourteen_waypoints(simt):
    """config 1 with T = 14, two seeds: ns = 21, Zst = 24 - the narrow instantiation (eight register slots, six columns per wave)"""
    assert _separator_rows(14, 7) == (4, 21)
    pci, s, g = pc.cfg(1, T=14)
    x0 = configs.seeds_for(1, pci, s, g, 2, sigma=0.05)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _qualifies(simt)
    _assert_first_qp_equal(_first_qp_three_ways(simt, x0))


def test_whole_optimize_of_config1_short_horizon(simt):
    """config 1 with T = 8, two seeds, the whole optimize(): one separator (ns = 7: three groups and a short one, two columns per
    wave), waves without an interior matrix.  At least one QP record has rho_updates > 0: the call from qp_check_nl is exercised."""
    assert _separator_rows(8, 7) == (2, 7)
    pci, s, g = pc.cfg(1, T=8)
    x0 = configs.seeds_for(1, pci, s, g, 2, sigma=0.05)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _qualifies(simt)
    a, b, c = _full_run_three_ways(simt, x0)
    assert _a_rho_update_happened([i for per_problem in a[3] for i in per_problem])
    assert a == b
    assert a == c


def test_first_qp_of_config1_with_an_even_separator_system(simt):
    """config 1 with T = 10, two seeds: three interiors, ns = 14 - every group is full"""
    assert _separator_rows(10, 7) == (3, 14)
    pci, s, g = pc.cfg(1, T=10)
    x0 = configs.seeds_for(1, pci, s, g, 2, sigma=0.05)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _qualifies(simt)
    _assert_first_qp_equal(_first_qp_three_ways(simt, x0))


@pytest.mark.parametrize("cid", [0, 9])
def test_first_qp_with_fewer_than_seven_joints(simt, cid):
    """D < 7: padded rows, the run-time step loops of the interiors, separator systems of other sizes"""
    pci, s, g = pc.cfg(cid)
    x0 = configs.seeds_for(cid, pci, s, g, 2)
    pc.make_ctx_inputs(simt, pci, x0)
    assert _qualifies(simt)
    _assert_first_qp_equal(_first_qp_three_ways(simt, x0))


def test_a_problem_outside_the_fast_path_is_untouched(simt):
    """config 16 (never on the dense fast path, the upload does not qualify): bit 6 changes nothing"""
    pci, s, g = pc.cfg(16)
    x0 = configs.seeds_for(16, pci, s, g, 2)
    pc.make_ctx_inputs(simt, pci, x0)
    assert not _qualifies(simt)
    a, b, c = _first_qp_three_ways(simt, x0)
    assert a == b
    assert a == c


@pytest.fixture()
def gpu(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_gpu_whole_optimize_of_config1(gpu):
    """BASELINE config 1, 16 seeds, whole optimize() three ways on one context: status, QP counts, trajectories and the integers of
    every QP record"""
    pci, s, g = pc.cfg(1)
    x0 = configs.seeds_for(1, pci, s, g, 16)
    pc.make_ctx_inputs(gpu, pci, x0)
    assert _qualifies(gpu)
    a, b, c = _full_run_three_ways(gpu, x0)
    assert _a_rho_update_happened([i for per_problem in a[3] for i in per_problem])
    assert a == b
    assert a == c


@pytest.mark.gpu
def test_gpu_whole_optimize_of_config1_short_horizon(gpu):
    """config 1 with T = 8 (ns = 7), 16 seeds, whole optimize() three ways"""
    pci, s, g = pc.cfg(1, T=8)
    x0 = configs.seeds_for(1, pci, s, g, 16)
    pc.make_ctx_inputs(gpu, pci, x0)
    assert _qualifies(gpu)
    a, b, c = _full_run_three_ways(gpu, x0)
    assert a == b
    assert a == c


@pytest.mark.gpu
def test_gpu_first_qp_of_config0(gpu):
    """config 0 (D < 7), 16 seeds, the first Model::optimize() three ways"""
    pci, s, g = pc.cfg(0)
    x0 = configs.seeds_for(0, pci, s, g, 16)
    pc.make_ctx_inputs(gpu, pci, x0)
    assert _qualifies(gpu)
    _assert_first_qp_equal(_first_qp_three_ways(gpu, x0))

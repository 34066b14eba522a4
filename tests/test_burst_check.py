"""The in-register residual and certificate check of the epoch-resident ADMM burst (trajopt_amd/csrc/tmx_part.h, admm_burst_core behind
`// ---- EPOCH MODE`: check_far_loads, check_rcps, norms14, certs8, block_max_rows and the decision) is a FILTER in front of qp_check_nl,
the authority: the burst goes on iterating only when the authority could do nothing.  DevProblem::dbg_flags bit 7 takes the filter out
of the SAME library: the burst never continues, and qp_check_nl ignores the norms the burst left and forms its own with the generic
compute_residuals - the authority decides at every check on its own numbers.  Flags 0 and 128 must agree in every bit: solutions byte
for byte, every integer of the QP records equal.  Every test first asserts the upload's verdict (tmx_debug_factor_fast and the other
fast-path verdicts), so the comparison cannot hold trivially.

CPU tier: libtmx_simt.so (tests/test_simt_emulation.py) - the device branches on cooperative fibers with real barriers and poisoned LDS.
GPU tier: the product library - the code the compiler made of the check, its typed global loads and its register allocation.
"""
import ctypes as C

import numpy as np
import pytest

import parity_checks as pc
from test_simt_emulation import simt, simt_lib  # noqa: F401  (fixtures)
from trajopt_amd import abi, configs

AUTHORITY = 128  # DevProblem::dbg_flags bit 7: no in-register filter, qp_check_nl on its own norms at every check
WAYS = (0, AUTHORITY)


def _set_flags(ctx, flags):
    fn = ctx.lib.tmx_debug_set_flags
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], C.c_int
    assert fn(ctx.h, flags) == 0


def _qualifies(ctx):
    """the upload's verdicts: register-resident setup, polish and factorisation - the dense fast path whose ADMM loop is the burst"""
    out = []
    for name in ("setup_fast", "polish_fast", "factor_fast"):
        fn = getattr(ctx.lib, "tmx_debug_" + name)
        fn.argtypes, fn.restype = [C.c_void_p], C.c_int
        out.append(fn(ctx.h))
    return out == [1, 1, 1] and not ctx.workspace_in_hbm()


def _list_lengths(ctx):
    """rows per waypoint (DevProblem::wp_start): n of the A'y sum of norms14"""
    buf = (C.c_int * 256)()
    fn = ctx.lib.tmx_debug_wp_start
    fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_int), C.c_int], C.c_int
    n = fn(ctx.h, buf, 256)
    assert n > 1
    ws = np.asarray(buf[:n])
    return np.diff(ws)


def _ints(rec):
    return [(r.osqp_status, r.osqp_iter, r.rho_updates, r.polish_status, r.hash_active) for r in rec]


def _first_qp_both_ways(ctx, x0):
    """the first Model::optimize() of the uploaded problem under flags 0 and bit 7"""
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


def _full_run_both_ways(ctx, x0):
    """whole optimize() both ways: the results and the integers of every QP record of the run (tmx_sqp_qp_records)"""
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
    a, b = res
    assert a[1] == b[1]
    assert a[0] == b[0]


def _settings(**kw):
    st = abi.default_osqp_settings()
    for k, v in kw.items():
        assert hasattr(st, k)
        setattr(st, k, v)
    return st


def _config1(ctx, T, B, osqp=None):
    pci, s, g = pc.cfg(1) if T is None else pc.cfg(1, T=T)
    x0 = configs.seeds_for(1, pci, s, g, B, sigma=0.05)
    pc.make_ctx_inputs(ctx, pci, x0, osqp=osqp)
    assert _qualifies(ctx)
    return x0


def _first_qp_of_baseline_config1(ctx, B):
    """config 1 at its real size (7 x 30): R > 256, so the last wave runs the two-row instantiations; the goal waypoint has 17 rows (the
    extra pair of the column cache); the lists of the waypoints (7, 10 and 17 rows) leave the remainders n mod 4 = 3, 2 and 1 - config 1 has
    no list of a multiple of four rows at any horizon, _first_qp_with_fewer_joints below brings that one"""
    x0 = _config1(ctx, None, B)
    n = _list_lengths(ctx)
    assert int(n.sum()) > 256
    assert int(n.max()) == 17
    assert set(int(k) & 3 for k in n) == {1, 2, 3}
    _assert_first_qp_equal(_first_qp_both_ways(ctx, x0))


def _first_qp_with_fewer_joints(ctx, cid, B):
    """configs 0 and 9 (D < 7; with the lists of config 1 every remainder n mod 4 occurs): config 9 has a list of exactly four rows - one
    full group and nothing behind it - next to lists of 3, 7, 11 and 14; config 0 has waypoints without any row (n = 0)"""
    pci, s, g = pc.cfg(cid)
    x0 = configs.seeds_for(cid, pci, s, g, B)
    pc.make_ctx_inputs(ctx, pci, x0)
    assert _qualifies(ctx)
    n = _list_lengths(ctx)
    assert (4 if cid == 9 else 0) in [int(k) for k in n]
    assert 0 in set(int(k) & 3 for k in n)
    _assert_first_qp_equal(_first_qp_both_ways(ctx, x0))


def _first_qp_fourteen_waypoints(ctx, B):
    """config 1 with T = 14: four interiors, the narrow instantiation, other list lengths"""
    x0 = _config1(ctx, 14, B)
    _assert_first_qp_equal(_first_qp_both_ways(ctx, x0))


def _whole_run_of_baseline_config1(ctx, B):
    """config 1 at 7 x 30, whole optimize(), every QP record.  At least one record has rho_updates > 0: a burst left for a rho update and
    entered again (the operands of the check are read anew)"""
    x0 = _config1(ctx, None, B)
    a, b = _full_run_both_ways(ctx, x0)
    assert any(i[2] > 0 for per_problem in a[3] for i in per_problem)
    assert a == b


def _first_qp_ending_at_max_iter(ctx, B):
    """max_iter = 60, no multiple of the check interval 25: the burst leaves through `iter_done < max_iter` after a last partial burst of
    ten iterations"""
    x0 = _config1(ctx, 14, B, osqp=_settings(max_iter=60))
    a, b = _first_qp_both_ways(ctx, x0)
    assert all(i[0] == abi.OSQP_MAX_ITER_REACHED and i[1] == 60 for i in a[1])
    _assert_first_qp_equal((a, b))


def _first_qp_checked_every_iteration(ctx, B):
    """check_termination = 1: every iteration is a check - bursts of one (peeled) iteration between two in-register checks.  With
    eps_abs = eps_rel = 1e-2 the termination test ends the solve after about a hundred of them (1e-3 by default: up to 1 400 checks, each
    of which the authority repeats under bit 7)"""
    x0 = _config1(ctx, 14, B, osqp=_settings(check_termination=1, eps_abs=1e-2, eps_rel=1e-2))
    a, b = _first_qp_both_ways(ctx, x0)
    assert all(i[1] > 1 for i in a[1]) and any(i[1] % 25 != 0 for i in a[1])  # (the setting took effect: an end between the default checks)
    _assert_first_qp_equal((a, b))


def test_first_qp_of_baseline_config1(simt):
    _first_qp_of_baseline_config1(simt, 2)


@pytest.mark.parametrize("cid", [0, 9])
def test_first_qp_with_fewer_than_seven_joints(simt, cid):
    _first_qp_with_fewer_joints(simt, cid, 2)


def test_first_qp_of_config1_with_fourteen_waypoints(simt):
    _first_qp_fourteen_waypoints(simt, 2)


def test_whole_optimize_of_baseline_config1(simt):
    _whole_run_of_baseline_config1(simt, 2)


def test_first_qp_ending_at_max_iter(simt):
    _first_qp_ending_at_max_iter(simt, 2)


def test_first_qp_checked_every_iteration(simt):
    _first_qp_checked_every_iteration(simt, 2)


@pytest.fixture()
def gpu(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_gpu_first_qp_of_baseline_config1(gpu):
    _first_qp_of_baseline_config1(gpu, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [0, 9])
def test_gpu_first_qp_with_fewer_than_seven_joints(gpu, cid):
    _first_qp_with_fewer_joints(gpu, cid, 2)


@pytest.mark.gpu
def test_gpu_first_qp_of_config1_with_fourteen_waypoints(gpu):
    _first_qp_fourteen_waypoints(gpu, 2)


@pytest.mark.gpu
def test_gpu_whole_optimize_of_baseline_config1(gpu):
    _whole_run_of_baseline_config1(gpu, 2)


@pytest.mark.gpu
def test_gpu_first_qp_ending_at_max_iter(gpu):
    _first_qp_ending_at_max_iter(gpu, 2)


@pytest.mark.gpu
def test_gpu_first_qp_checked_every_iteration(gpu):
    _first_qp_checked_every_iteration(gpu, 2)

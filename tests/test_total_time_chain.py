"""TotalTime terms on the block-chain QP solver.  A TotalTimeTermInfo (problem_description.cpp:1852-1890,
kinematic_terms.cpp:572-584) couples all time variables: one global row of A (HINGE cost, EQ / INEQ constraint) or the dense
objective block 2 c g g' over tau[1 .. T-1] (SQUARED cost).  Up to the dense engine's size limit (448 QP variables) such problems
keep that engine; above it - the advertised horizons: configuration 50 has 572 variables at 30 waypoints - they used to be refused
and now run on the structured solver, the terms as rank-one corrections K = K_chain + U W U' of the reduced KKT matrix
(TMX_TOTAL_TIME_CHAIN=1 puts a small problem there as well, =0 keeps the dense engine and its refusal).
The yardstick is the oracle and the oracle's own FMA build, stage by stage: exact values, the QP handed to OSQP (integer CSC arrays
bit-exact), the first QP solve, whole SQP histories by class."""
import contextlib
import os

import numpy as np
import pytest

import parity_checks as pc
from trajopt_amd import abi, configs, runtime

SWITCH = "TMX_TOTAL_TIME_CHAIN"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "total_time_dense_parent.npz")
LARGE = ((50, 30), (49, 100), (51, 100))   # 572, 1860 and 1115 QP variables: HINGE cost, INEQ constraint, SQUARED cost
TERMINAL = (abi.OPT_CONVERGED, abi.OPT_SCO_ITERATION_LIMIT, abi.OPT_PENALTY_ITERATION_LIMIT)


def seeds_time(cid, pci, s, g, B, dt0=1.3):
    """joint seeds of the 4-DOF test arm + a time column around dt0 (inside the dt limits of the configurations)"""
    x = configs.seeds_for(9, pci, s, g, B)
    rng = np.random.default_rng(1234 + cid)
    tau = dt0 + 0.3 * rng.standard_normal((B, x.shape[1], 1))
    return np.concatenate([x, np.clip(tau, 0.5, 4.0)], axis=2)


@contextlib.contextmanager
def switch(value):
    """TMX_TOTAL_TIME_CHAIN for the uploads inside the block: "1" the block chain at any size, "0" never, None = unset (the size rule,
    against the dense engine's DEFAULT limit: an override of it that another test module left in the environment is set aside)"""
    old = {k: os.environ.pop(k, None) for k in (SWITCH, "TMX_DENSE_QP_MAX_N")}
    if value is not None:
        os.environ[SWITCH] = value
    try:
        yield
    finally:
        os.environ.pop(SWITCH, None)
        for k, v in old.items():
            if v is not None:
                os.environ[k] = v


# ---- the problems ------------------------------------------------------------------------------------------------------------------
def _plain_time_problem():
    """a TotalTime HINGE cost in an otherwise plain use_time problem: no row on two waypoints (R2 = 0) - without the term this QP takes
    the register-resident dense fast path on the device, which knows nothing of global rows"""
    from trajopt_amd.problem import TotalTimeTermInfo
    pci, s, g = configs.config_mini()
    n = pci.basic_info.n_steps
    pci.basic_info.use_time = True
    pci.basic_info.dt_lower_lim, pci.basic_info.dt_upper_lim = 0.4, 6.0
    pci.cost_infos.append(TotalTimeTermInfo(coeff=2.0, limit=0.2 * (n - 1), name="total_time"))
    return pci, s, g, seeds_time(60, pci, s, g, 2)


def _two_terms_problem():
    """configuration 50 (TotalTime HINGE cost) + a TotalTime INEQ constraint: two rank-one terms"""
    from trajopt_amd.problem import TotalTimeTermInfo
    pci, s, g = pc.cfg(50)
    n = pci.basic_info.n_steps
    pci.cnt_infos.insert(0, TotalTimeTermInfo(coeff=1.0, limit=0.7 * (n - 1), is_constraint=True, name="total_time_limit"))
    return pci, s, g, seeds_time(61, pci, s, g, 2)


def _slack_hinge_problem():
    """configuration 50 with a limit the seeds stay far below (sum 1 / tau ~ 0.77 (n - 1) < 5 (n - 1)): the hinge is slack, the
    row is outside the polish's active set and enters that factorisation with weight zero"""
    from trajopt_amd.problem import TotalTimeTermInfo
    pci, s, g = pc.cfg(50)
    n = pci.basic_info.n_steps
    for ti in pci.cost_infos:
        if isinstance(ti, TotalTimeTermInfo):
            ti.limit = 5.0 * (n - 1)
    return pci, s, g, seeds_time(62, pci, s, g, 2)


def _seven_dof_problem(B=2):
    """D + 1 = 8: the 7-DOF arm of configs.config1 (glass_upright, 30 waypoints) as a time-optimal problem - velocity limits with time as
    INEQ constraints, TotalTime HINGE cost; the numbers of the mini configurations (tolerance 0.25, dt limits 0.4 .. 6, tau seeds
    1.3 +- 0.3, limit 0.2 (T - 1), coefficient 2), for which the oracle's first QP is solved"""
    from trajopt_amd.problem import JointVelTermInfo, TotalTimeTermInfo
    pci, s, g = configs.config1()
    D, n = pci.robot.n_dof, pci.basic_info.n_steps
    pci.basic_info.use_time = True
    pci.basic_info.dt_lower_lim, pci.basic_info.dt_upper_lim = 0.4, 6.0
    pci.cnt_infos.insert(0, JointVelTermInfo(coeffs=[1.0] * D, targets=[0.0] * D, first_step=0, last_step=n - 1, use_time=True, is_constraint=True,
                                             upper_tols=[0.25] * D, lower_tols=[-0.25] * D, name="vel_lim"))
    pci.cost_infos.append(TotalTimeTermInfo(coeff=2.0, limit=0.2 * (n - 1), name="total_time"))
    x = configs.seeds_for(1, pci, s, g, B)
    rng = np.random.default_rng(1234 + 63)
    tau = 1.3 + 0.3 * rng.standard_normal((B, x.shape[1], 1))
    return pci, s, g, np.concatenate([x, np.clip(tau, 0.5, 4.0)], axis=2)


SHAPES = {"no_pair_rows": _plain_time_problem, "two_terms": _two_terms_problem, "slack_hinge": _slack_hinge_problem, "seven_dof": _seven_dof_problem}


# ---- the checks --------------------------------------------------------------------------------------------------------------------
def _first_qp_records(o, desc, x0):
    out = []
    for b in range(x0.shape[0]):
        r = o.first_qp(desc, x0[b])["rec"]
        out.append((r.osqp_status, r.osqp_iter, r.rho_updates, r.polish_status))
    return out


def _stage_by_stage(make_ctx, orc, orc_fma, pci, x0, expect_solved=False):
    """exact values, QP structure (integer CSC arrays bit-exact: the export and the hashes need no knowledge of the engine) and the
    first QP solve.  STRICT (same iteration count, rho updates, polish status, active set; solution within TOL_TRAJ) on every seed
    on which the oracle and its FMA build produce the same first-QP record; on the others the status and the KKT certificate hold."""
    B = x0.shape[0]
    ctx = make_ctx()
    desc = pc.make_ctx_inputs(ctx, pci, x0)
    pc.check_evaluate(ctx, orc, desc, x0, 1e-12)
    for b in range(B):
        pc.check_first_qp_structure(ctx, orc, desc, x0, b, 1e-12)
    ctx.close()
    ra, rf = _first_qp_records(orc, desc, x0), _first_qp_records(orc_fma, desc, x0)
    strict = [b for b in range(B) if ra[b] == rf[b]]
    loose = [b for b in range(B) if ra[b] != rf[b]]
    print(f"first QP: strict form on {len(strict)} of {B} seeds, {len(loose)} left out (the two oracle builds disagree there); oracle records {ra}")
    if expect_solved:
        assert all(r[0] == abi.OSQP_SOLVED for r in ra), ra
    for group, same_iters in ((strict, True), (loose, False)):
        if group:
            ctx = make_ctx()
            pc.make_ctx_inputs(ctx, pci, x0[group])
            res = pc.check_first_qp_solve(ctx, orc, desc, x0[group], require_same_iters=same_iters)
            print(f"  require_same_iters={same_iters}: (same, |dx|) = {[(s, float(np.round(d, 9))) for s, d in res]}")
            ctx.close()
    return len(strict)


def _history_check(ctx, orc, orc_fma, pci, x0):
    """the rule of test_time_terms._history_check: whole SQP runs QP by QP, never in class "other" / "csc-noise", drift within the
    budget the oracle shows against its own FMA build, as many good seeds as the two oracle builds agree on (minus one)"""
    B = x0.shape[0]
    desc = pc.make_ctx_inputs(ctx, pci, x0)
    classes, dx, _ = pc.sqp_history_classes(ctx, orc, desc, x0)
    r0, r1 = orc.sqp_batch(desc, x0), orc_fma.sqp_batch(desc, x0)
    same_builds = int(((r0["n_qp_solves"] == r1["n_qp_solves"]) & (np.abs(r0["x"] - r1["x"]).reshape(B, -1).max(axis=1) < 1e-5)).sum())
    good = sum(c in ("identical", "tie") for c in classes)
    print(f"classes {classes}, |dx| {np.round(dx, 7)}, oracle vs FMA oracle same on {same_builds}/{B}")
    assert "other" not in classes and "csc-noise" not in classes
    assert classes.count("drift") <= pc.drift_budget(B, pc.oracle_self_classes(orc, orc_fma, desc, x0)), classes
    assert good >= max(1, same_builds - 1)
    return classes


def _runs_to_a_terminal_status(ctx, pci, x0, over_the_limit=True):
    pc.make_ctx_inputs(ctx, pci, x0)
    assert ctx.n_max > 448 or not over_the_limit
    ctx.run(0)
    r = ctx.results()
    assert all(int(st) in TERMINAL for st in r["status"]), r["status"]
    assert np.isfinite(r["x"]).all()
    return r


def _whole_sqp_of_a_shape(ctx, orc, orc_fma, pci, x0, shape):
    """the shapes on the 4-DOF arm by the history rule.  The 7-DOF time-optimal problem has no yardstick for whole runs: its first QPs
    take 3 - 4 thousand ADMM iterations, and the oracle and its own FMA build keep the same run (QP count, trajectory within 1e-5 rad)
    on 0 of 2 seeds - there the first QP is the check (strict, above) and the run has to reach a terminal status with a finite
    trajectory."""
    if shape == "seven_dof":
        _runs_to_a_terminal_status(ctx, pci, x0)
    else:
        _history_check(ctx, orc, orc_fma, pci, x0)


def _both_engines(make_ctx, orc, cid, B=4):
    """one small problem on the dense engine (switch unset and "0") and on the block chain ("1"): same first-QP integer record and
    active set, primal solutions within TOL_TRAJ - and both against the oracle (the dense engine alone is no yardstick)"""
    pci, s, g = pc.cfg(cid)
    x0 = seeds_time(cid, pci, s, g, B)
    got = {}
    for sw in (None, "0", "1"):
        with switch(sw):
            ctx = make_ctx()
            desc = pc.make_ctx_inputs(ctx, pci, x0)
            pc.check_first_qp_solve(ctx, orc, desc, x0)
            ctx.convexify()
            xq, cvx, rec = ctx.qp_solve()
            flags = ctx.qp_active_set()
            got[sw] = (xq.copy(), [(r.n, r.m, r.nnzP, r.hashP, r.nnzA, r.hashA, r.osqp_status, r.osqp_iter, r.rho_updates, r.polish_status, r.hash_active)
                                   for r in rec], flags.copy())
            ctx.close()
    for sw in (None, "0"):
        assert got[sw][1] == got["1"][1], f"switch {sw}: first-QP records differ between the engines"
        assert np.array_equal(got[sw][2], got["1"][2])
        dx = np.abs(got[sw][0] - got["1"][0]).max()
        print(f"config {cid}, switch {sw} vs 1: |dx| {dx:.3e}")
        assert dx <= pc.TOL_TRAJ


# ---- CPU tier (host build) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,T", LARGE)
def test_total_time_problems_over_the_dense_limit_upload_and_run(hostemu_lib, cid, T):
    """item 1: refused with TMX_ERR_UNSUPPORTED ("dense engine") before TotalTime terms ran on the block chain"""
    pci, s, g = pc.cfg(cid, T=T)
    with switch(None):
        ctx = runtime.Context(0, hostemu_lib)
        _runs_to_a_terminal_status(ctx, pci, seeds_time(cid, pci, s, g, 4))
        ctx.close()


@pytest.mark.parametrize("cid,T", LARGE)
def test_large_total_time_problems_stage_by_stage_on_host_build(hostemu_lib, orc, orc_fma, cid, T):
    pci, s, g = pc.cfg(cid, T=T)
    x0 = seeds_time(cid, pci, s, g, 8)
    with switch(None):
        n_strict = _stage_by_stage(lambda: runtime.Context(0, hostemu_lib), orc, orc_fma, pci, x0)
    assert n_strict >= 1
    if cid in (49, 51):   # (the two oracle builds agree on every seed of these: the strict cases)
        assert n_strict == 8


@pytest.mark.parametrize("cid", (49, 50, 51))
def test_small_total_time_problems_stage_by_stage_on_the_chain(hostemu_lib, orc, orc_fma, cid):
    pci, s, g = pc.cfg(cid)
    x0 = seeds_time(cid, pci, s, g, 4)
    with switch("1"):
        assert _stage_by_stage(lambda: runtime.Context(0, hostemu_lib), orc, orc_fma, pci, x0) >= 1


@pytest.mark.parametrize("cid,T", LARGE)
def test_large_total_time_problems_whole_sqp_on_host_build(hostemu_lib, orc, orc_fma, cid, T):
    pci, s, g = pc.cfg(cid, T=T)
    with switch(None):
        ctx = runtime.Context(0, hostemu_lib)
        _history_check(ctx, orc, orc_fma, pci, seeds_time(cid, pci, s, g, 8))
        ctx.close()


@pytest.mark.parametrize("cid", (49, 51))
def test_both_engines_agree_on_a_small_problem(hostemu_lib, orc, cid):
    _both_engines(lambda: runtime.Context(0, hostemu_lib), orc, cid)


@pytest.mark.parametrize("cid", (49, 50, 51))
def test_problems_under_the_limit_keep_the_dense_engine_bit_for_bit(hostemu_lib, cid):
    """the no-change guarantee: with the switch unset the small problems give the bytes they gave before TotalTime terms could run on
    the block chain (tests/golden/total_time_dense_parent.npz: status, counters and trajectories of 4 seeds, recorded from the host
    build of the commit before)"""
    gold = np.load(GOLDEN)
    pci, s, g = pc.cfg(cid)
    x0 = seeds_time(cid, pci, s, g, 4)
    with switch(None):
        ctx = runtime.Context(0, hostemu_lib)
        pc.make_ctx_inputs(ctx, pci, x0)
        ctx.run(0)
        r = ctx.results()
        ctx.close()
    for k in ("status", "n_qp_solves", "n_func_evals"):
        assert np.array_equal(r[k], gold[f"cfg{cid}_{k}"]), k
    assert r["x"].tobytes() == gold[f"cfg{cid}_x"].tobytes()
    assert r["total_cost"].tobytes() == gold[f"cfg{cid}_total_cost"].tobytes()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shapes_stage_by_stage_and_whole_sqp_on_host_build(hostemu_lib, orc, orc_fma, shape):
    pci, s, g, x0 = SHAPES[shape]()
    with switch("1"):
        _stage_by_stage(lambda: runtime.Context(0, hostemu_lib), orc, orc_fma, pci, x0, expect_solved=(shape == "seven_dof"))
        ctx = runtime.Context(0, hostemu_lib)
        _whole_sqp_of_a_shape(ctx, orc, orc_fma, pci, x0, shape)
        ctx.close()


def test_the_slack_hinge_row_is_outside_the_polish_active_set(hostemu_lib):
    """... so that the polish of that problem factors the correction with a zero weight (no division by it)"""
    pci, s, g, x0 = _slack_hinge_problem()
    with switch("1"):
        ctx = runtime.Context(0, hostemu_lib)
        pc.make_ctx_inputs(ctx, pci, x0)
        ctx.convexify()
        xq, cvx, rec = ctx.qp_solve()
        flags = ctx.qp_active_set()
        e = ctx.export_csc(0)
        ctx.close()
    assert rec[0].osqp_status == abi.OSQP_SOLVED and rec[0].polish_status != 0   # (the polish ran: accepted or not, it factored the system)
    A = pc.csc_dense_ops(e)[1].tocsr()
    D1 = pci.robot.n_dof + 1
    n_traj = pci.basic_info.n_steps * D1
    rows = [i for i in range(e["m"] - e["n"]) if set(A[i, :n_traj].indices) == {t * D1 + D1 - 1 for t in range(1, pci.basic_info.n_steps)}]
    assert len(rows) == 1, "the global row of the TotalTime cost"
    assert flags[0, rows[0]] == 0
    assert np.isfinite(xq[0, :rec[0].n]).all()


def test_correction_data_in_the_per_problem_scratch(hostemu_lib, orc, orc_fma):
    """the data of the correction live behind the QP workspace, or - when they alone would push an LDS-resident workspace out of
    the LDS - in the per-problem scratch: TMX_TT_PLACE=2 (test hook) puts a small problem there"""
    pci, s, g = pc.cfg(49)
    x0 = seeds_time(49, pci, s, g, 2)
    os.environ["TMX_TT_PLACE"] = "2"
    try:
        with switch("1"):
            assert _stage_by_stage(lambda: runtime.Context(0, hostemu_lib), orc, orc_fma, pci, x0) >= 1
    finally:
        del os.environ["TMX_TT_PLACE"]


def test_refusals_that_remain(hostemu_lib):
    """five TotalTime terms are more than the block chain carries: dense engine, refused above its limit with a message that says why;
    TMX_TOTAL_TIME_CHAIN=0 is the refusal of before"""
    from trajopt_amd.problem import TotalTimeTermInfo
    pci, s, g = pc.cfg(50, T=30)
    n = pci.basic_info.n_steps
    for k in range(4):
        pci.cost_infos.append(TotalTimeTermInfo(coeff=0.5, limit=(0.3 + 0.1 * k) * (n - 1), name=f"total_time_{k}"))
    with switch(None):
        ctx = runtime.Context(0, hostemu_lib)
        with pytest.raises(runtime.TmxError, match="more than 4 TotalTime terms.*dense engine"):
            pc.make_ctx_inputs(ctx, pci, seeds_time(50, pci, s, g, 1))
        ctx.close()
    pci, s, g = pc.cfg(50, T=30)
    with switch("0"):
        ctx = runtime.Context(0, hostemu_lib)
        with pytest.raises(runtime.TmxError, match="TMX_TOTAL_TIME_CHAIN=0.*dense engine"):
            pc.make_ctx_inputs(ctx, pci, seeds_time(50, pci, s, g, 1))
        ctx.close()
    # four terms are carried
    pci, s, g = pc.cfg(50, T=30)
    for k in range(3):
        pci.cost_infos.append(TotalTimeTermInfo(coeff=0.5, limit=(0.3 + 0.1 * k) * (n - 1), name=f"total_time_{k}"))
    with switch(None):
        ctx = runtime.Context(0, hostemu_lib)
        _runs_to_a_terminal_status(ctx, pci, seeds_time(50, pci, s, g, 1))
        ctx.close()


# ---- CPU tier: the device branches of the kernels on the SIMT emulation (256 cooperative fibers per workgroup) --------------------------
@pytest.fixture(scope="module")
def simt_lib():
    import subprocess
    hostemu_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("the ROCm toolchain's clang (host compiler of the SIMT emulation) is not installed")
    subprocess.check_call(["make", "-C", hostemu_dir, "simt"], stdout=subprocess.DEVNULL)
    return os.path.join(hostemu_dir, "_build", "libtmx_simt.so")


def test_simt_emulation_gives_the_host_builds_bits(hostemu_lib, simt_lib, orc, orc_fma):
    """256 threads per workgroup (the device branches: out-of-line ADMM loop, wave-walked chain sweeps) and one thread per workgroup
    give the same first-QP integer record and active set and the same solution (the two builds differ in the last bits elsewhere:
    the cost normalisation of the device branch is a tree sum) - and the emulation passes the oracle's checks"""
    pci, s, g = pc.cfg(50, T=30)
    x0 = seeds_time(50, pci, s, g, 2)
    sols = []
    with switch(None):
        for lib in (hostemu_lib, simt_lib):
            ctx = runtime.Context(0, lib)
            pc.make_ctx_inputs(ctx, pci, x0)
            ctx.convexify()
            xq, cvx, rec = ctx.qp_solve()
            sols.append((xq.copy(), [(r.osqp_status, r.osqp_iter, r.rho_updates, r.polish_status, r.hash_active) for r in rec]))
            ctx.close()
        assert sols[0][1] == sols[1][1]
        assert np.abs(sols[0][0] - sols[1][0]).max() <= pc.TOL_TRAJ
        _stage_by_stage(lambda: runtime.Context(0, simt_lib), orc, orc_fma, pci, x0)


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cid,T", LARGE)
def test_large_total_time_problems_on_device(gpu_ctx_factory, orc, orc_fma, cid, T):
    B = 32 if cid == 50 else 8   # (config 50 = the reference's arm_around_table with time: 32 seeds, as test_time_terms)
    pci, s, g = pc.cfg(cid, T=T)
    x0 = seeds_time(cid, pci, s, g, B)
    with switch(None):
        ctx = gpu_ctx_factory()
        _runs_to_a_terminal_status(ctx, pci, x0)
        ctx.close()
        n_strict = _stage_by_stage(gpu_ctx_factory, orc, orc_fma, pci, x0[:8])
        assert n_strict >= 1
        if cid in (49, 51):
            assert n_strict == 8
        ctx = gpu_ctx_factory()
        _history_check(ctx, orc, orc_fma, pci, x0)
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", (49, 51))
def test_both_engines_agree_on_a_small_problem_on_device(gpu_ctx_factory, orc, cid):
    _both_engines(gpu_ctx_factory, orc, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ("no_pair_rows", "seven_dof"))
def test_shapes_on_device(gpu_ctx_factory, orc, orc_fma, shape):
    pci, s, g, x0 = SHAPES[shape]()
    with switch("1"):
        _stage_by_stage(gpu_ctx_factory, orc, orc_fma, pci, x0, expect_solved=(shape == "seven_dof"))
        ctx = gpu_ctx_factory()
        _whole_sqp_of_a_shape(ctx, orc, orc_fma, pci, x0, shape)
        ctx.close()

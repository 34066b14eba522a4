"""Squared acceleration / jerk costs next to rows on two waypoints with dense coupling blocks.  A squared
JointAcc / JointJerk cost makes the objective block banded (couplings at distance 2 / 3 waypoints, diagonal blocks); LVS_DISCRETE /
CONTINUOUS / LVS_CONTINUOUS collision rows and CartVel rows couple consecutive waypoints with DENSE blocks.  Up to the dense engine's
size limit (448 QP variables) the combination keeps that engine; above it such problems used to be refused and now run on the banded
block factorisation with a dense first coupling (DevProblem::band_pairs; TMX_BAND_PAIR_CHAIN=1 puts a small problem there as well, =0
keeps the dense engine and its refusal).
The yardstick is the oracle and the oracle's own FMA build, stage by stage: exact values, the QP handed to OSQP (integer CSC arrays
bit-exact), the first QP solve (strict on every seed), whole SQP histories by class - the helpers and the rules of
tests/test_vel_time_chain.py."""
import contextlib
import os

import numpy as np
import pytest

import parity_checks as pc
from trajopt_amd import abi, configs, runtime

SWITCH = "TMX_BAND_PAIR_CHAIN"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "band_pair_dense_parent.npz")
TERMINAL = (abi.OPT_CONVERGED, abi.OPT_SCO_ITERATION_LIMIT, abi.OPT_PENALTY_ITERATION_LIMIT)
N_SEEDS = 8
N_SMALL = 4
K_STEPS = 4  # configs.config3 at the smallest number of waypoints whose QP workspace (with the cost) leaves the LDS: 326 656 B; 118 520 B at 3


@contextlib.contextmanager
def switch(value):
    """TMX_BAND_PAIR_CHAIN for the uploads inside the block: "1" the banded route at any size, "0" never, None = unset (the size rule,
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
def acc_cost(D, n, coeffs=(2.0, 1.0, 0.5, 1.5, 1.0, 1.0, 1.0)):
    from trajopt_amd.problem import JointAccTermInfo
    return JointAccTermInfo(coeffs=list(coeffs)[:D], targets=[0.0] * D, first_step=0, last_step=n - 1, name="acc_smooth")


def jerk_cost(D, n):
    from trajopt_amd.problem import JointJerkTermInfo
    return JointJerkTermInfo(coeffs=[1.0, 0.5, 2.0, 1.0, 1.0, 1.0, 1.0][:D], targets=[0.0] * D, first_step=0, last_step=n - 1, name="jerk_smooth")


def _mini(cid, T, acc, jerk, B):
    """the 4-DOF test arm with a cast / LVS collision cost (16, 17) or a CartVel constraint (23) plus the smoothing costs"""
    pci, s, g = pc.cfg(cid, T=T)
    D, n = pci.robot.n_dof, pci.basic_info.n_steps
    if acc:
        pci.cost_infos.append(acc_cost(D, n))
    if jerk:
        pci.cost_infos.append(jerk_cost(D, n))
    return pci, configs.seeds_for(9, pci, s, g, B)


def _glass(T, B):
    """glass_upright (configs.config1: 7 joints) with every collision term on the LVS_CONTINUOUS evaluator plus an acceleration cost"""
    from trajopt_amd.problem import CollisionTermInfo
    pci, s, g = configs.config1() if T is None else configs.config1(T)
    for ti in pci.cost_infos + pci.cnt_infos:
        if isinstance(ti, CollisionTermInfo):
            ti.evaluator_type, ti.longest_valid_segment_length, ti.max_substates = 4, 0.12, 4
    pci.cost_infos.append(acc_cost(pci.robot.n_dof, pci.basic_info.n_steps))
    return pci, configs.seeds_for(1, pci, s, g, B)


def _car_seat(B):
    """BASELINE configuration 3 (car_seat: 10 joints, LVS collision rows) plus an acceleration cost with coefficients 1: the
    HBM-workspace kernels"""
    pci, s, g = configs.config3(K_STEPS)
    D, n = pci.robot.n_dof, pci.basic_info.n_steps
    pci.cost_infos.append(acc_cost(D, n, coeffs=[1.0] * D))
    return pci, configs.seeds_for(3, pci, s, g, B)


# over the dense engine's size limit
PROBLEMS = {
    "E": lambda B=N_SEEDS: _mini(17, 30, True, False, B),
    "F": lambda B=N_SEEDS: _mini(17, 30, True, True, B),
    "G": lambda B=N_SEEDS: _mini(23, 45, False, True, B),
    "H": lambda B=N_SEEDS: _glass(None, B),
    "K": lambda B=N_SMALL: _car_seat(B),
}
# small shapes (TMX_BAND_PAIR_CHAIN=1): S2 / S2b band 3 reaching both ends of the horizon; S3 block size 7 (band_sweeps_wave<7>); S5 CartVel rows
SMALL = {
    "S1": lambda B=N_SMALL: _mini(17, 14, True, True, B),
    "S2": lambda B=N_SMALL: _mini(17, 6, False, True, B),
    "S2b": lambda B=N_SMALL: _mini(17, 5, False, True, B),
    "S3": lambda B=N_SMALL: _glass(8, B),
    "S5": lambda B=N_SMALL: _mini(23, 14, True, False, B),
}
ALL = dict(PROBLEMS, **SMALL)


# ---- the checks --------------------------------------------------------------------------------------------------------------------
def _on_the_route(ctx, over_the_limit):
    assert ctx.band_pairs() and ctx.debug_flag("qp_dense") == 0
    if over_the_limit:
        assert ctx.n_max > 448


def _leaves_the_lds(ctx, expected):
    """the QP workspace of the uploaded problem lives in HBM (the k_*_hbm kernels).  The host build has no such kernels and always says
    in_hbm = 0; it reports the workspace's size, and the rule of the upload is size > 160 KB of LDS"""
    ws = ctx.workspace_info()
    assert (ws["in_hbm"] or ws["lds_bytes"] > 160 * 1024) == expected, ws


def _stage_by_stage(make_ctx, orc, pci, x0, over_the_limit=False):
    """exact values, QP structure (integer CSC arrays and hashes bit-exact: the export needs no knowledge of the engine) and the first
    QP solve in its STRICT form on every seed: same iteration count, rho updates, polish status and active set, solution within TOL_TRAJ"""
    ctx = make_ctx()
    desc = pc.make_ctx_inputs(ctx, pci, x0)
    _on_the_route(ctx, over_the_limit)
    pc.check_evaluate(ctx, orc, desc, x0, 1e-12)
    for b in range(x0.shape[0]):
        pc.check_first_qp_structure(ctx, orc, desc, x0, b, 1e-12)
    ctx.close()
    ctx = make_ctx()
    pc.make_ctx_inputs(ctx, pci, x0)
    res = pc.check_first_qp_solve(ctx, orc, desc, x0, require_same_iters=True)
    print(f"first QP, strict form on all {x0.shape[0]} seeds: (same, |dx|) = {[(s, float(np.round(d, 9))) for s, d in res]}")
    ctx.close()


def _history_check(ctx, orc, orc_fma, pci, x0):
    """the rule of test_vel_time_chain._history_check: whole SQP runs QP by QP, never in class "other" / "csc-noise", drift within the
    budget the oracle shows against its own FMA build, as many good seeds as the two oracle builds agree on (minus one)"""
    B = x0.shape[0]
    desc = pc.make_ctx_inputs(ctx, pci, x0)
    _on_the_route(ctx, False)
    classes, dx, _ = pc.sqp_history_classes(ctx, orc, desc, x0)
    r0, r1 = orc.sqp_batch(desc, x0), orc_fma.sqp_batch(desc, x0)
    same_builds = int(((r0["n_qp_solves"] == r1["n_qp_solves"]) & (np.abs(r0["x"] - r1["x"]).reshape(B, -1).max(axis=1) < 1e-5)).sum())
    good = sum(c in ("identical", "tie") for c in classes)
    print(f"classes {classes}, |dx| {np.round(dx, 7)}, oracle vs FMA oracle same on {same_builds}/{B}")
    assert "other" not in classes and "csc-noise" not in classes
    assert classes.count("drift") <= pc.drift_budget(B, pc.oracle_self_classes(orc, orc_fma, desc, x0)), classes
    assert good >= max(1, same_builds - 1)
    return classes


def _runs_to_a_terminal_status(ctx, pci, x0):
    pc.make_ctx_inputs(ctx, pci, x0)
    _on_the_route(ctx, True)
    ctx.run(0)
    r = ctx.results()
    assert all(int(st) in TERMINAL for st in r["status"]), r["status"]
    assert np.isfinite(r["x"]).all()
    return r


def _first_qp(ctx):
    ctx.convexify()
    xq, cvx, rec = ctx.qp_solve()
    flags = ctx.qp_active_set()
    return (xq.copy(), [(r.n, r.m, r.nnzP, r.hashP, r.nnzA, r.hashA, r.osqp_status, r.osqp_iter, r.rho_updates, r.polish_status, r.hash_active)
                        for r in rec], flags.copy())


def _both_engines(make_ctx, orc, name):
    """one small problem on the dense engine (switch unset and "0") and on the banded route ("1"): same first-QP integer record and
    active set, primal solutions within TOL_TRAJ - and both against the oracle (the dense engine alone is no yardstick)"""
    pci, x0 = SMALL[name]()
    got = {}
    for sw in (None, "0", "1"):
        with switch(sw):
            ctx = make_ctx()
            desc = pc.make_ctx_inputs(ctx, pci, x0)
            assert ctx.n_max <= 448 and ctx.band_pairs() == (sw == "1") and ctx.debug_flag("qp_dense") == (0 if sw == "1" else 1)
            pc.check_first_qp_solve(ctx, orc, desc, x0)
            got[sw] = _first_qp(ctx)
            ctx.close()
    for sw in (None, "0"):
        assert got[sw][1] == got["1"][1], f"switch {sw}: first-QP records differ between the engines"
        assert np.array_equal(got[sw][2], got["1"][2])
        dx = np.abs(got[sw][0] - got["1"][0]).max()
        print(f"{name}, switch {sw} vs 1: |dx| {dx:.3e}")
        assert dx <= pc.TOL_TRAJ


# ---- CPU tier (host build) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_problems_over_the_dense_limit_upload_and_run(hostemu_lib, name):
    """item 1: refused with TMX_ERR_UNSUPPORTED ("dense engine") before the banded factorisation took a dense first coupling"""
    pci, x0 = PROBLEMS[name](B=2)
    with switch(None):
        ctx = runtime.Context(0, hostemu_lib)
        _runs_to_a_terminal_status(ctx, pci, x0)
        if name == "K":
            _leaves_the_lds(ctx, True)
        ctx.close()


def test_problem_k_is_the_smallest_car_seat_in_hbm(hostemu_lib):
    """one waypoint less and the QP workspace of configuration 3 with the cost stays in the LDS"""
    pci, s, g = configs.config3(K_STEPS - 1)
    D, n = pci.robot.n_dof, pci.basic_info.n_steps
    pci.cost_infos.append(acc_cost(D, n, coeffs=[1.0] * D))
    with switch(None):
        ctx = runtime.Context(0, hostemu_lib)
        pc.make_ctx_inputs(ctx, pci, configs.seeds_for(3, pci, s, g, 1))
        assert ctx.band_pairs()
        _leaves_the_lds(ctx, False)
        ctx.close()


@pytest.mark.parametrize("name", ("E", "F", "G", "H"))
def test_problems_stage_by_stage_on_host_build(hostemu_lib, orc, name):
    pci, x0 = PROBLEMS[name]()
    with switch(None):
        _stage_by_stage(lambda: runtime.Context(0, hostemu_lib), orc, pci, x0, over_the_limit=True)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_shapes_stage_by_stage_on_host_build(hostemu_lib, orc, name):
    pci, x0 = SMALL[name]()
    with switch("1"):
        _stage_by_stage(lambda: runtime.Context(0, hostemu_lib), orc, pci, x0)


@pytest.mark.parametrize("name", ("E", "F", "G", "S1", "S3"))
def test_problems_whole_sqp_on_host_build(hostemu_lib, orc, orc_fma, name):
    """whole SQP runs by the history rule (H runs whole on the GPU tier only)"""
    pci, x0 = ALL[name]()
    with switch(None if name in PROBLEMS else "1"):
        ctx = runtime.Context(0, hostemu_lib)
        _history_check(ctx, orc, orc_fma, pci, x0)
        ctx.close()


@pytest.mark.parametrize("name", ("S1", "S3"))
def test_both_engines_agree(hostemu_lib, orc, name):
    _both_engines(lambda: runtime.Context(0, hostemu_lib), orc, name)


@pytest.mark.parametrize("name", ("S1", "S3"))
def test_problems_under_the_limit_keep_the_dense_engine_bit_for_bit(hostemu_lib, name):
    """the no-change guarantee: with the switch unset the small problems give the bytes they gave before the banded route existed
    (tests/golden/band_pair_dense_parent.npz: status, counters, trajectories and total cost of 4 seeds, recorded from the host build of
    the commit before by tools/record_band_pair_dense_golden.py)"""
    gold = np.load(GOLDEN)
    pci, x0 = SMALL[name](4)
    with switch(None):
        ctx = runtime.Context(0, hostemu_lib)
        pc.make_ctx_inputs(ctx, pci, x0)
        assert ctx.n_max <= 448 and not ctx.band_pairs() and ctx.debug_flag("qp_dense") == 1
        ctx.run(0)
        r = ctx.results()
        ctx.close()
    for k in ("status", "n_qp_solves", "n_func_evals"):
        assert np.array_equal(r[k], gold[f"{name}_{k}"]), k
    assert r["x"].tobytes() == gold[f"{name}_x"].tobytes()
    assert r["total_cost"].tobytes() == gold[f"{name}_total_cost"].tobytes()


def test_refusals_that_remain(hostemu_lib):
    """what stays on the dense engine is refused above its limit with a message that says why"""
    from trajopt_amd.problem import Ex, FuncCostTermInfo, JointAccTermInfo, sq

    def refused(pci, x0, sw, pattern):
        with switch(sw):
            ctx = runtime.Context(0, hostemu_lib)
            with pytest.raises(runtime.TmxError, match=pattern):
                pc.make_ctx_inputs(ctx, pci, x0)
            ctx.close()

    # TMX_BAND_PAIR_CHAIN=0 is the refusal of before
    pci, x0 = PROBLEMS["E"](B=1)
    refused(pci, x0, "0", "acceleration / jerk costs next to rows on two waypoints.*with TMX_BAND_PAIR_CHAIN=0.*dense engine")
    # acceleration ROWS (an INEQ constraint) next to the collision rows keep the dense engine, with or without the cost
    pci, x0 = PROBLEMS["E"](B=1)
    D, n = pci.robot.n_dof, pci.basic_info.n_steps
    pci.cnt_infos.append(JointAccTermInfo(coeffs=[1.0] * D, targets=[0.0] * D, first_step=0, last_step=n - 1, upper_tols=[0.3] * D,
                                          lower_tols=[-0.3] * D, is_constraint=True, name="acc_limits"))
    for sw in (None, "1"):
        refused(pci, x0, sw, "acceleration / jerk rows next to collision / CartVel rows on two waypoints.*dense engine")
    # the cost next to a function cost (dynamic objective blocks)
    pci, x0 = PROBLEMS["E"](B=1)
    x = [Ex.var(i) for i in range(D)]
    pci.cost_infos.append(FuncCostTermInfo(f=0.2 * sq(x[0] - 0.3 * x[1]) + 0.1 * sq(x[2] + x[3]), first_step=1, last_step=n - 2, full_hessian=True, name="bowl"))
    for sw in (None, "1"):
        refused(pci, x0, sw, "acceleration / jerk costs next to rows on two waypoints or function costs \\(here: function costs\\).*dense engine")


# ---- CPU tier: the device branches of the kernels on the SIMT emulation (256 cooperative fibers per workgroup) --------------------------
@pytest.fixture(scope="module")
def simt_lib():
    import subprocess
    hostemu_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("the ROCm toolchain's clang (host compiler of the SIMT emulation) is not installed")
    subprocess.check_call(["make", "-C", hostemu_dir, "simt"], stdout=subprocess.DEVNULL)
    return os.path.join(hostemu_dir, "_build", "libtmx_simt.so")


def test_simt_emulation_gives_the_host_builds_bytes(hostemu_lib, simt_lib):
    """256 threads per workgroup (the device branches: out-of-line ADMM loop, wave-walked band sweeps) and one thread per workgroup:
    first QP and one whole run of S1 on the banded route, byte for byte (every sum of this route is formed by one thread per entry:
    none follows the number of threads)"""
    pci, x0 = SMALL["S1"](2)
    first, runs = [], []
    with switch("1"):
        for lib in (hostemu_lib, simt_lib):
            ctx = runtime.Context(0, lib)
            pc.make_ctx_inputs(ctx, pci, x0)
            _on_the_route(ctx, False)
            xq, rec, flags = _first_qp(ctx)
            first.append((xq.tobytes(), rec, flags.tobytes()))
            ctx.close()
            ctx = runtime.Context(0, lib)
            pc.make_ctx_inputs(ctx, pci, x0)
            ctx.run(0)
            r = ctx.results()
            runs.append((r["status"].tobytes(), r["n_qp_solves"].tobytes(), r["n_func_evals"].tobytes(), r["x"].tobytes(), r["total_cost"].tobytes()))
            ctx.close()
    assert first[0][1] == first[1][1]
    assert first[0] == first[1]
    assert runs[0] == runs[1]


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_shapes_on_device(gpu_ctx_factory, orc, name):
    pci, x0 = SMALL[name]()
    with switch("1"):
        _stage_by_stage(gpu_ctx_factory, orc, pci, x0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("S1", "S3"))
def test_both_engines_agree_on_device(gpu_ctx_factory, orc, name):
    _both_engines(gpu_ctx_factory, orc, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("E", "H"))
def test_problems_on_device(gpu_ctx_factory, orc, orc_fma, name):
    pci, x0 = PROBLEMS[name]()
    with switch(None):
        ctx = gpu_ctx_factory()
        _runs_to_a_terminal_status(ctx, pci, x0)
        ctx.close()
        _stage_by_stage(gpu_ctx_factory, orc, pci, x0, over_the_limit=True)
        ctx = gpu_ctx_factory()
        _history_check(ctx, orc, orc_fma, pci, x0)
        ctx.close()


@pytest.mark.gpu
def test_car_seat_in_the_hbm_workspace_on_device(gpu_ctx_factory, orc):
    pci, x0 = PROBLEMS["K"]()
    with switch(None):
        ctx = gpu_ctx_factory()
        _runs_to_a_terminal_status(ctx, pci, x0)
        assert ctx.workspace_info()["in_hbm"]
        ctx.close()
        _stage_by_stage(gpu_ctx_factory, orc, pci, x0, over_the_limit=True)

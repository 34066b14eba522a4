"""Acceleration / jerk ROWS next to rows on two waypoints with dense coupling blocks.  JointAcc / JointJerk
inequality (hinge) costs and equality / inequality constraints are difference rows of order 2 / 3 on one joint; LVS_DISCRETE /
CONTINUOUS / LVS_CONTINUOUS collision rows and CartVel rows couple consecutive waypoints with DENSE blocks.  The combination keeps the
dense engine (refused above 448 QP variables) unless the upload hook TMX_BAND_ROW_PAIR_CHAIN=1 is set: then the problem runs on the
banded block factorisation with a dense first coupling (DevProblem::band_rows and band_pairs both), at any size, and its polish carries
that factorisation in double-double.
The yardstick is the oracle and the oracle's own FMA build, stage by stage: exact values, the QP handed to OSQP (integer CSC arrays
bit-exact), the first QP solve in its strict form, whole SQP histories by class - the helpers and the rules of
tests/test_band_pair_chain.py, whose small builders are copied here.
Hinge bands can make the polish active set rank-deficient; round-off then decides the reference's own outcome (the comment in
tests/test_joint_costs_kat.py).  The strict form of the first QP solve is therefore demanded on every seed whose first-QP record the
oracle's plain and FMA builds agree on, and at most ONE seed per problem may be left out this way (the oracle pair alone is asserted
to stay within that cap)."""
import contextlib
import os

import numpy as np
import pytest

import parity_checks as pc
from trajopt_amd import abi, configs, runtime

SWITCH = "TMX_BAND_ROW_PAIR_CHAIN"
TERMINAL = (abi.OPT_CONVERGED, abi.OPT_SCO_ITERATION_LIMIT, abi.OPT_PENALTY_ITERATION_LIMIT)
N_SEEDS = 8
N_SMALL = 4
K_STEPS = 4  # configs.config3 at the smallest number of waypoints whose QP workspace leaves the LDS (tests/test_band_pair_chain.py)


@contextlib.contextmanager
def switch(value):
    """TMX_BAND_ROW_PAIR_CHAIN for the uploads inside the block: "1" the banded route at any size, "0" / None (unset) the dense engine
    and its limit.  TMX_DENSE_QP_MAX_N and TMX_BAND_PAIR_CHAIN that another test module left in the environment are set aside."""
    old = {k: os.environ.pop(k, None) for k in (SWITCH, "TMX_DENSE_QP_MAX_N", "TMX_BAND_PAIR_CHAIN")}
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


def acc_limits(D, n, tol=0.3):
    from trajopt_amd.problem import JointAccTermInfo
    return JointAccTermInfo(coeffs=[1.0] * D, targets=[0.0] * D, first_step=0, last_step=n - 1, upper_tols=[tol] * D, lower_tols=[-tol] * D,
                            is_constraint=True, name="acc_limits")


def acc_pinned(D, first, last):
    """acceleration EQ constraint on a stretch of steps: pinned second differences (the conditioning the dd polish is for)"""
    from trajopt_amd.problem import JointAccTermInfo
    return JointAccTermInfo(coeffs=[1.0] * D, targets=[0.0] * D, first_step=first, last_step=last, is_constraint=True, name="acc_pinned")


def jerk_hinge(D, n, tol=0.05):
    from trajopt_amd.problem import JointJerkTermInfo
    return JointJerkTermInfo(coeffs=[2.0, 1.0, 1.5, 1.0, 1.0, 1.0, 1.0][:D], targets=[0.0] * D, first_step=0, last_step=n - 1, upper_tols=[tol] * D,
                             lower_tols=[-tol] * D, name="jerk_hinge")


def jerk_limits(D, n, tol=0.4):
    from trajopt_amd.problem import JointJerkTermInfo
    return JointJerkTermInfo(coeffs=[1.0] * D, targets=[0.0] * D, first_step=0, last_step=n - 1, upper_tols=[tol] * D, lower_tols=[-tol] * D,
                             is_constraint=True, name="jerk_limits")


def _mini(cid, T, B, costs=(), cnts=()):
    """the 4-DOF test arm with an LVS collision cost (17) or a CartVel constraint (23) plus difference-row terms"""
    pci, s, g = pc.cfg(cid, T=T)
    D, n = pci.robot.n_dof, pci.basic_info.n_steps
    for make in costs:
        pci.cost_infos.append(make(D, n))
    for make in cnts:
        pci.cnt_infos.append(make(D, n))
    return pci, configs.seeds_for(9, pci, s, g, B)


def _glass(T, B, evaluator=4, lvs=0.12, sub=4):
    """glass_upright (configs.config1: 7 joints) with its collision terms on an LVS evaluator plus acceleration limits"""
    from trajopt_amd.problem import CollisionTermInfo
    pci, s, g = configs.config1() if T is None else configs.config1(T)
    for ti in pci.cost_infos + pci.cnt_infos:
        if isinstance(ti, CollisionTermInfo):
            ti.evaluator_type, ti.longest_valid_segment_length, ti.max_substates = evaluator, lvs, sub
    pci.cnt_infos.append(acc_limits(pci.robot.n_dof, pci.basic_info.n_steps))
    return pci, configs.seeds_for(1, pci, s, g, B)


def _car_seat(B):
    """BASELINE configuration 3 (car_seat: 10 joints, LVS collision rows) at 4 waypoints plus acceleration limits: HBM workspace, band 2"""
    pci, s, g = configs.config3(K_STEPS)
    pci.cnt_infos.append(acc_limits(pci.robot.n_dof, pci.basic_info.n_steps))
    return pci, configs.seeds_for(3, pci, s, g, B)


# the smallest shapes at which each piece can go wrong
SMALL = {
    "R1": lambda B=N_SMALL: _mini(17, 6, B, cnts=(acc_limits,)),                                     # band 2 from rows alone
    "R2": lambda B=N_SMALL: _mini(17, 5, B, costs=(jerk_hinge,)),                                    # band 3 reaching both ends of the horizon
    "R3": lambda B=N_SMALL: _mini(17, 14, B, costs=(acc_cost, jerk_hinge), cnts=(lambda D, n: acc_pinned(D, 4, 9),)),  # costs and rows; pinned stretch
    "R4": lambda B=N_SMALL: _glass(8, B),                                                            # D = 7: band_sweeps_wave<7>
    "R5": lambda B=N_SMALL: _mini(23, 14, B, cnts=(jerk_limits,)),                                   # CartVel rows next to order-3 rows
}
# over the dense engine's size limit
PROBLEMS = {
    "P1": lambda B=N_SEEDS: _mini(17, 30, B, costs=(acc_cost,), cnts=(acc_limits,)),   # problem "E" of test_band_pair_chain.py + acceleration limits
    "P2": lambda B=N_SMALL: _glass(None, B, evaluator=2, lvs=0.2, sub=2),              # the problem tests/test_joint_costs_kat.py pins
    "P3": lambda B=N_SMALL: _car_seat(B),
}
ALL = dict(PROBLEMS, **SMALL)


# ---- the checks --------------------------------------------------------------------------------------------------------------------
def _on_the_route(ctx, over_the_limit=False):
    assert ctx.band_row_pairs() and ctx.debug_flag("qp_dense") == 0
    if over_the_limit:
        assert ctx.n_max > 448


def _leaves_the_lds(ctx, expected):
    """the host build has no HBM-workspace kernels and always says in_hbm = 0; it reports the workspace's size, and the rule of the
    upload is size > 160 KB of LDS"""
    ws = ctx.workspace_info()
    assert (ws["in_hbm"] or ws["lds_bytes"] > 160 * 1024) == expected, ws


def _oracle_record(o, desc, x):
    q = o.first_qp(desc, x)
    r = q["rec"]
    return (r.osqp_status, r.osqp_iter, r.rho_updates, r.polish_status, r.hash_active), q["x"]


def _oracle_pair_agrees(orc, orc_fma, desc, x0):
    """per seed: do the oracle and its FMA build give the same first-QP record (status, iterations, rho updates, polish status, active set)
    and solutions within TOL_TRAJ?  At most one seed per problem may part (module docstring)."""
    agree = []
    for b in range(x0.shape[0]):
        (r0, xa), (r1, xb) = _oracle_record(orc, desc, x0[b]), _oracle_record(orc_fma, desc, x0[b])
        agree.append(r0 == r1 and float(np.abs(xa - xb).max()) <= pc.TOL_TRAJ)
    assert agree.count(False) <= 1, f"the oracle pair alone parts on {agree.count(False)} seeds: {agree}"
    return agree


def _first_qp_strict(make_ctx, orc, orc_fma, pci, x0, desc):
    agree = _oracle_pair_agrees(orc, orc_fma, desc, x0)
    ctx = make_ctx()
    pc.make_ctx_inputs(ctx, pci, x0)
    res = pc.check_first_qp_solve(ctx, orc, desc, x0, require_same_iters=False)
    ctx.close()
    print(f"first QP: oracle pair agrees {agree}, (strict, |dx|) = {[(s, float(np.round(d, 9))) for s, d in res]}")
    for b, ((same, dx), ok) in enumerate(zip(res, agree)):
        if ok:
            assert same, f"seed {b}: first QP solve not in the strict form (the oracle's two builds agree on this seed)"
            assert dx <= pc.TOL_TRAJ


def _stage_by_stage(make_ctx, orc, orc_fma, pci, x0, over_the_limit=False):
    """exact values, QP structure (integer CSC arrays and hashes bit-exact) on every seed and the first QP solve in its STRICT form: same
    iteration count, rho updates, polish status and active set, solution within TOL_TRAJ - on every seed on which the oracle's two builds
    agree (module docstring)"""
    ctx = make_ctx()
    desc = pc.make_ctx_inputs(ctx, pci, x0)
    _on_the_route(ctx, over_the_limit)
    pc.check_evaluate(ctx, orc, desc, x0, 1e-12)
    for b in range(x0.shape[0]):
        pc.check_first_qp_structure(ctx, orc, desc, x0, b, 1e-12)
    ctx.close()
    _first_qp_strict(make_ctx, orc, orc_fma, pci, x0, desc)


def _history_check(ctx, orc, orc_fma, pci, x0):
    """the rule of test_band_pair_chain._history_check: whole SQP runs QP by QP, never in class "other" / "csc-noise", drift within the
    budget the oracle shows against its own FMA build, as many good seeds as the two oracle builds agree on (minus one)"""
    B = x0.shape[0]
    desc = pc.make_ctx_inputs(ctx, pci, x0)
    _on_the_route(ctx)
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
    """one small problem on the dense engine (hook unset) and on the banded route ("1"): same first-QP integer record and active set,
    primal solutions within TOL_TRAJ - and both against the oracle (the dense engine alone is no yardstick)"""
    pci, x0 = SMALL[name]()
    got = {}
    for sw in (None, "1"):
        with switch(sw):
            ctx = make_ctx()
            desc = pc.make_ctx_inputs(ctx, pci, x0)
            assert ctx.n_max <= 448 and ctx.band_row_pairs() == (sw == "1") and ctx.debug_flag("qp_dense") == (0 if sw == "1" else 1)
            pc.check_first_qp_solve(ctx, orc, desc, x0)
            got[sw] = _first_qp(ctx)
            ctx.close()
    assert got[None][1] == got["1"][1], "first-QP records differ between the engines"
    assert np.array_equal(got[None][2], got["1"][2])
    dx = np.abs(got[None][0] - got["1"][0]).max()
    print(f"{name}, dense engine vs banded route: |dx| {dx:.3e}")
    assert dx <= pc.TOL_TRAJ


# ---- CPU tier (host build) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL))
def test_every_shape_uploads_on_the_route(hostemu_lib, name):
    """refused ("dense engine") above the limit, on the dense engine below it, before the route existed - and still with the hook unset"""
    pci, x0 = ALL[name](B=1)
    with switch("1"):
        ctx = runtime.Context(0, hostemu_lib)
        pc.make_ctx_inputs(ctx, pci, x0)
        _on_the_route(ctx, name in PROBLEMS)
        _leaves_the_lds(ctx, name in ("P2", "P3"))  # (P2: 30 waypoints of 7 joints with LVS_DISCRETE rows - 322 KB; band 2 in both)
        ctx.close()
    with switch(None):
        ctx = runtime.Context(0, hostemu_lib)
        if name in PROBLEMS:
            with pytest.raises(runtime.TmxError, match="acceleration / jerk rows next to collision / CartVel rows on two waypoints or to time-parameterised terms: the QP"):
                pc.make_ctx_inputs(ctx, pci, x0)
        else:
            pc.make_ctx_inputs(ctx, pci, x0)
            assert not ctx.band_row_pairs() and not ctx.band_pairs() and ctx.debug_flag("qp_dense") == 1
        ctx.close()


@pytest.mark.parametrize("name", sorted(SMALL) + ["P1"])
def test_stage_by_stage_on_host_build(hostemu_lib, orc, orc_fma, name):
    pci, x0 = ALL[name]()
    with switch("1"):
        _stage_by_stage(lambda: runtime.Context(0, hostemu_lib), orc, orc_fma, pci, x0, over_the_limit=name in PROBLEMS)


def test_p2_stage_by_stage_on_host_build(hostemu_lib, orc, orc_fma):
    pci, x0 = PROBLEMS["P2"](2)
    with switch("1"):
        _stage_by_stage(lambda: runtime.Context(0, hostemu_lib), orc, orc_fma, pci, x0, over_the_limit=True)


@pytest.mark.parametrize("name", ("R1", "R3", "R4", "P1"))
def test_whole_sqp_on_host_build(hostemu_lib, orc, orc_fma, name):
    pci, x0 = ALL[name]()
    with switch("1"):
        ctx = runtime.Context(0, hostemu_lib)
        _history_check(ctx, orc, orc_fma, pci, x0)
        ctx.close()


@pytest.mark.parametrize("name", ("R1", "R4"))
def test_both_engines_agree(hostemu_lib, orc, name):
    _both_engines(lambda: runtime.Context(0, hostemu_lib), orc, name)


def test_refusals_that_remain_with_the_hook(hostemu_lib):
    """TMX_BAND_ROW_PAIR_CHAIN=1 does not reach function costs, time-parameterised problems or the trajopt_sqp flavour: refused above the
    dense engine's limit with a message that says what stands in the way"""
    from trajopt_amd.problem import Ex, FuncCostTermInfo, TotalTimeTermInfo, sq

    def refused(pci, x0, pattern):
        with switch("1"):
            ctx = runtime.Context(0, hostemu_lib)
            with pytest.raises(runtime.TmxError, match=pattern):
                pc.make_ctx_inputs(ctx, pci, x0)
            ctx.close()

    head = "acceleration / jerk rows next to collision / CartVel rows on two waypoints or to time-parameterised terms \\(TMX_BAND_ROW_PAIR_CHAIN=1 does not apply: "
    # next to a function cost (dynamic objective blocks)
    pci, x0 = PROBLEMS["P1"](B=1)
    D, n = pci.robot.n_dof, pci.basic_info.n_steps
    x = [Ex.var(i) for i in range(D)]
    pci.cost_infos.append(FuncCostTermInfo(f=0.2 * sq(x[0] - 0.3 * x[1]) + 0.1 * sq(x[2] + x[3]), first_step=1, last_step=n - 2, full_hessian=True, name="bowl"))
    refused(pci, x0, head + "function costs\\).*dense engine")
    # inside a use_time problem
    pci, x0 = PROBLEMS["P1"](B=1)
    pci.basic_info.use_time = True
    pci.basic_info.dt_lower_lim, pci.basic_info.dt_upper_lim = 0.05, 2.0
    pci.cost_infos.append(TotalTimeTermInfo(coeff=1.0, limit=0.0, name="total_time"))
    refused(pci, x0, head + "time-parameterised terms\\).*dense engine")
    # in the trajopt_sqp flavour
    pci, x0 = PROBLEMS["P1"](B=1)
    pci.flavor = abi.FLAVOR_SQP
    pci.basic_info.fixed_timesteps, pci.basic_info.fixed_dofs = [], []   # (not part of the trajopt_sqp path)
    # (that flavour lowers JointAcc / JointJerk terms as squared costs only: the rows are refused by the lowering, before any engine choice)
    refused(pci, x0, "this term kind is not lowered for the trajopt_sqp flavour")


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
    """256 threads per workgroup (the device branches: out-of-line ADMM loop, out-of-line banded routines, wave-walked band sweeps) and
    one thread per workgroup: first QP and one whole run of R3, byte for byte (every sum of this route is formed by one thread per entry
    in a fixed order: none follows the number of threads)"""
    pci, x0 = SMALL["R3"](2)
    first, runs = [], []
    with switch("1"):
        for lib in (hostemu_lib, simt_lib):
            ctx = runtime.Context(0, lib)
            pc.make_ctx_inputs(ctx, pci, x0)
            _on_the_route(ctx)
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


def test_assembly_against_the_operator_in_a_debug_build(tmp_path):
    """host debug build (TMX_DEBUG_KKT): the assembled Sinv / Cd / bk2 / bk3 of the polish of R3 against the operator
    K = diag + bands + sum_r w_r a_r a_r' applied to unit vectors"""
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = str(tmp_path / "libtmx_hostemu_dbg.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fopenmp", "-fPIC", "-ffp-contract=off", "-DTMX_HOST_EMU", "-DTMX_DEBUG_KKT", "-DTMX_LINK_ROWS=1", "-w",
                           "-shared", "-o", lib, os.path.join(root, "trajopt_amd", "csrc", "tmx_api.cpp")])
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_band_row_pair_chain as m, parity_checks as pc\n"
            "from trajopt_amd import runtime\n"
            "pci, x0 = m.SMALL['R3'](1)\n"
            "with m.switch('1'):\n"
            "    ctx = runtime.Context(0, %r); pc.make_ctx_inputs(ctx, pci, x0); assert ctx.band_row_pairs(); ctx.convexify(); ctx.qp_solve(); ctx.close()\n"
            % (root, os.path.join(root, "tests"), lib))
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert out.returncode == 0, out.stdout
    worst = [float(v) for v in re.findall(r"polish assembly vs operator: worst \|diff\| (\S+)", out.stdout)]
    resid = [(float(a), float(b)) for a, b in re.findall(r"reduced solve: \|K x - b\| (\S+)\s+\|b\| (\S+)", out.stdout)]
    print(f"assembly vs operator: {worst}; reduced solves (|Kx - b|, |b|): {resid[:4]} ...")
    assert worst, out.stdout
    # the entries are sums of a few dozen products of size <= w_max = 1 / delta = 1e6 times O(1) scaled coefficients: 1e-16 relative
    # rounding per term, two summation orders - 1e-8 absolute is 100 x that and far below any entry a wrong term would add (>= w a^2)
    assert max(worst) <= 1e-8


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_shapes_on_device(gpu_ctx_factory, orc, orc_fma, name):
    pci, x0 = SMALL[name]()
    with switch("1"):
        _stage_by_stage(gpu_ctx_factory, orc, orc_fma, pci, x0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("R1", "R4"))
def test_both_engines_agree_on_device(gpu_ctx_factory, orc, name):
    _both_engines(gpu_ctx_factory, orc, name)


@pytest.mark.gpu
def test_p1_on_device(gpu_ctx_factory, orc, orc_fma):
    pci, x0 = PROBLEMS["P1"]()
    with switch("1"):
        ctx = gpu_ctx_factory()
        _runs_to_a_terminal_status(ctx, pci, x0)
        ctx.close()
        _stage_by_stage(gpu_ctx_factory, orc, orc_fma, pci, x0, over_the_limit=True)
        ctx = gpu_ctx_factory()
        _history_check(ctx, orc, orc_fma, pci, x0)
        ctx.close()


@pytest.mark.gpu
def test_p2_on_device(gpu_ctx_factory, orc, orc_fma):
    """terminal status with 2 seeds, the first QP stage by stage with 4 (no whole-run classes: the glass-size difference-row runs are the
    slow tests of the tier)"""
    with switch("1"):
        pci, x0 = PROBLEMS["P2"](2)
        ctx = gpu_ctx_factory()
        _runs_to_a_terminal_status(ctx, pci, x0)
        ctx.close()
        pci, x0 = PROBLEMS["P2"](4)
        _stage_by_stage(gpu_ctx_factory, orc, orc_fma, pci, x0, over_the_limit=True)


@pytest.mark.gpu
def test_car_seat_in_the_hbm_workspace_on_device(gpu_ctx_factory, orc, orc_fma):
    pci, x0 = PROBLEMS["P3"]()
    with switch("1"):
        ctx = gpu_ctx_factory()
        _runs_to_a_terminal_status(ctx, pci, x0)
        assert ctx.workspace_info()["in_hbm"]
        ctx.close()
        _stage_by_stage(gpu_ctx_factory, orc, orc_fma, pci, x0, over_the_limit=True)

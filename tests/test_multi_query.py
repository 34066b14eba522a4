"""Multi-query batches (include/tmx.h: tmx_queries_set, tmx_query_set_targets, tmx_argmin_queries, tmx_best_trajectories): a batch of
Q queries x S seeds that share the uploaded description and differ in the goal targets of their cart-pose and joint-position terms.

The yardstick is the library's own one-query path, which the parity tiers hold to the oracle: a query of a multi-query batch must give
the BYTES of the same seeds run alone, on a fresh context whose description carries that query's targets - x, status, total_cost,
n_func_evals, n_qp_solves and every integer of every QP record.  That rests on one property, checked first on the unchanged path:
a problem's arithmetic does not depend on what else is in the batch.

Tiers: the host build (libtmx_hostemu.so), the SIMT emulation (libtmx_simt.so: the device branches, the fused evaluation of the fast
step, the wave reduction of k_argmin_queries) and, marked gpu, the product library on the device.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import parity_checks as pc
from test_simt_emulation import simt_lib  # noqa: F401  (fixture)
from trajopt_amd import abi, configs, runtime
from trajopt_amd.problem import CartPoseTermInfo, JointPosTermInfo

GENERIC_EVAL = 16  # DevProblem::dbg_flags bit 4
KEYS = ("x", "status", "total_cost", "n_func_evals", "n_qp_solves")


@pytest.fixture(params=["host", "simt", pytest.param("gpu", marks=pytest.mark.gpu)])
def make_ctx(request):
    """a factory of contexts of the tier; every context it made is closed at the end"""
    made = []
    if request.param == "gpu":
        factory = request.getfixturevalue("gpu_ctx_factory")
    else:
        lib = request.getfixturevalue("hostemu_lib" if request.param == "host" else "simt_lib")
        factory = lambda: runtime.Context(0, lib)  # noqa: E731

    def make():
        made.append(factory())
        return made[-1]
    make.tier = request.param
    yield make
    for c in made:
        c.close()


def _set_flags(ctx, flags):
    fn = ctx.lib.tmx_debug_set_flags
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], C.c_int
    assert fn(ctx.h, flags) == 0


def _eval_fast(ctx):
    fn = ctx.lib.tmx_debug_eval_fast
    fn.argtypes, fn.restype = [C.c_void_p], C.c_int
    return fn(ctx.h)


def _snapshot(ctx, lo=0, hi=None, cap=128):
    """results() and the integers of every QP record of problems lo .. hi - 1, as bytes / integers"""
    r = ctx.results()
    hi = ctx.B if hi is None else hi
    recs, cnt = ctx.qp_records(cap)
    assert int(cnt.max()) <= cap
    ints = [[recs[b * cap + k].key() for k in range(int(cnt[b]))] for b in range(lo, hi)]
    return tuple(np.ascontiguousarray(r[k][lo:hi]).tobytes() for k in KEYS), ints


def _upload(ctx, pci):
    desc = pci.to_desc()
    ctx.upload(desc, abi.default_sqp_params(), abi.default_osqp_settings())
    return desc


def _target_of(ti):
    return np.asarray(ti.target_pose, np.float64).reshape(-1)[:12] if isinstance(ti, CartPoseTermInfo) else np.asarray(ti.targets, np.float64)


def _send_targets(ctx, pcis):
    """set_queries(len(pcis)) on a context that holds pcis[0], then the targets of every cart-pose / joint-position term in which some
    query differs from pcis[0]; returns the term indices that were sent"""
    Q = len(pcis)
    ctx.set_queries(Q)
    terms = [list(p.cost_infos) + list(p.cnt_infos) for p in pcis]
    sent = []
    for k, ti in enumerate(terms[0]):
        if not isinstance(ti, (CartPoseTermInfo, JointPosTermInfo)):
            continue
        rows = np.stack([_target_of(terms[q][k]) for q in range(Q)])
        if any(rows[q].tobytes() != rows[0].tobytes() for q in range(Q)):
            assert pcis[0].term_index(ti) == k
            ctx.set_query_targets(k, rows)
            sent.append(k)
    return sent


def _compare_with_separate_uploads(make_ctx, pcis, x0s, flags=(0,), want_eval_fast=None):
    """the multi-query batch (description pcis[0], query q with the targets of pcis[q] and the seeds x0s[q]) under every dbg_flags value
    of `flags` against one fresh context per query; returns the multi-query context (holding the batch of the last flags value)"""
    Q, S = len(pcis), x0s[0].shape[0]
    ctx = make_ctx()
    _upload(ctx, pcis[0])
    if want_eval_fast is not None:
        assert _eval_fast(ctx) == want_eval_fast
    assert _send_targets(ctx, pcis)
    multi = []
    for fl in flags:
        _set_flags(ctx, fl)
        ctx.set_x0(np.concatenate(x0s))
        assert ctx.run(0) == 0
        multi.append([_snapshot(ctx, q * S, (q + 1) * S) for q in range(Q)])
    _set_flags(ctx, 0)
    for m in multi[1:]:
        assert m == multi[0]   # the generic and the fused evaluation give equal bytes to each other
    for q in range(Q):
        alone = make_ctx()
        _upload(alone, pcis[q])
        alone.set_x0(x0s[q])
        assert alone.run(0) == 0
        ref = _snapshot(alone)
        assert len(ref[1]) == S and all(len(per) >= 1 for per in ref[1])
        assert multi[0][q][1] == ref[1], f"query {q}: QP record integers differ"
        assert multi[0][q][0] == ref[0], f"query {q}: result bytes differ"
    # the queries are different problems: their runs differ from each other
    assert len({multi[0][q][0][0] for q in range(Q)}) == Q
    return ctx


def _rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _config1_queries(T=8):
    """glass_upright at a short horizon: query 0 = the description's own targets, query 1 = another joint goal inside the limits and an
    upright target tilted by 0.2 rad about x, query 2 = a third goal"""
    goals = [None, configs.CFG1_GOAL + np.array([-0.3, 0.1, 0.15, 0.1, -0.2, 0.1, 0.2]),
             configs.CFG1_GOAL + np.array([0.25, -0.1, -0.1, -0.15, 0.1, -0.1, -0.25])]
    pcis, x0s = [], []
    for q, goal in enumerate(goals):
        pci, s, g = pc.cfg(1, T=T)
        if goal is not None:
            assert np.all(goal > pci.robot.lower + 1e-2) and np.all(goal < pci.robot.upper - 1e-2)
            pci.cnt_infos[-1].targets = list(goal)
            g = goal
        if q == 1:
            for ti in pci.cnt_infos:
                if isinstance(ti, CartPoseTermInfo):
                    pose = np.array(ti.target_pose, dtype=np.float64).reshape(3, 4)
                    pose[:, :3] = _rot_x(0.2) @ pose[:, :3]
                    ti.target_pose = pose
        pcis.append(pci)
        x0s.append(configs.seeds_for(1, pci, s, g, 2, sigma=0.05, first=2))
    return pcis, x0s


def _mini_queries():
    """configs.config_mini (4 DOF, 14 waypoints, a position-only cart-pose constraint, a joint band, a joint goal, collision): query 1
    moves the via point, the band centre and the goal"""
    pcis, x0s = [], []
    for q in range(2):
        pci, s, g = configs.config_mini()
        if q == 1:
            g = configs.MINI_GOAL + np.array([-0.2, 0.1, -0.15, 0.2])
            pci.cnt_infos[-1].targets = list(g)
            band = pci.cnt_infos[-2]
            assert band.name == "band"
            band.targets = list(np.asarray(band.targets) + np.array([0.05, -0.03, 0.04, 0.02]))
            via = np.array(pci.cnt_infos[0].target_pose, dtype=np.float64).reshape(3, 4)
            via[:, 3] += np.array([0.02, -0.03, 0.02])
            pci.cnt_infos[0].target_pose = via
        pcis.append(pci)
        x0s.append(configs.seeds_for(9, pci, s, g, 2))
    return pcis, x0s


# ---- the property everything below rests on, on the unchanged one-query path ---------------------------------------------------

@pytest.mark.parametrize("which", ["config1_T8", "mini"])
def test_a_problem_does_not_depend_on_the_rest_of_the_batch(make_ctx, which):
    """the same two seeds in a batch of 2 and in a batch of 6 (one query, no query call at all): equal bytes"""
    if which == "config1_T8":
        pci, s, g = pc.cfg(1, T=8)
        x0 = configs.seeds_for(1, pci, s, g, 6, sigma=0.05, first=2)
    else:
        pci, s, g = configs.config_mini()
        x0 = configs.seeds_for(9, pci, s, g, 6)
    ctx = make_ctx()
    _upload(ctx, pci)
    ctx.set_x0(x0)
    assert ctx.run(0) == 0
    six = _snapshot(ctx, 0, 2)
    ctx.set_x0(x0[:2])
    assert ctx.run(0) == 0
    assert _snapshot(ctx) == six


# ---- case 1: state and refusals -------------------------------------------------------------------------------------------

def _refused(status, text, fn, *args):
    with pytest.raises(runtime.TmxError) as e:
        fn(*args)
    assert str(e.value).startswith(f"tmx status {status}:"), str(e.value)
    assert text in str(e.value), str(e.value)


def test_state_and_refusals(make_ctx):
    ctx = make_ctx()
    _refused(abi.TMX_ERR_STATE, "no problem uploaded", ctx.set_queries, 2)
    ctx.Q = 2
    _refused(abi.TMX_ERR_STATE, "no problem uploaded", ctx.set_query_targets, 0, np.zeros((2, 4)))
    pci, s, g = configs.config_mini(n_steps=6, with_pos_costs=True)
    # a cart-pose term with a tolerance band goes the function-term way
    tol = copy.deepcopy(pci.cnt_infos[0])
    tol.timestep, tol.lower_tolerance, tol.upper_tolerance = 2, [-0.01] * 6, [0.01] * 6
    pci.cnt_infos.append(tol)
    terms = list(pci.cost_infos) + list(pci.cnt_infos)
    k_vel, k_posture, k_soft = 0, pci.term_index(pci.cost_infos[2]), pci.term_index(pci.cost_infos[3])
    k_via, k_goal, k_tol = pci.term_index(pci.cnt_infos[0]), pci.term_index(pci.cnt_infos[-2]), pci.term_index(tol)
    assert pci.cost_infos[2].name == "posture" and pci.cost_infos[3].name == "soft_band"
    x0 = configs.seeds_for(10, pci, s, g, 4)
    _upload(ctx, pci)
    ctx.set_x0(x0[:2])
    _refused(abi.TMX_ERR_INVALID, "at least 1", ctx.set_queries, 0)
    ctx.Q = 2   # (the binding's own shape check; the library still has one query)
    _refused(abi.TMX_ERR_STATE, "one query", ctx.set_query_targets, k_goal, np.zeros((2, 4)))
    # while a launch is pending
    ctx.launch()
    _refused(abi.TMX_ERR_STATE, "pending", ctx.set_queries, 2)
    _refused(abi.TMX_ERR_STATE, "pending", ctx.set_query_targets, k_goal, np.zeros((2, 4)))
    ctx.wait()
    ctx.results()
    # the calls invalidate the batch: nothing runs or reads it until the next set_x0
    ctx.set_queries(2)
    for call in (lambda: ctx.run(0), ctx.launch, ctx.evaluate, ctx.convexify, ctx.results, ctx.argmin_queries, ctx.best_trajectories):
        _refused(abi.TMX_ERR_STATE, "", call)
    goal2 = np.stack([g, g + 0.05])
    ctx.set_x0(x0)
    ctx.evaluate()
    ctx.set_query_targets(k_goal, goal2)
    for call in (lambda: ctx.run(0), ctx.launch, ctx.evaluate, ctx.convexify):
        _refused(abi.TMX_ERR_STATE, "", call)
    # accepted kinds: cart-pose instances (12), joint-position constraints and the inequality cost (n_dof)
    ctx.set_query_targets(k_via, np.stack([_target_of(terms[k_via])] * 2))
    ctx.set_query_targets(k_soft, np.stack([_target_of(terms[k_soft])] * 2))
    ctx.set_query_targets(pci.term_index(pci.cnt_infos[1]), np.stack([_target_of(pci.cnt_infos[1])] * 2))   # the band: an inequality constraint
    # refused kinds, each with its reason
    _refused(abi.TMX_ERR_UNSUPPORTED, "no per-query target", ctx.set_query_targets, k_vel, np.zeros((2, 4)))
    _refused(abi.TMX_ERR_UNSUPPORTED, "static objective", ctx.set_query_targets, k_posture, np.zeros((2, 4)))
    _refused(abi.TMX_ERR_UNSUPPORTED, "function term", ctx.set_query_targets, k_tol, np.zeros((2, 12)))
    # bad index, wrong len, non-finite values
    _refused(abi.TMX_ERR_INVALID, "term index", ctx.set_query_targets, -1, goal2)
    _refused(abi.TMX_ERR_INVALID, "term index", ctx.set_query_targets, len(terms), goal2)
    _refused(abi.TMX_ERR_INVALID, "len must be 4", ctx.set_query_targets, k_goal, np.zeros((2, 5)))
    _refused(abi.TMX_ERR_INVALID, "len must be 12", ctx.set_query_targets, k_via, np.zeros((2, 4)))
    bad = goal2.copy()
    bad[1, 2] = np.nan
    _refused(abi.TMX_ERR_INVALID, "non-finite", ctx.set_query_targets, k_goal, bad)
    bad[1, 2] = np.inf
    _refused(abi.TMX_ERR_INVALID, "non-finite", ctx.set_query_targets, k_goal, bad)
    # a batch holds the same number of seeds for every query
    _refused(abi.TMX_ERR_INVALID, "batch % n_queries", ctx.set_x0, x0[:3])
    _refused(abi.TMX_ERR_INVALID, "batch % n_queries", ctx.set_x0_device, x0.ctypes.data, 3)
    ctx.set_x0(x0)
    ctx.evaluate()
    # one query again: any batch size; a new upload returns to one query as well
    ctx.set_queries(1)
    _refused(abi.TMX_ERR_STATE, "", ctx.evaluate)
    ctx.set_x0(x0[:3])
    ctx.set_queries(2)
    _upload(ctx, pci)
    assert ctx.Q == 1
    ctx.Q = 2
    _refused(abi.TMX_ERR_STATE, "one query", ctx.set_query_targets, k_goal, goal2)
    ctx.Q = 1
    ctx.set_x0(x0[:3])
    # the trajopt_sqp flavour is refused at set_queries
    pci4, s4, g4 = configs.config4(n_steps=6, with_collision=False)
    ctx.upload(pci4.to_desc(), abi.default_sqp_params(), configs.osqp_settings_config4())
    _refused(abi.TMX_ERR_UNSUPPORTED, "TMX_FLAVOR_SQP", ctx.set_queries, 2)
    ctx.set_queries(1)


# ---- cases 2, 6, 7: glass_upright at a short horizon --------------------------------------------------------------------------

def test_glass_upright_three_queries_against_three_uploads(make_ctx, orc):
    """config 1 at T = 8 (the horizon of test_whole_optimize_of_config1_short_horizon_stepped), three queries of two seeds, with the
    fused evaluation (dbg_flags 0) and the generic one (16); then the first exact evaluation of the multi-query batch against the
    oracle's values for every query's own description (the oracle call and the tolerance of pc.check_evaluate)"""
    pcis, x0s = _config1_queries()
    # (the verdict of the upload; the host build has no device branches and runs the generic evaluation either way)
    ctx = _compare_with_separate_uploads(make_ctx, pcis, x0s, flags=(0, GENERIC_EVAL), want_eval_fast=1)
    ctx.set_x0(np.concatenate(x0s))
    cv, vv = ctx.evaluate()
    differ = 0.0
    for q, pci in enumerate(pcis):
        desc = pci.to_desc()
        for s in range(2):
            ocv, ovv = orc.evaluate(desc, x0s[q][s], x0s[q][s])
            assert cv[2 * q + s].shape == ocv.shape and vv[2 * q + s].shape == ovv.shape
            assert np.abs(cv[2 * q + s] - ocv).max(initial=0.0) <= 1e-12, "cost values differ"
            assert np.abs(vv[2 * q + s] - ovv).max(initial=0.0) <= 1e-12, "constraint violations differ"
            ocv0, ovv0 = orc.evaluate(pcis[0].to_desc(), x0s[q][s], x0s[q][s])
            differ = max(differ, np.abs(ovv - ovv0).max(initial=0.0))
    assert differ > 1e-3   # (the queries' targets matter at these points)


def test_unchanged_targets_give_the_plain_batch(make_ctx):
    """set_queries(3) with no target changed: the bytes of the plain batch"""
    pci, s, g = pc.cfg(1, T=8)
    x0 = configs.seeds_for(1, pci, s, g, 3, sigma=0.05, first=2)
    ctx = make_ctx()
    _upload(ctx, pci)
    ctx.set_x0(x0)
    assert ctx.run(0) == 0
    plain = _snapshot(ctx)
    ctx.set_queries(3)
    ctx.set_x0(x0)
    assert ctx.run(0) == 0
    assert _snapshot(ctx) == plain
    ctx.set_queries(1)
    ctx.set_x0(x0)
    assert ctx.run(0) == 0
    assert _snapshot(ctx) == plain


# ---- cases 3 and 4: the mini arm, and the other launch modes on the device -----------------------------------------------------

def test_mini_arm_two_queries(make_ctx):
    pcis, x0s = _mini_queries()
    _compare_with_separate_uploads(make_ctx, pcis, x0s)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [("TMX_SQP_MODE", "0"), ("TMX_SQP_MODE", "1"), ("TMX_WAVE", "1")],
                         ids=["piecewise_kernels", "fused_in_order_kernel", "wave_pair_solver"])
def test_mini_arm_two_queries_in_other_launch_modes(gpu_ctx_factory, monkeypatch, env):
    """the piecewise kernels (k_convexify / k_evaluate), the fused in-order kernel and the wave-pair solver (it calls the shared term
    functions): the hooks are read at upload, so the multi-query context and the separate ones run the same mode"""
    monkeypatch.setenv(*env)
    made = []

    def make():
        made.append(gpu_ctx_factory())
        return made[-1]
    make.tier = "gpu"
    try:
        pcis, x0s = _mini_queries()
        _compare_with_separate_uploads(make, pcis, x0s)
    finally:
        for c in made:
            c.close()


# ---- case 5: the workspace outside the LDS ---------------------------------------------------------------------------------

HBM_STEPS = 4   # the smallest configs.config3(n) whose QP workspace leaves the LDS (asserted below): 326 656 B; 118 520 B at 3


def _in_hbm(ctx):
    """the rule of the upload: a workspace over the 160 KB of LDS lives in HBM.  (The host build has no such kernels and always says
    in_hbm = 0; it reports the workspace's size.)"""
    ws = ctx.workspace_info()
    return bool(ws["in_hbm"] or ws["lds_bytes"] > 160 * 1024)


def test_hbm_workspace_two_queries(make_ctx):
    """car_seat at the shortest horizon whose workspace is carved in HBM (k_sqp_fused_hbm / k_prepare on the HBM scratch): two queries
    that differ in the goal JointPos constraint, two seeds each"""
    probe = make_ctx()
    _upload(probe, configs.config3(HBM_STEPS - 1)[0])
    assert not _in_hbm(probe)
    pcis, x0s = [], []
    for q in range(2):
        pci, s, g = configs.config3(HBM_STEPS)
        if q == 1:
            g = configs.CFG3_GOAL + np.array([-0.05, 0.05, 0.03, 0.1, -0.05, 0.05, 0.05, -0.05, 0.05, -0.05])
            assert pci.cnt_infos[-1].name == "goal"
            pci.cnt_infos[-1].targets = list(g)
        pcis.append(pci)
        x0s.append(configs.seeds_for(3, pci, s, g, 2, sigma=0.02))
    ctx = _compare_with_separate_uploads(make_ctx, pcis, x0s)
    assert _in_hbm(ctx)
    assert make_ctx.tier == "host" or ctx.workspace_info()["in_hbm"]


# ---- case 8: the best seed of every query -----------------------------------------------------------------------------------

def _numpy_argmin(r, Q, S):
    bi, bc = np.full(Q, -1, np.int64), np.full(Q, 1e300)
    for q in range(Q):
        for b in range(q * S, (q + 1) * S):
            if r["status"][b] == abi.OPT_CONVERGED and r["total_cost"][b] < bc[q]:
                bi[q], bc[q] = b, r["total_cost"][b]
    return bi, bc


@pytest.mark.parametrize("S", [1, 65, 257])
def test_argmin_and_best_trajectory_per_query(make_ctx, S):
    """config 0 at 3 waypoints, four queries of S seeds (S = 1; 65: a wave and one seed; 257: one more than the kernel's block of 256 threads; seeds close to the straight line, which
    converge in a few QPs):
    query 0 and 3 ordinary (3 with another goal), query 1 holds ONE seed S times (equal cost bytes: the lowest index wins), every
    seed of query 2 is taken out of OPT_CONVERGED; against numpy over results()"""
    Q = 4
    pci, s, g = pc.cfg(0, T=3)
    ctx = make_ctx()
    _upload(ctx, pci)
    ctx.set_queries(Q)
    goals = np.stack([g, g, g, g + np.array([0.1, -0.1, 0.1, 0.1, 0.1, 0.1, -0.1])])
    ctx.set_query_targets(pci.term_index(pci.cnt_infos[-1]), goals)
    x0 = configs.seeds_for(0, pci, s, g, Q * S, sigma=0.01)
    x0[S:2 * S] = x0[S]
    ctx.set_x0(x0)
    assert ctx.run(0) == 0
    for b in range(2 * S, 3 * S):
        ctx.stop(b, abi.OPT_FAILED)
    r = ctx.results()
    assert (r["status"][:2 * S] == abi.OPT_CONVERGED).all() and (r["status"][3 * S:] == abi.OPT_CONVERGED).any()
    want_i, want_c = _numpy_argmin(r, Q, S)
    bi, bc = ctx.argmin_queries()
    assert bi.tolist() == want_i.tolist() and bc.tobytes() == want_c.tobytes()
    assert bi[1] == S and bi[2] == -1 and bc[2] == 1e300
    assert len({r["total_cost"][b].tobytes() for b in range(S, 2 * S)}) == 1
    x, found = ctx.best_trajectories()
    assert found.tolist() == [True, True, False, True]
    for q in range(Q):
        assert x[q].tobytes() == (r["x"][bi[q]] if bi[q] >= 0 else np.zeros_like(x[q])).tobytes()
    # tmx_argmin keeps its meaning over the whole batch
    gi, gc = ctx.argmin()
    k = int(np.argmin(want_c))
    assert (gi, gc) == (int(want_i[k]), float(want_c[k]))
    # one query: the local argmin of the batch
    if S == 1:
        ctx.set_queries(1)
        ctx.set_x0(x0)
        assert ctx.run(0) == 0
        r1 = ctx.results()
        w_i, w_c = _numpy_argmin(r1, 1, Q * S)
        b1, c1 = ctx.argmin_queries()
        assert b1.tolist() == w_i.tolist() and c1.tobytes() == w_c.tobytes()
        x1, f1 = ctx.best_trajectories()
        assert f1.tolist() == [True] and x1[0].tobytes() == r1["x"][b1[0]].tobytes()


# ---- the optimizer class above the C-ABI --------------------------------------------------------------------------------

def test_batched_optimizer_takes_a_list_of_queries(make_ctx):
    """BatchedTrustRegionSQP with queries given as (TermInfo, target) pairs: the result bytes of the Context calls, and the best seed of
    every query next to the statuses"""
    pcis, x0s = _mini_queries()
    pci = pcis[0]
    queries = [[], [(pci.cnt_infos[k], _target_of(pcis[1].cnt_infos[k])) for k in (0, -2, -1)]]
    lib = None if make_ctx.tier == "gpu" else make_ctx().lib._name
    opt = runtime.BatchedTrustRegionSQP(pci, lib_path=lib, queries=queries)
    try:
        opt.initialize(np.concatenate(x0s))
        status, best = opt.optimize()
        got = _snapshot(opt.ctx)
        r = opt.results()
    finally:
        opt.ctx.close()
    ctx = make_ctx()
    _upload(ctx, pci)
    _send_targets(ctx, pcis)
    ctx.set_x0(np.concatenate(x0s))
    assert ctx.run(0) == 0
    assert _snapshot(ctx) == got
    assert status.tobytes() == r["status"].tobytes()
    want_i, want_c = _numpy_argmin(r, 2, 2)
    assert best["index"].tolist() == want_i.tolist() and best["total_cost"].tobytes() == want_c.tobytes()
    for q in range(2):
        assert bool(best["found"][q]) == (want_i[q] >= 0)
        if want_i[q] >= 0:
            assert best["x"][q].tobytes() == r["x"][want_i[q]].tobytes()

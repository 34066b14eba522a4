"""Every QP engine under NON-DEFAULT OSQP settings (tmx_osqp_settings is part of the C-ABI; both adapters pass the caller's settings
straight into it): the first cold Model::optimize() of every route against the oracle's OSQP under the SAME settings - integer record,
polish active set row by row, primal solution, KKT certificate (parity_checks.check_first_qp_solve) - the dense fast path against the
generic code of the same library byte for byte, and whole runs by the history classes.  Each engine reads the settings in code of its
own: the burst scheduler of the register-resident loop (next multiple of check_termination / adaptive_rho_interval, max_iter), the
can_check / do_rho sites, the register-resident setup (scaling) and polish (delta, polish_refine_iter), the generic polish loop, the
wave-pair solver, the dense engine.

ROUTES (each the smallest shape that still takes it; every test asserts the upload's verdicts - tmx_debug_setup_fast / _polish_fast /
_step_fast / _wave_ok / _qp_dense / _tt_chain / _tv_chain and tmx_workspace_info - before it compares anything):
  fast      pc.cfg(1, T=6)                         dense fast path (setup, polish and step verdicts 1)
  pairs     pc.cfg(16)                             generic loop with pair rows (the three verdicts 0)
  chain     pc.cfg(13)                             generic block chain (10 joints: no fast polish, no fast step)
  norows    pc.cfg(15)                             no row slot
  dense     pc.cfg(50)                             dense engine (qp_dense)
  rowstime  pc.cfg(53)                             rows-only time problem on the structured solver
  ttchain   pc.cfg(50), TMX_TOTAL_TIME_CHAIN=1     TotalTime term as a rank-one correction of the block chain (tt_chain)
  tvchain   pc.cfg(52), TMX_VEL_TIME_CHAIN=1       squared velocity-with-time cost on the dense-coupling chain (tv_chain)
  hbm       pc.cfg(2, T=65)                        k_qp_solve_hbm: 65 waypoints is the smallest horizon of config 2 whose QP workspace
                                                   the upload places in HBM (64 still fits the LDS; asserted).  CPU tier: the seven rows of
                                                   HBM_CPU_ROWS (test_first_qp_under_settings says why)
  wave      pc.cfg(1, T=3), TMX_WAVE=1             wave-pair solver: 3 waypoints is the smallest horizon of config 1 whose row template fits
                                                   the lane plan (2 does not; asserted); one seed, the five settings of WAVE_ROWS

SETTINGS TABLE.  Thirty settings were candidates (scaling 0 / 1 / 3, polishing 0, polish_refine_iter 0 / 1, adaptive_rho 0,
adaptive_rho_interval 0 / 13 / 25 / 100, check_termination 1 / 7 / 0 (the last with max_iter 33: without a check OSQP runs to max_iter),
max_iter 1 / 10 / 25 / 26 / 33 / 60 / 300, alpha 1.0 / 1.9, rho 1 / 1e-3, sigma 1e-3, eps_abs = eps_rel 1e-8 / 1e-2,
adaptive_rho_tolerance 1.5, delta 1e-4).  A row stays only if, ON THE ORACLE ALONE, it changes the integer record or the bytes of x of
at least one seed of at least one route against the default-settings solve of the same QP (test_every_setting_changes_something_on_the_oracle):
all thirty do - none was dropped.  (On the fast route alone scaling 3 and adaptive_rho_interval 100 give the default's record; they
change other routes.)

TOLERANCES.  x after a successful polish with the default three refinement passes: parity_checks.TOL_TRAJ, the default of
check_first_qp_solve.  Unpolished iterates (polishing 0, a rejected polish, OSQP_MAX_ITER_REACHED) and polish_refine_iter < 3: ten times
max |x_oracle - x_oracle_fma| of the same QP under the same settings (the project's yardstick for two correct builds; taken on the seeds
on which the two oracle builds return the same record), and not less than TOL_TRAJ.

OSQP_MAX_ITER_REACHED.  OSQP stores its current iterate whatever the status (the reference copies solution->x and returns CVX_FAILED,
trajopt_sco/src/osqp_interface.cpp) and so do all engines here: the rows are compared like any unpolished iterate.  (oracle.first_qp used
to return something else on such a stop - the SQP around it shrank the trust box after the failure and solved again, so the returned
x and bounds were those of the LAST QP next to the record of the first; it now stops after the first Model::optimize(). DESIGN.md S3.)

CPU tier: libtmx_simt.so (tests/test_simt_emulation.py) - the device branches on cooperative fibers.  GPU tier: the product library."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import parity_checks as pc
from test_fast_step import _steps
from test_simt_emulation import simt, simt_lib  # noqa: F401  (fixtures)
from test_time_terms import seeds_time
from test_total_time_chain import switch as tt_switch
from test_vel_time_chain import switch as tv_switch
from trajopt_amd import abi, configs, runtime

# ---- the settings ------------------------------------------------------------------------------------------------------------------
TABLE = [
    ("scaling=0", dict(scaling=0)), ("scaling=1", dict(scaling=1)), ("scaling=3", dict(scaling=3)),
    ("polishing=0", dict(polishing=0)),
    ("polish_refine_iter=0", dict(polish_refine_iter=0)), ("polish_refine_iter=1", dict(polish_refine_iter=1)),
    ("adaptive_rho=0", dict(adaptive_rho=0)),
    ("adaptive_rho_interval=0", dict(adaptive_rho_interval=0)), ("adaptive_rho_interval=13", dict(adaptive_rho_interval=13)),
    ("adaptive_rho_interval=25", dict(adaptive_rho_interval=25)), ("adaptive_rho_interval=100", dict(adaptive_rho_interval=100)),
    ("check_termination=1", dict(check_termination=1)), ("check_termination=7", dict(check_termination=7)),
    ("check_termination=0", dict(check_termination=0, max_iter=33)),
    ("max_iter=1", dict(max_iter=1)), ("max_iter=10", dict(max_iter=10)), ("max_iter=25", dict(max_iter=25)), ("max_iter=26", dict(max_iter=26)),
    ("max_iter=33", dict(max_iter=33)), ("max_iter=60", dict(max_iter=60)), ("max_iter=300", dict(max_iter=300)),
    ("alpha=1.0", dict(alpha=1.0)), ("alpha=1.9", dict(alpha=1.9)),
    ("rho=1", dict(rho=1.0)), ("rho=1e-3", dict(rho=1e-3)),
    ("sigma=1e-3", dict(sigma=1e-3)),
    ("eps=1e-8", dict(eps_abs=1e-8, eps_rel=1e-8)), ("eps=1e-2", dict(eps_abs=1e-2, eps_rel=1e-2)),
    ("adaptive_rho_tolerance=1.5", dict(adaptive_rho_tolerance=1.5)),
    ("delta=1e-4", dict(delta=1e-4)),
]
WAVE_ROWS = ("scaling=0", "polish_refine_iter=0", "check_termination=7", "adaptive_rho_interval=13", "max_iter=60")
HBM_CPU_ROWS = WAVE_ROWS + ("polish_refine_iter=1", "delta=1e-4")   # the HBM route on the CPU tier (test_first_qp_under_settings)
MAX_ITER_ROWS = tuple(name for name, _ in TABLE if name.startswith("max_iter="))


def settings(**kw):
    st = abi.default_osqp_settings()
    for k, v in kw.items():
        assert hasattr(st, k)
        setattr(st, k, v)
    return st


# ---- the routes --------------------------------------------------------------------------------------------------------------------
def _seeds(cid, pci, s, g, B):
    if pci.basic_info.use_time:
        return seeds_time(cid, pci, s, g, B)
    return configs.seeds_for(cid, pci, s, g, B, sigma=0.05) if cid == 1 else configs.seeds_for(cid, pci, s, g, B)


@contextlib.contextmanager
def _wave_switch(value):
    old = os.environ.pop("TMX_WAVE", None)
    os.environ["TMX_WAVE"] = value
    try:
        yield
    finally:
        os.environ.pop("TMX_WAVE", None)
        if old is not None:
            os.environ["TMX_WAVE"] = old


# name -> (config id, horizon, seeds, environment switch of the upload, expected verdicts)
# verdicts: (setup_fast, polish_fast, step_fast, wave_ok, qp_dense, tt_chain, tv_chain, workspace in HBM)
ROUTES = {
    "fast": (1, 6, 2, None, (1, 1, 1, 0, 0, 0, 0, 0)),
    "pairs": (16, None, 2, None, (0, 0, 0, 0, 0, 0, 0, 0)),
    "chain": (13, None, 2, None, (1, 0, 0, 0, 0, 0, 0, 0)),
    "norows": (15, None, 2, None, (1, 1, 0, 0, 0, 0, 0, 0)),
    "dense": (50, None, 2, None, (0, 0, 0, 0, 1, 0, 0, 0)),
    "rowstime": (53, None, 2, None, (0, 0, 0, 0, 0, 0, 0, 0)),
    "ttchain": (50, None, 2, lambda: tt_switch("1"), (0, 0, 0, 0, 0, 1, 0, 0)),
    "tvchain": (52, None, 2, lambda: tv_switch("1"), (1, 0, 0, 0, 0, 0, 1, 0)),
    "hbm": (2, 65, 2, None, (1, 0, 0, 0, 0, 0, 0, 1)),
    "wave": (1, 3, 1, lambda: _wave_switch("1"), (1, 1, 1, 1, 0, 0, 0, 0)),
}
FULL_TABLE_ROUTES = [r for r in ROUTES if r != "wave"]


def _verdicts(ctx):
    out = []
    for name in ("setup_fast", "polish_fast", "step_fast", "wave_ok", "qp_dense", "tt_chain", "tv_chain"):
        fn = getattr(ctx.lib, "tmx_debug_" + name)
        fn.argtypes, fn.restype = [C.c_void_p], C.c_int
        out.append(fn(ctx.h))
    return tuple(out) + (1 if ctx.workspace_in_hbm() else 0,)


def _problem(route):
    cid, T, B, _, _ = ROUTES[route]
    pci, s, g = pc.cfg(cid, T)
    return pci, _seeds(cid, pci, s, g, B)


def _rows(route):
    return [(n, kw) for n, kw in TABLE if route != "wave" or n in WAVE_ROWS]


_ORACLE = {}   # (oracle build, route, settings row) -> the oracle's first QPs of the route's seeds; filled once, never changed


def _oracle_first_qps(orc, route, name):
    """oracle.first_qp of every seed of `route` under the row `name` of TABLE ("default": the default settings)"""
    key = (orc.lib()._name, route, name)
    if key not in _ORACLE:
        pci, x0 = _problem(route)
        desc = pci.to_desc()
        st = settings(**({} if name == "default" else dict(TABLE)[name]))
        _ORACLE[key] = [orc.first_qp(desc, x0[b], osqp=st) for b in range(x0.shape[0])]
    return _ORACLE[key]


def _ints(rec):
    return (rec.osqp_status, rec.osqp_iter, rec.rho_updates, rec.polish_status)


def _check_route(make_ctx, orc, orc_fma, route, only=None):
    """the route's problem under every row of its table (`only`: a subset of it): verdicts, then check_first_qp_solve in its strict form
    under the row's settings"""
    cid, T, B, switch, expect = ROUTES[route]
    pci, x0 = _problem(route)
    worst = {"polished": 0.0, "refine<3": 0.0, "unpolished": 0.0, "yardstick": 0.0}
    with (switch() if switch else contextlib.nullcontext()):
        if route in ("hbm", "wave"):  # ... at the SMALLEST horizon that takes the route: one waypoint less does not
            ctx = make_ctx()
            pl, sl, gl = pc.cfg(cid, T - 1)
            pc.make_ctx_inputs(ctx, pl, _seeds(cid, pl, sl, gl, 1))
            assert _verdicts(ctx)[3 if route == "wave" else 7] == 0
            ctx.close()
        for name, kw in _rows(route):
            if only is not None and name not in only:
                continue
            st = settings(**kw)
            ctx = make_ctx()
            try:
                desc = pc.make_ctx_inputs(ctx, pci, x0, osqp=st)
                assert _verdicts(ctx) == expect, (route, name, _verdicts(ctx))
                oq = _oracle_first_qps(orc, route, name)
                loose = st.polish_refine_iter < 3 or any(q["rec"].polish_status != 1 for q in oq)
                x_tol = pc.TOL_TRAJ
                if loose:
                    fq = _oracle_first_qps(orc_fma, route, name)
                    yard = max([float(np.abs(a["x"] - f["x"]).max()) for a, f in zip(oq, fq) if _ints(a["rec"]) == _ints(f["rec"])], default=0.0)
                    worst["yardstick"] = max(worst["yardstick"], yard)
                    x_tol = max(pc.TOL_TRAJ, 10.0 * yard)
                try:
                    res = pc.check_first_qp_solve(ctx, orc, desc, x0, x_tol=x_tol, osqp=st)
                except AssertionError as e:
                    raise AssertionError(f"route {route} under {name}: {e}") from e
                assert all(same for same, _ in res), (route, name, res)
                for (_, dx), q in zip(res, oq):
                    kind = "polished" if q["rec"].polish_status == 1 and st.polish_refine_iter >= 3 else ("refine<3" if q["rec"].polish_status == 1 else "unpolished")
                    worst[kind] = max(worst[kind], float(dx))
            finally:
                ctx.close()
    print(f"route {route}: worst |x - x_oracle| " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


# ---- the table on the oracle alone -------------------------------------------------------------------------------------------------
def test_every_setting_changes_something_on_the_oracle(orc):
    """A row that changes nothing tests nothing: every row of TABLE changes the integer record or the bytes of x of at least one seed of
    at least one route against the default-settings solve of the same QP, and the outcomes the rows aim at occur: OSQP_MAX_ITER_REACHED
    under every max_iter row, polish_status 0 with polishing = 0, a rejected polish (-1) with polish_refine_iter = 0, more than two rho
    updates with adaptive_rho_tolerance = 1.5"""
    base = {r: _oracle_first_qps(orc, r, "default") for r in FULL_TABLE_ROUTES}
    seen = {}
    for name, _ in TABLE:
        changed, recs = [], []
        for r in FULL_TABLE_ROUTES:
            for q, d in zip(_oracle_first_qps(orc, r, name), base[r]):
                recs.append(_ints(q["rec"]))
                if _ints(q["rec"]) != _ints(d["rec"]) or q["x"].tobytes() != d["x"].tobytes():
                    changed.append(r)
        assert changed, f"{name} changes nothing on the oracle: drop the row"
        seen[name] = recs
    for name in MAX_ITER_ROWS + ("check_termination=0",):
        assert any(r[0] == abi.OSQP_MAX_ITER_REACHED for r in seen[name]), name
    assert all(r[3] == 0 for r in seen["polishing=0"])
    assert any(r[3] == -1 for r in seen["polish_refine_iter=0"])
    assert any(r[2] > 2 for r in seen["adaptive_rho_tolerance=1.5"])
    # the wave-pair route's subset on its own problem
    d = _oracle_first_qps(orc, "wave", "default")
    for name in WAVE_ROWS:
        q = _oracle_first_qps(orc, "wave", name)
        assert _ints(q[0]["rec"]) != _ints(d[0]["rec"]) or q[0]["x"].tobytes() != d[0]["x"].tobytes(), name


def test_oracle_first_qp_is_the_first_qp_when_osqp_fails(orc):
    """oracle.first_qp under max_iter = 10: record, bounds and iterate are those of ONE QP - solving the returned QP again gives the returned
    x bit for bit (the SQP around it used to shrink the trust box after OSQP_MAX_ITER_REACHED and solve again)"""
    st = settings(max_iter=10)
    for q in _oracle_first_qps(orc, "fast", "max_iter=10"):
        assert q["rec"].osqp_status == abi.OSQP_MAX_ITER_REACHED and q["rec"].osqp_iter == 10
        o = orc.qp_solve(q, osqp=st)
        assert (o["status"], o["iters"]) == (abi.OSQP_MAX_ITER_REACHED, 10)
        assert o["x"].tobytes() == q["x"].tobytes()


# ---- first QP of every route, CPU tier ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_first_qp_under_settings(simt_lib, orc, orc_fma, route):
    """Measured on the emulation, worst over the table and both seeds: |x - x_oracle| at most 1.3e-11 after a three-pass polish (the HBM
    route under delta = 1e-4; 3.3e-16 elsewhere), 9.1e-8 with fewer passes (the HBM route, where the two oracle builds are 4.7e-8 apart; 1.6e-10 elsewhere),
    2.9e-9 unpolished (the velocity-with-time chain; 8.1e-11 elsewhere); the yardstick |x_oracle - x_oracle_fma| on the same QPs at most
    4.7e-8 - ten times that stays below TOL_TRAJ, which is what binds.  Per route: DESIGN.md S3.
    The HBM route costs the emulation eleven minutes for the whole table (1 235 variables on 512 fibers; the plain host build places this
    horizon in its LDS stand-in, so it cannot take the route): the CPU tier runs the seven rows of HBM_CPU_ROWS on it - the five of the
    wave-pair route plus the two with the largest deviations on this route, polish_refine_iter = 1 (9.1e-8, through the regularised
    passes of the HBM kernels' polish) and delta = 1e-4 (1.3e-11) - and the GPU tier runs the whole table on the device."""
    _check_route(lambda: runtime.Context(0, simt_lib), orc, orc_fma, route, only=HBM_CPU_ROWS if route == "hbm" else None)


# ---- the dense fast path against the generic code of the same library ---------------------------------------------------------------
FAST_VS_GENERIC = [dict(scaling=0), dict(polish_refine_iter=0), dict(check_termination=7, adaptive_rho_interval=13), dict(max_iter=60)]
GENERIC_ALL = 14  # DevProblem::dbg_flags bits 1 - 3: generic QP setup, generic polish, generic SQP shell


def _fast_against_generic(ctx, kw):
    """whole optimize() of pc.cfg(1, T=6), stepped with run(1), with dbg_flags 0 and 14: results, state, step log after every step and the
    record integers byte for byte (tests/test_fast_step.py)"""
    pci, x0 = _problem("fast")
    pc.make_ctx_inputs(ctx, pci, x0, osqp=settings(**kw))
    assert _verdicts(ctx) == ROUTES["fast"][4]
    a = _steps(ctx, x0, 0, 0)
    b = _steps(ctx, x0, GENERIC_ALL, 0)
    assert all(len(per) >= 1 for per in a[1]) and len(a[0]) >= 1
    assert a[1] == b[1]
    assert a[0] == b[0]


@pytest.mark.parametrize("kw", FAST_VS_GENERIC, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_fast_path_against_generic_code_under_settings(simt, kw):
    _fast_against_generic(simt, kw)


# ---- whole runs ---------------------------------------------------------------------------------------------------------------------
WHOLE_RUNS = [dict(warm_starting=0), dict(adaptive_rho=0), dict(check_termination=7, adaptive_rho_interval=13)]


def _whole_runs(make_ctx, orc, orc_fma, cid, T, kw):
    """QP by QP against the oracle's run under the same settings (parity_checks.sqp_history_classes); a seed that parts at an ADMM-level
    integer is judged as elsewhere: by what the oracle shows against its own FMA build on these seeds (oracle_self_classes) and
    drift_budget.  With two seeds that budget is one: what is ASSERTED is no "other" / "csc-noise" seed, at most one seed parting at an
    ADMM integer or drifting (plus what the oracle does against itself), and TOL_TRAJ on every identical / tie seed - less than the
    "all identical" that was measured on both tiers"""
    st = settings(**kw)
    pci, s, g = pc.cfg(cid, T)
    x0 = _seeds(cid, pci, s, g, 2)
    ctx = make_ctx()
    try:
        desc = pc.make_ctx_inputs(ctx, pci, x0, osqp=st)
        trace = []
        classes, dx, res = pc.sqp_history_classes(ctx, orc, desc, x0, trace=trace, osqp=st)
    finally:
        ctx.close()
    own = pc.oracle_self_classes(orc, orc_fma, desc, x0, osqp=st)
    print(f"config {cid} under {kw}: classes {classes}, |dx| {np.round(dx, 9)}, the oracle against its FMA build {own}")
    assert "other" not in classes and "csc-noise" not in classes, trace
    assert classes.count("drift") <= pc.drift_budget(len(classes), own), trace
    assert classes.count("admm") + classes.count("drift") <= sum(c != "identical" for c in own) + pc.drift_budget(len(classes)), (classes, own, trace)
    for b, c in enumerate(classes):
        if c in ("identical", "tie"):
            assert dx[b] <= pc.TOL_TRAJ, (b, c, dx[b])


@pytest.mark.parametrize("kw", WHOLE_RUNS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
@pytest.mark.parametrize("cid,T", [(1, 8), (16, None)])
def test_whole_runs_under_settings(simt_lib, orc, orc_fma, cid, T, kw):
    _whole_runs(lambda: runtime.Context(0, simt_lib), orc, orc_fma, cid, T, kw)


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_gpu_first_qp_under_settings(gpu_ctx_factory, orc, orc_fma, route):
    _check_route(gpu_ctx_factory, orc, orc_fma, route)


@pytest.mark.gpu
def test_gpu_fast_path_against_generic_code_under_settings(gpu_ctx_factory):
    for kw in FAST_VS_GENERIC:
        ctx = gpu_ctx_factory()
        try:
            _fast_against_generic(ctx, kw)
        finally:
            ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid,T", [(1, 8), (16, None)])
def test_gpu_whole_runs_under_settings(gpu_ctx_factory, orc, orc_fma, cid, T):
    for kw in WHOLE_RUNS:
        _whole_runs(gpu_ctx_factory, orc, orc_fma, cid, T, kw)

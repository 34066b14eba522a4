"""tmx_qp_solve_batched — the sco::Model / trajopt_sqp::QPSolver boundary for QPs handed over in CSC form (SURVEY.md §8b S1,
S5).  CPU tier: the kernel sources on the host against the oracle's OSQP restatement and a numpy KKT certificate; GPU tier:
the HIP library on the same QPs."""
import numpy as np
import pytest

import parity_checks as pc
from test_simt_emulation import simt, simt_lib  # noqa: F401  (fixtures)
from trajopt_amd import abi, configs, runtime


def _random_qp(rng, n, m, infeasible=False):
    """strictly convex random QP with box + general rows, a few equalities and infinite bounds, in OSQP's CSC form"""
    import scipy.sparse as sp
    M = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.4)
    P = M @ M.T + 0.1 * np.eye(n)
    Pu = sp.csc_matrix(np.triu(P))
    G = rng.standard_normal((m - n, n)) * (rng.random((m - n, n)) < 0.5)
    A = sp.csc_matrix(np.vstack([G, np.eye(n)]))
    x_feas = rng.standard_normal(n)
    mid = A @ x_feas
    l, u = mid - rng.uniform(0.1, 2.0, m), mid + rng.uniform(0.1, 2.0, m)
    eq = rng.random(m) < 0.15
    eq[m - n:] = False
    l[eq] = u[eq] = mid[eq]
    l[rng.random(m) < 0.2] = -1e30
    u[rng.random(m) < 0.2] = 1e30
    if infeasible:   # two contradicting rows
        A = sp.vstack([A, sp.csc_matrix(np.eye(n)[:1])]).tocsc()
        l, u = np.append(l, u[m - n] + 5.0), np.append(u, u[m - n] + 6.0)
    A.sort_indices()
    Pu.sort_indices()
    return dict(n=n, m=A.shape[0], P_p=Pu.indptr.astype(np.int64), P_i=Pu.indices.astype(np.int64), P_x=Pu.data.copy(),
                q=rng.standard_normal(n), A_p=A.indptr.astype(np.int64), A_i=A.indices.astype(np.int64), A_x=A.data.copy(), l=l, u=u)


def _check_batch(ctx, orc, qps, x_tol=1e-6):
    res = ctx.qp_solve_batched(qps)
    n_same = 0
    for q, r in zip(qps, res):
        o = orc.qp_solve(q, warm_x=q.get("x_warm"), warm_y=q.get("y_warm"))
        assert r["info"].osqp_status == o["status"], (r["info"].osqp_status, o["status"])
        if o["status"] in (3, 4, 5, 6):
            assert r["cvx_status"] == abi.CVX_INFEASIBLE and np.isnan(r["x"]).all()
            continue
        assert r["cvx_status"] == abi.CVX_SOLVED
        same = (r["info"].iter, r["info"].rho_updates, r["info"].polish_status) == (o["iters"], o["rho_updates"], o["polish_status"])
        n_same += same
        if same and np.array_equal(r["active"], o["active"]):
            assert np.abs(r["x"] - o["x"]).max() <= x_tol
        if r["info"].polish_status == 1:
            st, pr, su = pc.kkt_certificate(q, r["x"], r["y"])
            assert st <= 1e-8 and pr <= pc.KKT_PRIM_TOL and su <= pc.KKT_PRIM_TOL, (st, pr, su)
        # both are minimisers of the same strictly convex QP to OSQP's tolerance
        assert np.abs(r["x"] - o["x"]).max() <= 1e-3
    return n_same, len(qps)


def _qps(seed, count=12):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(rng.integers(2, 24))
        out.append(_random_qp(rng, n, n + int(rng.integers(1, 20)), infeasible=(k % 6 == 5)))
    return out


def test_generic_qp_matches_oracle_on_host_build(hostemu_lib, orc):
    ctx = runtime.Context(0, hostemu_lib)
    same, tot = _check_batch(ctx, orc, _qps(3))
    assert same >= tot - 4        # identical ADMM history for (nearly) all: different linear algebra, same algorithm
    ctx.close()


def test_generic_qp_warm_start_and_trajectory_qp(hostemu_lib, orc):
    """(i) osqp_warm_start through the boundary; (ii) a real trajectory QP (config 0's first QP, exported by the device path
    in reference layout) solved through the generic entry gives the term-structured solver's answer"""
    ctx = runtime.Context(0, hostemu_lib)
    q = _qps(5, 1)[0]
    first = ctx.qp_solve_batched([q])[0]
    q2 = dict(q, x_warm=first["x"], y_warm=first["y"])
    r2 = ctx.qp_solve_batched([q2])[0]
    o2 = orc.qp_solve(q, warm_x=first["x"], warm_y=first["y"])
    assert r2["info"].iter == o2["iters"] <= first["info"].iter and np.abs(r2["x"] - first["x"]).max() < 1e-6
    pci, s, g = configs.config0()
    x0 = configs.seeds_for(0, pci, s, g, 1)
    pc.make_ctx_inputs(ctx, pci, x0)
    ctx.convexify()
    xq, cvx, rec = ctx.qp_solve()
    e = ctx.export_csc(0)
    r = ctx.qp_solve_batched([e])[0]
    assert r["cvx_status"] == abi.CVX_SOLVED and r["info"].iter == rec[0].osqp_iter
    assert np.abs(r["x"] - xq[0, :e["n"]]).max() < 1e-9
    ctx.close()


def test_generic_qp_rejects_malformed_input(hostemu_lib):
    ctx = runtime.Context(0, hostemu_lib)
    q = _qps(7, 1)[0]
    bad = dict(q, l=q["u"] + 1.0)
    with pytest.raises(runtime.TmxError, match="lower bound above upper bound"):
        ctx.qp_solve_batched([bad])
    bad = dict(q, A_i=q["A_i"] + 1000)
    with pytest.raises(runtime.TmxError, match="row index out of range"):
        ctx.qp_solve_batched([bad])
    # what osqp_setup's validate_data rejects as well: column pointers that do not start at 0 / decrease / overrun nnz (the
    # kernel walks them over device memory), a P given with its lower triangle (it would be counted twice), NaN bounds
    Pp = q["P_p"].copy()
    Pp[0] = 1
    with pytest.raises(runtime.TmxError, match="must start at 0"):
        ctx.qp_solve_batched([dict(q, P_p=Pp)])
    Ap = q["A_p"].copy()
    Ap[1], Ap[2] = Ap[2] + 1, Ap[1]
    with pytest.raises(runtime.TmxError, match="non-decreasing"):
        ctx.qp_solve_batched([dict(q, A_p=Ap)])
    Ap = q["A_p"].copy()
    Ap[3] = Ap[-1] + 5
    with pytest.raises(runtime.TmxError, match="non-decreasing and end at nnz"):
        ctx.qp_solve_batched([dict(q, A_p=Ap)])
    import scipy.sparse as sp
    n = q["n"]
    Pu = sp.csc_matrix((q["P_x"], q["P_i"], q["P_p"]), shape=(n, n))
    Pfull = sp.csc_matrix(Pu + sp.triu(Pu, 1).T)
    Pfull.sort_indices()
    if Pfull.nnz > Pu.nnz:
        with pytest.raises(runtime.TmxError, match="upper triangle"):
            ctx.qp_solve_batched([dict(q, P_p=Pfull.indptr.astype(np.int64), P_i=Pfull.indices.astype(np.int64), P_x=Pfull.data)])
    lnan = q["l"].copy()
    lnan[0] = np.nan
    with pytest.raises(runtime.TmxError, match="NaN bound"):
        ctx.qp_solve_batched([dict(q, l=lnan)])
    ctx.close()


def test_entry_points_refuse_while_a_launch_is_pending(hostemu_lib):
    """tmx_sqp_launch / tmx_sqp_wait: until the launch is collected, everything that would re-prepare, reallocate or read the
    batch returns TMX_ERR_STATE"""
    ctx = runtime.Context(0, hostemu_lib)
    pci, s, g = configs.config0()
    x0 = configs.seeds_for(0, pci, s, g, 2)
    pc.make_ctx_inputs(ctx, pci, x0)
    ctx.launch()
    for call in (lambda: ctx.set_x0(x0), ctx.results, ctx.evaluate, ctx.convexify, lambda: ctx.argmin(0), ctx.launch,
                 lambda: ctx.upload(pci.to_desc(), abi.default_sqp_params(), abi.default_osqp_settings()),
                 lambda: ctx.qp_solve_batched(_qps(7, 1))):
        with pytest.raises(runtime.TmxError):
            call()
    assert ctx.wait() == 0
    r = ctx.results()
    assert (r["status"] == abi.OPT_CONVERGED).all()
    ctx.close()


# ---- edge QPs and non-default settings ---------------------------------------------------------------------------------------------
def _csc(n, P, q, A, l, u):
    """dense P (its upper triangle is kept), A -> the CSC dict of tmx_qp_solve_batched; zeros of P / A are not stored"""
    import scipy.sparse as sp
    Pu = sp.csc_matrix(np.triu(np.asarray(P, dtype=np.float64).reshape(n, n)))
    A = sp.csc_matrix(np.asarray(A, dtype=np.float64).reshape(-1, n))
    Pu.sort_indices()
    A.sort_indices()
    return dict(n=n, m=A.shape[0], P_p=Pu.indptr.astype(np.int64), P_i=Pu.indices.astype(np.int64), P_x=Pu.data.astype(np.float64),
                q=np.asarray(q, dtype=np.float64), A_p=A.indptr.astype(np.int64), A_i=A.indices.astype(np.int64), A_x=A.data.astype(np.float64),
                l=np.asarray(l, dtype=np.float64), u=np.asarray(u, dtype=np.float64))


def _settings(**kw):
    st = abi.default_osqp_settings()
    for k, v in kw.items():
        assert hasattr(st, k)
        setattr(st, k, v)
    return st


INF = 1e30
EDGE_SETTINGS = [dict(scaling=0), dict(scaling=1), dict(polishing=0), dict(polish_refine_iter=0), dict(polish_refine_iter=1), dict(adaptive_rho=0),
                 dict(adaptive_rho_interval=13), dict(check_termination=7), dict(check_termination=0, max_iter=33), dict(alpha=1.0), dict(rho=1e-3),
                 dict(eps_abs=1e-8, eps_rel=1e-8)]


def _edge_cases():
    """(name, QP, settings or None, OSQP status the case aims at or None).  What the random QPs above never have: n = 1, no row at all, P = 0, a
    zero row of A, q = 0, duplicate rows, equalities only, free rows only, sizes around the 256 threads of the kernel, fewer rows than
    variables, the infeasibility verdicts (3: primal, 5: dual, 6: dual, inaccurate - found at max_iter) and OSQP_MAX_ITER_REACHED (7)"""
    rng = np.random.default_rng(17)
    M = rng.standard_normal((6, 6))
    P6, q6 = M @ M.T + 0.1 * np.eye(6), rng.standard_normal(6)
    G = rng.standard_normal((4, 6))
    mid = G @ rng.standard_normal(6)
    cases = [
        ("n=1", _csc(1, [[2.0]], [-1.0], [[1.0]], [-0.25], [0.25]), None, 1),
        ("m=0", _csc(3, np.diag([1.0, 2.0, 3.0]), [1.0, -1.0, 0.5], np.zeros((0, 3)), [], []), None, 1),
        ("P=0", _csc(3, np.zeros((3, 3)), [1.0, -2.0, 0.5], np.vstack([np.eye(3), [[1.0, 1.0, 1.0]]]), [-1, -1, -1, -0.5], [1, 1, 1, 0.5]), None, 1),
        ("zero row", _csc(6, P6, q6, np.vstack([G, np.zeros((1, 6)), np.eye(6)]), np.r_[mid - 1, -1.0, -np.ones(6) * 3], np.r_[mid + 1, 1.0, np.ones(6) * 3]), None, 1),
        ("q=0", _csc(6, P6, np.zeros(6), np.vstack([G, np.eye(6)]), np.r_[mid - 1, -np.ones(6) * 3], np.r_[mid + 1, np.ones(6) * 3]), None, 1),
        ("duplicate rows", _csc(6, P6, q6, np.vstack([G, G[:2], np.eye(6)]), np.r_[mid - 1, mid[:2] - 1, -np.ones(6) * 3], np.r_[mid + 1, mid[:2] + 1, np.ones(6) * 3]), None, 1),
        ("all equality", _csc(6, P6, q6, G, mid, mid), None, 1),
        ("all free", _csc(6, P6, q6, np.vstack([G, np.eye(6)]), -INF * np.ones(10), INF * np.ones(10)), None, 1),
        ("m<n", _csc(6, P6, q6, G[:2], mid[:2] - 0.1, mid[:2] + 0.1), None, 1),
        ("dual infeasible LP", _csc(2, np.zeros((2, 2)), [-1.0, 0.5], np.eye(2), [0.0, 0.0], [INF, 1.0]), None, 5),
        ("dual infeasible QP", _csc(2, [[1.0, 0.0], [0.0, 0.0]], [0.3, -1.0], np.eye(2), [-1.0, 0.0], [1.0, INF]), None, 5),
        ("primal infeasible QP", _csc(2, np.eye(2), [1.0, 1.0], [[1.0, 1.0], [1.0, 1.0], [1.0, 0.0]], [1.0, -INF, -5.0], [INF, 0.0, 5.0]), None, 3),
        ("max_iter", _random_qp(np.random.default_rng(23), 9, 15), dict(max_iter=10), 7),
    ]
    for n in (255, 256, 257):
        cases.append((f"n={n}", _random_qp(np.random.default_rng(n), n, n + 5), None, 1))
    r2 = np.random.default_rng(29)
    for k, kw in enumerate(EDGE_SETTINGS):
        n = int(r2.integers(5, 20))
        cases.append((f"settings {kw}", _random_qp(r2, n, n + int(r2.integers(1, 12))), kw, 7 if "max_iter" in kw else 1))
    return cases


# the dual-infeasible LP stopped at max_iter before the certificate holds to eps_dual_inf, but within ten times it: OSQP_DUAL_INFEASIBLE_INACCURATE
INACCURATE = ("dual infeasible LP", dict(max_iter=23, check_termination=0))   # (status 6 for max_iter 21 .. 25, 5 from 26 on, 7 below)


def _check_edge_cases(ctx, orc):
    cases = _edge_cases()
    lp = dict((c[0], c[1]) for c in cases)[INACCURATE[0]]
    cases.append(("dual infeasible, inaccurate", lp, INACCURATE[1], 6))
    for name, q, kw, aim in cases:
        st = _settings(**kw) if kw else None
        o = orc.qp_solve(q, osqp=st)
        assert aim is None or o["status"] == aim, f"{name}: the oracle ends with status {o['status']}, the case aims at {aim}"
        r = ctx.qp_solve_batched([q], st)[0]
        i = r["info"]
        assert (i.osqp_status, i.iter, i.rho_updates, i.polish_status) == (o["status"], o["iters"], o["rho_updates"], o["polish_status"]), name
        if o["status"] in (3, 4, 5, 6):
            assert r["cvx_status"] == abi.CVX_INFEASIBLE and np.isnan(r["x"]).all(), name
            continue
        assert r["cvx_status"] == (abi.CVX_SOLVED if o["status"] in (1, 2) else abi.CVX_FAILED), name
        assert np.array_equal(r["active"], o["active"]), name
        assert np.abs(r["x"] - o["x"]).max(initial=0.0) <= 1e-6, (name, np.abs(r["x"] - o["x"]).max())   # (x_tol of _check_batch; measured 7e-15)
        if o["status"] not in (1, 2):
            continue
        # every solved case carries a KKT certificate (numpy, from the CSC arrays)
        s_eff = st if st is not None else abi.default_osqp_settings()
        sta, pr, su = pc.kkt_certificate(q, r["x"], r["y"])
        P, A = pc.csc_dense_ops(q)
        ax = A @ r["x"]
        if i.polish_status == 1 and s_eff.polish_refine_iter >= 3:
            # a polish with the default three passes: stationary to round-off, feasible / tight to what OSQP promises
            stat_tol, prim_tol = 1e-8, max(pc.KKT_PRIM_TOL, s_eff.eps_abs)
        elif i.polish_status == 1:
            # fewer passes leave the delta terms of the regularised polish system in the residuals, scaled by Ruiz factors no caller sees
            # (parity_checks.check_first_qp_solve): twice the residuals of the oracle's own polished point on top of the tolerances
            so, po, suo = pc.kkt_certificate(q, o["x"], o["y"])
            stat_tol, prim_tol = 1e-8 + 2.0 * so, max(pc.KKT_PRIM_TOL, s_eff.eps_abs) + 2.0 * max(po, suo)
        else:
            # an unpolished iterate that OSQP called solved passed its termination test (unscaled residuals, scaled_termination = 0):
            # |Ax - z| < eps_abs + eps_rel max(|Ax|, |z|) with z inside the bounds (so Ax is that close to the box, and to the bound of every
            # row with a multiplier: y_i != 0 only where z_i was clipped) and |Px + q + A'y| < eps_abs + eps_rel max(|Px|, |A'y|, |q|)
            factor = 10.0 if o["status"] == 2 else 1.0
            nrm = lambda v: float(np.abs(v).max(initial=0.0))
            prim_tol = factor * (s_eff.eps_abs + s_eff.eps_rel * max(nrm(ax), nrm(np.clip(ax, q["l"], q["u"]))))
            scale = max(1.0, nrm(q["q"]), nrm(r["y"]))   # kkt_certificate reports the stationarity residual over this scale
            stat_tol = factor * (s_eff.eps_abs + s_eff.eps_rel * max(nrm(P @ r["x"]), nrm(A.T @ r["y"]), nrm(q["q"]))) / scale
        assert sta <= stat_tol and pr <= prim_tol and su <= prim_tol, (name, sta, pr, su, stat_tol, prim_tol)


def test_edge_qps_and_settings_on_host_build(hostemu_lib, orc):
    ctx = runtime.Context(0, hostemu_lib)
    _check_edge_cases(ctx, orc)
    ctx.close()


def test_edge_qps_and_settings_on_the_simt_emulation(simt, orc):
    _check_edge_cases(simt, orc)


@pytest.mark.gpu
def test_edge_qps_and_settings_on_device(gpu_ctx_factory, orc):
    ctx = gpu_ctx_factory()
    _check_edge_cases(ctx, orc)
    ctx.close()


@pytest.mark.gpu
def test_generic_qp_matches_oracle_on_device(gpu_ctx_factory, orc):
    ctx = gpu_ctx_factory()
    same, tot = _check_batch(ctx, orc, _qps(3) + _qps(11, 20))
    assert same >= tot - 8
    pci, s, g = configs.config1()
    x0 = configs.seeds_for(1, pci, s, g, 1)
    pc.make_ctx_inputs(ctx, pci, x0)
    ctx.convexify()
    xq, cvx, rec = ctx.qp_solve()
    e = ctx.export_csc(0)                     # n = 572, m = 876: the glass_upright trajectory QP through the dense generic path
    r = ctx.qp_solve_batched([e])[0]
    assert r["cvx_status"] == abi.CVX_SOLVED and np.abs(r["x"] - xq[0, :e["n"]]).max() < 1e-5
    ctx.close()


def _small_problems(orc, ctx):
    """trajopt_sco/test/small-problems-unit.cpp:48-172 on the restated sco SQP; with a context every Model::optimize() is
    solved by tmx_qp_solve_batched (the S1 boundary: host callbacks convexify, the device solves the QP)"""
    import ctypes as C
    FN = C.CFUNCTYPE(C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.POINTER(C.c_double),
                     C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                     C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                     C.POINTER(C.c_double), C.c_void_p)
    calls = []

    def backend(n, m, Pp, Pi, Px, q, Ap, Ai, Ax, l, u, xw, yw, rho, x, y, rho_final, user):
        a = lambda p, k, dt: (np.ctypeslib.as_array(p, shape=(k,)).astype(dt) if k > 0 else np.zeros(0, dt))
        nzP, nzA = int(Pp[n]), int(Ap[n])
        qp = dict(n=n, m=m, P_p=a(Pp, n + 1, np.int64), P_i=a(Pi, nzP, np.int64), P_x=a(Px, nzP, np.float64), q=a(q, n, np.float64),
                  A_p=a(Ap, n + 1, np.int64), A_i=a(Ai, nzA, np.int64), A_x=a(Ax, nzA, np.float64), l=a(l, m, np.float64), u=a(u, m, np.float64))
        if bool(xw):
            qp["x_warm"], qp["y_warm"] = a(xw, n, np.float64), a(yw, m, np.float64)
        st = abi.default_osqp_settings()
        st.rho = rho
        r = ctx.qp_solve_batched([qp], st)[0]
        for j in range(n):
            x[j] = r["x"][j]
        for i in range(m):
            y[i] = r["y"][i]
        rho_final[0] = r["info"].rho_final
        calls.append(r["info"].osqp_status)
        return r["info"].osqp_status

    cb = FN(backend)
    x = np.zeros((6, 3))
    status, nqp = np.zeros(6, np.int32), np.zeros(6, np.int32)
    fn = orc.lib().orc_small_problems
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    total = fn(C.cast(cb, C.c_void_p) if ctx is not None else None, None, x.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p),
               nqp.ctypes.data_as(C.c_void_p))
    assert total > 0 and (ctx is None or len(calls) == total)
    return x, status, nqp


SMALL_EXPECT = [((0, 1, 2), 1e-3), ((1, 7, 2), 1e-2), ((1, 1), 1e-2), ((0, 0), 1e-2), ((1, 1), 1e-2), ((0, float(np.float32(3) ** 0.5)), 1e-2)]


def _check_small(x, status):
    for k, (sol, tol) in enumerate(SMALL_EXPECT):
        assert status[k] == abi.OPT_CONVERGED, (k, status[k])
        assert np.abs(x[k, :len(sol)] - np.array(sol)).max() < tol, (k, x[k])


def test_small_problems_unit_with_the_generic_qp_backend_on_host_build(hostemu_lib, orc):
    xo, so, no = _small_problems(orc, None)           # restated OSQP: the KAT itself
    _check_small(xo, so)
    ctx = runtime.Context(0, hostemu_lib)
    xd, sd, nd = _small_problems(orc, ctx)            # every QP through tmx_qp_solve_batched
    _check_small(xd, sd)
    # problem 3 passes through ONE Model::optimize() whose polish fails after four rho updates (n = 3, m = 4, 225 iterations in both
    # arithmetics): its unpolished ADMM iterate is the same to 3.3e-4 only, with or without the refinement step of the dense engine
    # (measured, round 6: TMX_DENSE_REFINE=0 / 1 give 3.34e-4 / 3.25e-4 on that QP and 4e-12 / 1.7e-5 at the end of the run) - the
    # reduced system P + sigma I + A' rho A at rho ~ 1e6 is not QDLDL's quasi-definite one.  The other five agree to round-off.
    d = np.abs(xd - xo).max(axis=1)
    assert np.array_equal(sd, so) and np.array_equal(nd, no)
    assert d[[0, 1, 2, 4, 5]].max() < 1e-9 and d[3] < 1e-4, d
    ctx.close()


@pytest.mark.gpu
def test_small_problems_unit_with_the_generic_qp_backend_on_device(gpu_ctx_factory, orc):
    ctx = gpu_ctx_factory()
    xd, sd, nd = _small_problems(orc, ctx)
    _check_small(xd, sd)
    ctx.close()

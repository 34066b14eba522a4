"""Batched trajectory collision check (include/tmx.h: tmx_check_trajectories, tmx_best_trajectories_checked).

The yardstick is the oracle's CollisionConstraint: a description of the same scene whose only constraint is a collision term with
coefficient 1, no safety_margin_buffer and no fixed steps, carrying the check's evaluator type, margin, longest valid segment length
and max_substates, gives one violation per step (types 0 / 1) or per segment (types 2..4) - that is `penetration`, to 1e-12 (the bar
of every parity_checks.check_evaluate call on collision values).  With margin 10 every contact counts, so a scene with one primitive
and one obstacle also pins `min_distance` = 10 - violation.  Types 2 / 4 on spheres are restated in numpy on top.

Shapes: the 4-DOF test arm (three link primitives), T = 6, two obstacles, n = 3 trajectories with UNEQUAL segment lengths: at
lvs = 0.05 |goal - start| the first segment does not split, the second splits into 3 sub-states, the others reach 5 and 8 - with
max_substates 5 one is at the cap and one clamped by it, with max_substates 2 every segment is clamped.  Every check runs with the
default tile, with TMX_CHECK_TILE = the items of one step (one step per chunk) and with TMX_CHECK_TILE = 4 (a tile smaller than one
step that straddles sub-states), and the three must give the same bytes.

Tiers: the host build (one thread per workgroup), the SIMT emulation (256 fibers) and, marked gpu, the device.
"""
import ctypes as C

import numpy as np
import pytest

import parity_checks as pc
from test_simt_emulation import simt_lib  # noqa: F401  (fixture)
from trajopt_amd import abi, configs, runtime
from trajopt_amd.problem import CollisionTermInfo

T = 6
L = float(np.linalg.norm(configs.MINI_GOAL - configs.MINI_START))
LVS = 0.05 * L
FRACTIONS = np.array([0.0, 0.02, 0.10, 0.30, 0.65, 1.0])   # segment lengths 0.02, 0.08, 0.20, 0.35, 0.35 of |goal - start|
KEYS = ("min_distance", "penetration", "worst")


@pytest.fixture(params=["host", "simt", pytest.param("gpu", marks=pytest.mark.gpu)])
def make_ctx(request):
    """a factory of contexts of the tier; every context it made is closed at the end"""
    made = []
    lib = None
    if request.param == "gpu":
        factory = request.getfixturevalue("gpu_ctx_factory")
    else:
        lib = request.getfixturevalue("hostemu_lib" if request.param == "host" else "simt_lib")
        factory = lambda: runtime.Context(0, lib)  # noqa: E731

    def make():
        made.append(factory())
        return made[-1]
    make.tier = request.param
    make.lib_path = None if request.param == "gpu" else lib
    yield make
    for c in made:
        c.close()


def trajectories(n=3, use_time=False):
    """n trajectories from MINI_START to MINI_GOAL at unequal steps; the later ones leave the straight line in the interior"""
    rng = np.random.default_rng(11)
    x = np.stack([configs.MINI_START[None, :] + FRACTIONS[:, None] * (configs.MINI_GOAL - configs.MINI_START)[None, :] for _ in range(n)])
    for b in range(1, n):
        x[b, 1:-1] += rng.uniform(-0.02, 0.02, (T - 2, 4))
    if use_time:
        x = np.concatenate([x, rng.uniform(0.5, 2.0, (n, T, 1))], axis=2)
    return x


def scene(kind="sphere"):
    """(pci without a collision term, obstacle list): the test arm over T waypoints and two obstacles of the kind next to its path"""
    cid = {"sphere": None, "capsule": 29, "box": 31, "mesh": 34, "capsule_links": 29, "hull": 45}[kind]
    pci, _, _ = configs.config_mini(T) if cid is None else pc.cfg(cid, T=T)
    if kind == "sphere":
        (c0, r0) = pci.obstacles[0]
        pci.obstacles = [(c0, r0), ((c0[0] - 0.1, c0[1] + 0.15, c0[2] + 0.2), 0.08)]
    if kind == "capsule":
        pci.robot.link_spheres = configs.mini_arm().link_spheres   # (config 29 also has capsule links: sphere links here)
    pci.cost_infos = [ti for ti in pci.cost_infos if not isinstance(ti, CollisionTermInfo)]
    pci.cnt_infos = []
    pci.basic_info.fixed_timesteps = []
    return pci


def with_term(make_pci, cfg, first=0, last=T - 1):
    """the scene (a fresh one from make_pci) with ONE constraint: the collision term that carries the check's settings (coefficient 1,
    no buffer, no fixed steps)"""
    p = make_pci()
    p.cnt_infos = [CollisionTermInfo(first_step=first, last_step=last, dist_pen=cfg.margin, coeff=1.0, safety_margin_buffer=0.0, is_constraint=True,
                                     fixed_steps=[], evaluator_type=cfg.evaluator_type, longest_valid_segment_length=cfg.longest_valid_segment_length,
                                     max_substates=max(2, cfg.max_substates))]
    return p


def make_cfg(ev, margin, kmax=5):
    # (CONTINUOUS never splits in the check; the term of the oracle has no such type of its own: it gets a length no segment reaches)
    return abi.default_check_config(ev, margin, 1e3 if ev == 3 else LVS, kmax)


def upload(ctx, pci):
    ctx.upload(pci.to_desc(), abi.default_sqp_params(), abi.default_osqp_settings())


def step_items(ctx, cfg):
    """items of one step at the cap of sub-states (what TMX_CHECK_TILE is measured in)"""
    ev, k = cfg.evaluator_type, max(2, cfg.max_substates)
    nsub = 1 if ev in (0, 1, 3) else (k - 1 if ev == 4 else k)
    return max(1, nsub * ctx.desc.n_link_spheres * ctx.desc.n_obstacles)


def as_bytes(r):
    return tuple(np.ascontiguousarray(r[k]).tobytes() for k in KEYS)


def check(ctx, cfg, x=None):
    """check_trajectories under the default tile and under both forced decompositions: equal bytes; returns the default's result"""
    r = ctx.check_trajectories(cfg, x)
    with pytest.MonkeyPatch.context() as mp:
        for tile in (step_items(ctx, cfg), 4):
            mp.setenv("TMX_CHECK_TILE", str(tile))
            assert as_bytes(ctx.check_trajectories(cfg, x)) == as_bytes(r), f"TMX_CHECK_TILE={tile} changes the result"
    return r


def oracle_violations(orc, make_pci, cfg, x):
    """[n][T] (types 0 / 1) or [n][T - 1]: CollisionConstraint::violation of every step / segment"""
    desc = with_term(make_pci, cfg).to_desc()
    out = []
    for b in range(x.shape[0]):
        _, vv = orc.evaluate(desc, x[b], x[b])
        out.append(vv)
    return np.stack(out)


# ---- 1. against the oracle: every evaluator type and primitive kind ----------------------------------------------------------------
CASES = ([(k, ev) for k in ("sphere", "capsule", "box", "mesh") for ev in (1, 2, 3, 4)] + [("capsule_links", 1), ("capsule_links", 2)] +
         [("hull", 2), ("hull", 4)])


@pytest.mark.parametrize("kind,ev", CASES)
def test_penetration_is_the_oracles_violation(make_ctx, orc, kind, ev):
    pci = scene(kind)
    x = trajectories(3)
    ctx = make_ctx()
    # (a cast check of the hull scene needs no cast term: its links are hulls already; the capsule links stay capsules)
    upload(ctx, pci)
    assert bool(ctx.desc.n_hull_vertices) == (kind == "hull")
    for kmax in (2, 5):
        d_all = check(ctx, make_cfg(ev, 10.0, kmax), x)["min_distance"]
        d_all = d_all[d_all < 1e299]
        # a margin between the smallest and the largest per-step distance of the scene: the hinge clips some contacts, not all
        clip = float(0.5 * (d_all.min() + d_all.max()))
        for margin in (10.0, clip):
            cfg = make_cfg(ev, margin, kmax)
            r = check(ctx, cfg, x)
            vv = oracle_violations(orc, lambda: scene(kind), cfg, x)
            ne = vv.shape[1]
            assert ne == (T if ev < 2 else T - 1)
            err = float(np.abs(r["penetration"][:, :ne] - vv).max())
            print(f"{kind} type {ev} max_substates {kmax} margin {margin:.4f}: |penetration - oracle| = {err:.3e}")
            assert err <= 1e-12
            if margin == clip:
                assert (r["penetration"][:, :ne] > 0).any() and (vv < oracle_violations(orc, lambda: scene(kind), make_cfg(ev, 10.0, kmax), x)).all()
    # n = 1 gives the first trajectory's bytes
    one = check(ctx, cfg, x[:1])
    assert all(np.ascontiguousarray(one[k]).tobytes() == np.ascontiguousarray(r[k][:1]).tobytes() for k in KEYS)


# ---- 2. minimum distance -----------------------------------------------------------------------------------------------------------
def test_min_distance_per_pair_and_worst(make_ctx, orc):
    pci = scene("sphere")
    x = trajectories(3)
    cfg = make_cfg(3, 10.0)
    full_ctx = make_ctx()
    upload(full_ctx, pci)
    full = check(full_ctx, cfg, x)
    S, O = len(pci.robot.link_spheres), len(pci.obstacles)
    pair = np.zeros((S, O, 3, T))
    for s in range(S):
        for o in range(O):
            def one_pair(s=s, o=o):
                p = scene("sphere")
                p.robot.link_spheres, p.obstacles = [p.robot.link_spheres[s]], [p.obstacles[o]]
                return p
            ctx = make_ctx()
            upload(ctx, one_pair())
            r = check(ctx, cfg, x)
            vv = oracle_violations(orc, one_pair, cfg, x)
            err = float(np.abs(r["min_distance"][:, :T - 1] - (10.0 - vv)).max())
            print(f"pair ({s}, {o}): |min_distance - (10 - violation)| = {err:.3e}")
            assert err <= 1e-12
            assert (r["worst"]["primitive"] == 0).all() and (r["worst"]["obstacle"] == 0).all() and (r["worst"]["substate"] == 0).all()
            pair[s, o] = r["min_distance"]
            ctx.close()
    flat = pair.reshape(S * O, 3, T)
    assert full["min_distance"].tobytes() == flat.min(axis=0).tobytes()      # a minimum does not round
    for b in range(3):
        w = full["worst"][b]
        per_step = flat[:, b, :T - 1]
        k, t = np.unravel_index(np.argmin(per_step), per_step.shape)
        assert (w["step"], w["primitive"], w["obstacle"], w["substate"]) == (t, k // O, k % O, 0)
        assert w["min_distance"] == per_step[k, t] == full["min_distance"][b].min()
    # tie: two identical obstacles - the lower index wins
    p = scene("sphere")
    p.obstacles = [pci.obstacles[1], pci.obstacles[1], pci.obstacles[0]]
    ctx = make_ctx()
    upload(ctx, p)
    r = check(ctx, cfg, x)
    assert r["min_distance"].tobytes() == full["min_distance"].tobytes()
    for b in range(3):
        want_o = {1: 0, 0: 2}[int(full["worst"][b]["obstacle"])]
        assert int(r["worst"][b]["obstacle"]) == want_o and r["worst"][b]["step"] == full["worst"][b]["step"]
    assert (full["worst"]["obstacle"] == 1).any()   # (the tie is exercised: some trajectory is closest to the doubled obstacle)


def lin_spaced(size, low, high, i):
    """Eigen's LinSpaced as lin_spaced_at (tmx_terms.h) states it"""
    step = (high - low) / (size - 1)
    if abs(high) < abs(low):
        return low if i == 0 else high - (size - 1 - i) * step
    return high if i == size - 1 else low + i * step


def restate(pci, cfg, x):
    """numpy restatement for sphere links and sphere obstacles, types 2 / 4: (min_distance, penetration) [n][T]"""
    rob, ev, kmax = pci.robot, cfg.evaluator_type, max(2, cfg.max_substates)
    md, pen = np.full((x.shape[0], T), 1e300), np.zeros((x.shape[0], T))

    def centres(q):
        links = rob.fk_links(q)
        return [links[ls[0]][:3, :3] @ np.asarray(ls[1]) + links[ls[0]][:3, 3] for ls in rob.link_spheres]
    for b in range(x.shape[0]):
        for t in range(T - 1):
            q0, q1 = x[b, t, :4], x[b, t + 1, :4]
            dist = float(np.sqrt(((q1 - q0) ** 2).sum()))
            cnt = min(kmax, int(np.ceil(dist / cfg.longest_valid_segment_length)) + 1 if dist > cfg.longest_valid_segment_length else 2)
            states = [centres(np.array([lin_spaced(cnt, q0[j], q1[j], i) for j in range(4)])) for i in range(cnt)]
            ds = []
            for i in range(cnt if ev == 2 else cnt - 1):
                for s, ls in enumerate(rob.link_spheres):
                    for (oc, orad) in pci.obstacles:
                        a = states[i][s]
                        if ev == 2:
                            d = np.linalg.norm(a - np.asarray(oc))
                        else:   # point-to-segment distance: the obstacle centre against the swept centre
                            e = states[i + 1][s] - a
                            tau = np.clip(((np.asarray(oc) - a) @ e) / (e @ e), 0.0, 1.0) if e @ e > 0 else 0.0
                            d = np.linalg.norm(a + tau * e - np.asarray(oc))
                        ds.append(d - ls[2] - orad)
            md[b, t] = min(ds)
            pen[b, t] = sum(max(0.0, cfg.margin - d) for d in ds)
    return md, pen


@pytest.mark.parametrize("ev", [2, 4])
def test_lvs_types_against_a_numpy_restatement(make_ctx, ev):
    pci = scene("sphere")
    x = trajectories(3)
    ctx = make_ctx()
    upload(ctx, pci)
    for kmax in (2, 5):
        for margin in (10.0, 0.25):
            cfg = make_cfg(ev, margin, kmax)
            r = check(ctx, cfg, x)
            md, pen = restate(pci, cfg, x)
            e1, e2 = float(np.abs(r["min_distance"] - md).max()), float(np.abs(r["penetration"] - pen).max())
            print(f"type {ev} max_substates {kmax} margin {margin}: |min_distance| {e1:.3e} |penetration| {e2:.3e}")
            assert e1 <= 1e-12 and e2 <= 1e-12


# ---- 3. consistency ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ev", [1, 2, 3, 4])
def test_consistency(make_ctx, ev):
    pci = scene("box")
    x = trajectories(3)
    ctx = make_ctx()
    upload(ctx, pci)
    cfg = make_cfg(ev, 0.12)
    r = check(ctx, cfg, x)
    assert ((r["penetration"] > 0) == (r["min_distance"] < cfg.margin)).all()
    assert (r["penetration"] > 0).any() and (r["penetration"] == 0).any()
    assert (r["free"] == (r["min_distance"] >= cfg.margin).all(axis=1)).all()
    if ev >= 2:
        assert (r["min_distance"][:, T - 1] == 1e300).all() and (r["penetration"][:, T - 1] == 0).all()
    assert (r["worst"]["min_distance"] == r["min_distance"].min(axis=1)).all()
    # x_host = NULL after set_x0: the same bytes as the trajectories passed through x_host
    ctx.set_x0(x)
    assert as_bytes(check(ctx, cfg, None)) == as_bytes(r)
    # a use_time problem: the bytes of the same joints without the time column
    pt = scene("box")
    pt.basic_info.use_time = True
    ct = make_ctx()
    upload(ct, pt)
    xt = trajectories(3, use_time=True)
    assert (xt[:, :, :4] == x).all() and ct.D == 5
    assert as_bytes(check(ct, cfg, xt)) == as_bytes(r)
    # a scene without obstacles
    pe = scene("box")
    pe.obstacles = []
    ce = make_ctx()
    upload(ce, pe)
    e = check(ce, cfg, x)
    assert (e["min_distance"] == 1e300).all() and (e["penetration"] == 0).all() and e["free"].all()
    assert all((e["worst"][k] == -1).all() for k in ("step", "primitive", "obstacle", "substate")) and (e["worst"]["min_distance"] == 1e300).all()


# ---- 4. independence of the decomposition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ev", [("sphere", 1), ("box", 2), ("mesh", 4), ("capsule", 3), ("hull", 4)])
def test_host_build_and_simt_emulation_give_equal_bytes(hostemu_lib, simt_lib, kind, ev):  # noqa: F811
    pci = scene(kind)
    x = trajectories(3)
    got = []
    for lib in (hostemu_lib, simt_lib):
        ctx = runtime.Context(0, lib)
        upload(ctx, pci)
        got.append([as_bytes(check(ctx, make_cfg(ev, m, k), x)) for k in (2, 5) for m in (10.0, 0.12)])
        ctx.close()
    assert got[0] == got[1]


# ---- 5. selection ------------------------------------------------------------------------------------------------------------------
def selection_problem():
    """config_mini WITHOUT its collision cost (the seeds are free to cut through the obstacle), 2 queries x 8 seeds"""
    pci, s, g = configs.config_mini(8)
    pci.cost_infos = [ti for ti in pci.cost_infos if not isinstance(ti, CollisionTermInfo)]
    x0 = np.concatenate([configs.seeds_for(9, pci, s, g, 8, sigma=0.25, first=0), configs.seeds_for(9, pci, s, g, 8, sigma=0.25, first=8)])
    return pci, x0


def rule(res, chk, margin, Q, S):
    """the rule of tmx_best_trajectories_checked in numpy"""
    idx, cost, clear = np.full(Q, -1, np.int64), np.full(Q, 1e300), np.full(Q, 1e300)
    xs = np.zeros((Q,) + res["x"].shape[1:])
    for q in range(Q):
        for b in range(q * S, (q + 1) * S):
            if res["status"][b] == abi.OPT_CONVERGED and (chk["min_distance"][b] >= margin).all() and res["total_cost"][b] < cost[q]:
                idx[q], cost[q] = b, res["total_cost"][b]
        if idx[q] >= 0:
            clear[q], xs[q] = chk["min_distance"][idx[q]].min(), res["x"][idx[q]]
    return idx, cost, clear, xs


def test_best_collision_free_seed_per_query(make_ctx):
    pci, x0 = selection_problem()
    Q, S = 2, 8
    ctx = make_ctx()
    upload(ctx, pci)
    ctx.set_queries(Q)
    ctx.set_x0(x0)
    assert ctx.run(0) == 0
    res = ctx.results()
    cfg = make_cfg(4, 0.0)
    chk = check(ctx, cfg, None)
    assert as_bytes(chk) == as_bytes(check(ctx, cfg, res["x"]))
    conv = res["status"] == abi.OPT_CONVERGED
    clear = chk["min_distance"].min(axis=1)
    bi, bc = ctx.argmin_queries()
    # the margin: just above the clearance of a query's lowest-cost converged seed, below that of another converged seed of the query
    margin = None
    for q in range(Q):
        if bi[q] < 0:
            continue
        others = [b for b in range(q * S, (q + 1) * S) if conv[b] and clear[b] > clear[bi[q]]]
        if others:
            margin = float(0.5 * (clear[bi[q]] + min(clear[b] for b in others)))
            break
    assert margin is not None, "precondition: in some query the lowest-cost converged seed is not the one with the largest clearance"
    cfg.margin = margin
    chk = check(ctx, cfg, None)
    want = rule(res, chk, margin, Q, S)
    assert any(bi[q] >= 0 and not chk["free"][bi[q]] and want[0][q] >= 0 for q in range(Q)), "precondition: a lowest-cost seed in collision, another one free"
    got = ctx.best_trajectories_checked(cfg)
    with pytest.MonkeyPatch.context() as mp:
        for tile in (step_items(ctx, cfg), 4):
            mp.setenv("TMX_CHECK_TILE", str(tile))
            again = ctx.best_trajectories_checked(cfg)
            assert all(again[k].tobytes() == got[k].tobytes() for k in got)
    assert (got["index"] == want[0]).all() and got["total_cost"].tobytes() == want[1].tobytes()
    assert got["min_distance"].tobytes() == want[2].tobytes() and got["x"].tobytes() == want[3].tobytes()
    assert (got["found"] == (want[0] >= 0)).all()
    # no restriction: what argmin_queries / best_trajectories return
    cfg.margin = -1e300
    free = ctx.best_trajectories_checked(cfg)
    bx, found = ctx.best_trajectories()
    assert (free["index"] == bi).all() and free["total_cost"].tobytes() == bc.tobytes() and free["x"].tobytes() == bx.tobytes()
    assert (free["found"] == found).all()
    # a margin above every distance: nothing is free
    cfg.margin = 5.0
    none = ctx.best_trajectories_checked(cfg)
    assert (none["index"] == -1).all() and (none["total_cost"] == 1e300).all() and not none["x"].any() and not none["found"].any()
    # one query: the whole batch
    ctx.set_queries(1)
    ctx.set_x0(x0)
    assert ctx.run(0) == 0
    cfg.margin = margin
    res1, chk1 = ctx.results(), ctx.check_trajectories(cfg)
    one, w1 = ctx.best_trajectories_checked(cfg), rule(res1, chk1, margin, 1, Q * S)
    assert (one["index"] == w1[0]).all() and one["total_cost"].tobytes() == w1[1].tobytes() and one["x"].tobytes() == w1[3].tobytes()


def test_optimizer_surface(make_ctx):
    """BatchedTrustRegionSQP: check_trajectories(x=...) before initialize() as the reference's tests check the initial trajectory, and
    best_per_query(check=...)"""
    pci, x0 = selection_problem()
    if make_ctx.tier == "gpu":
        make_ctx().close()   # (the tier's own checks of the library and the device)
    opt = runtime.BatchedTrustRegionSQP(pci, lib_path=make_ctx.lib_path)
    ctx = opt.ctx
    cfg = make_cfg(4, 0.0)
    before = opt.check_trajectories(cfg, x=x0)
    assert before["min_distance"].shape == (16, 8)
    cfg.margin = float(np.median(before["min_distance"].min(axis=1)))   # at this margin part of the initial trajectories is in collision
    before = opt.check_trajectories(cfg, x=x0)
    assert before["free"].any() and not before["free"].all()
    opt.initialize(x0)
    opt.optimize()
    plain, checked = opt.best_per_query(), opt.best_per_query(check=cfg)
    assert set(checked) == set(plain) | {"min_distance"}
    want = ctx.best_trajectories_checked(cfg)
    assert all(checked[k].tobytes() == want[k].tobytes() for k in want)
    assert checked["found"].any() and (checked["min_distance"][checked["found"]] >= cfg.margin).all()
    ctx.close()


# ---- 6. refusals and state ---------------------------------------------------------------------------------------------------------
def _refused(ctx, status, call):
    with pytest.raises(runtime.TmxError) as e:
        call()
    head, reason = str(e.value).split(":", 1)
    assert head == f"tmx status {status}" and len(reason.strip()) > 20, str(e.value)


def test_refusals_and_state(make_ctx):
    pci = scene("sphere")
    x = trajectories(3)
    ctx = make_ctx()
    ctx.T, ctx.D = T, 4
    ok = make_cfg(4, 0.0)
    _refused(ctx, abi.TMX_ERR_STATE, lambda: ctx.check_trajectories(ok, x))             # no problem
    _refused(ctx, abi.TMX_ERR_STATE, lambda: ctx.best_trajectories_checked(ok))
    upload(ctx, pci)
    raw = lambda cfgp, xp, n: ctx._chk(ctx.lib.tmx_check_trajectories(ctx.h, cfgp, xp, n, None, None, None))  # noqa: E731
    _refused(ctx, abi.TMX_ERR_STATE, lambda: raw(C.byref(ok), None, 3))                   # x_host == NULL without a batch
    _refused(ctx, abi.TMX_ERR_STATE, lambda: ctx.best_trajectories_checked(ok))           # no batch
    _refused(ctx, abi.TMX_ERR_INVALID, lambda: raw(None, runtime._ptr(x), 3))             # null config
    _refused(ctx, abi.TMX_ERR_INVALID, lambda: raw(C.byref(ok), runtime._ptr(x), 0))      # n < 1
    bad = x.copy()
    bad[1, 2, 3] = np.nan
    _refused(ctx, abi.TMX_ERR_INVALID, lambda: ctx.check_trajectories(ok, bad))
    bad[1, 2, 3] = np.inf
    _refused(ctx, abi.TMX_ERR_INVALID, lambda: ctx.check_trajectories(ok, bad))
    for ev, margin, lvs, kmax in ((4, np.nan, LVS, 5), (4, 0.0, np.inf, 5), (4, 0.0, 0.0, 5), (2, 0.0, -1.0, 5), (5, 0.0, LVS, 5), (-1, 0.0, LVS, 5),
                                  (4, 0.0, LVS, -1), (4, 0.0, LVS, 0x8000)):
        _refused(ctx, abi.TMX_ERR_INVALID, lambda: ctx.check_trajectories(abi.default_check_config(ev, margin, lvs, kmax), x))
    # lvs is not read by the types that never split; max_substates 0 means 2
    assert as_bytes(ctx.check_trajectories(abi.default_check_config(3, 0.0, 0.0, 0), x)) == as_bytes(ctx.check_trajectories(make_cfg(3, 0.0, 2), x))
    assert as_bytes(ctx.check_trajectories(abi.default_check_config(1, 0.0, -1.0, 0), x)) == as_bytes(ctx.check_trajectories(make_cfg(0, 0.0), x))
    ctx.set_x0(x)
    _refused(ctx, abi.TMX_ERR_INVALID, lambda: raw(C.byref(ok), None, 2))                 # x_host == NULL: n must equal the batch
    # the library's default config
    d = ctx.default_check_config()
    assert (d.evaluator_type, d.max_substates, d.margin, d.longest_valid_segment_length) == (4, 32, 0.0, 0.05)
    assert as_bytes(ctx.check_trajectories()) == as_bytes(ctx.check_trajectories(d, x))
    # capsule links under a cast check: refused; under the discrete checks: fine
    cap = make_ctx()
    upload(cap, scene("capsule_links"))
    for ev in (3, 4):
        _refused(cap, abi.TMX_ERR_UNSUPPORTED, lambda: cap.check_trajectories(make_cfg(ev, 0.0), x))
    cap.set_x0(x)
    _refused(cap, abi.TMX_ERR_UNSUPPORTED, lambda: cap.best_trajectories_checked(make_cfg(4, 0.0)))
    cap.check_trajectories(make_cfg(2, 0.0), x)
    # a pending launch refuses both calls
    ctx.launch()
    _refused(ctx, abi.TMX_ERR_STATE, lambda: ctx.check_trajectories(ok, x))
    _refused(ctx, abi.TMX_ERR_STATE, lambda: ctx.best_trajectories_checked(ok))
    ctx.wait()
    ctx.check_trajectories(ok)

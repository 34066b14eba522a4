#!/usr/bin/env python3
"""Times the trajectory collision check on glass_upright (configuration 1, its link spheres and its obstacle), 1 024 trajectories x 30
waypoints, LVS_CONTINUOUS at the default config (margin 0, lvs 0.05, max_substates 32) on one MI355X and writes
profiles/check_trajectories_timing.txt:

  (a) tmx_check_trajectories on the resident batch (the iterates the optimizer left), all three outputs copied back;
  (b) tmx_best_trajectories_checked on 32 queries x 32 seeds (only the converged seeds are checked, only the winners come back);
  (c) the route without the check: tmx_sqp_results (all B x T x D doubles to the host), a second upload whose collision term carries
      the check's settings, tmx_batch_set_x0 (the doubles go back), tmx_evaluate - at the largest max_substates the upload accepts.

Every way runs REPS times after one warm-up; medians and spreads (max - min) in ms.

    python tools/time_check.py [--reps 5] [--out profiles/check_trajectories_timing.txt]

With --self the self-collision side instead (tmx_check_set_link_pairs with every pair of NON-ADJACENT links that carry primitives), written
to profiles/check_self_timing.txt: tmx_check_self_trajectories next to tmx_check_trajectories on the same resident batch, and
tmx_best_trajectories_checked on 32 queries x 32 seeds with and without the pairs.

    python tools/time_check.py --self [--reps 5] [--out profiles/check_self_timing.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trajopt_amd import abi, configs, runtime  # noqa: E402
from trajopt_amd.problem import CollisionTermInfo  # noqa: E402

Q, S = 32, 32


def goals_for(pci, goal):
    """32 goals around the configuration's own that differ in the shoulder pan only: the upright constraint at the goal stays feasible
    (the goals of tools/time_multi_query.py also move the elbow, and no seed converges there)"""
    pan = np.eye(len(goal))[0]
    return np.stack([np.clip(goal + pan * (-0.4 + 0.025 * q), pci.robot.lower + 0.05, pci.robot.upper - 0.05) for q in range(Q)])


def timed(fn, reps):
    fn()   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), max(ts) - min(ts)


def item_count(x, n_dof, cfg, so):
    """(swept sub-segments, items) of the trajectories x under cfg: the sub-state rule of the check"""
    d = np.sqrt(((x[:, 1:, :n_dof] - x[:, :-1, :n_dof]) ** 2).sum(axis=2))
    cnt = np.where(d > cfg.longest_valid_segment_length, np.ceil(d / cfg.longest_valid_segment_length) + 1, 2)
    sub = int((np.minimum(cnt, max(2, cfg.max_substates)) - 1).sum())
    return sub, sub * so


def main_self(args):
    pci, start, goal = configs.config1()
    B, T, D = Q * S, pci.basic_info.n_steps, pci.robot.n_dof
    links = sorted({ls[0] for ls in pci.robot.link_spheres})
    pairs = [(a, b) for a in links for b in links if b - a >= 2]
    sqp, osqp = abi.default_sqp_params(), abi.default_osqp_settings()
    cfg = abi.default_check_config()
    ctx = runtime.Context(0, args.lib)
    ctx.upload(pci.to_desc(), sqp, osqp)
    ctx.check_set_link_pairs(pairs)
    n_pairs, pp = ctx.check_link_pairs()
    so = len(pci.robot.link_spheres) * len(pci.obstacles)
    lines = ["glass_upright: %d trajectories x %d waypoints, %d link spheres x %d obstacle(s), %d non-adjacent link pairs = %d primitive pairs; "
             "LVS_CONTINUOUS, margin %g, lvs %g, max_substates %d; one MI355X, %d runs after one warm-up" %
             (B, T, len(pci.robot.link_spheres), len(pci.obstacles), n_pairs, pp, cfg.margin, cfg.longest_valid_segment_length, cfg.max_substates, args.reps),
             "way                                                          ms (median, spread)   swept sub-segments        items"]
    ctx.set_x0(configs.seeds_for(1, pci, start, goal, B))
    ctx.run(0)
    res = ctx.results()
    sub, items = item_count(res["x"], D, cfg, so)
    med, spread = timed(lambda: ctx.check_trajectories(cfg), args.reps)
    lines.append("%-60s %9.3f  %9.3f   %18d %12d" % ("tmx_check_trajectories, resident batch, 3 outputs", med, spread, sub, items))
    sub, items = item_count(res["x"], D, cfg, pp)
    med, spread = timed(lambda: ctx.check_self_trajectories(cfg), args.reps)
    slf = ctx.check_self_trajectories(cfg)
    lines.append("%-60s %9.3f  %9.3f   %18d %12d" % ("tmx_check_self_trajectories, the same batch, 3 outputs", med, spread, sub, items))
    lines.append("    %d of %d trajectories free of themselves; smallest self distance %.6f" % (int(slf["free"].sum()), B, float(slf["min_distance"].min())))
    goals = goals_for(pci, goal)
    ctx.upload(pci.to_desc(), sqp, osqp)
    ctx.set_queries(Q)
    ctx.set_query_targets(pci.term_index(pci.cnt_infos[-1]), goals)
    ctx.set_x0(np.concatenate([configs.seeds_for(1, pci, start, goals[q], S, first=q * S) for q in range(Q)]))
    ctx.run(0)
    conv = ctx.results()["status"] == abi.OPT_CONVERGED
    med, spread = timed(lambda: ctx.best_trajectories_checked(cfg), args.reps)
    plain = ctx.best_trajectories_checked(cfg)
    lines.append("%-60s %9.3f  %9.3f" % ("tmx_best_trajectories_checked, %d x %d seeds, no pairs" % (Q, S), med, spread))
    ctx.check_set_link_pairs(pairs)
    med, spread = timed(lambda: ctx.best_trajectories_checked(cfg), args.reps)
    both = ctx.best_trajectories_checked(cfg)
    lines.append("%-60s %9.3f  %9.3f" % ("tmx_best_trajectories_checked, %d x %d seeds, with the pairs" % (Q, S), med, spread))
    lines.append("    %d of %d seeds converged; queries with a free converged seed: %d without the pairs, %d with them" %
                 (int(conv.sum()), B, int(plain["found"].sum()), int(both["found"].sum())))
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out or os.path.join(ROOT, "profiles", "check_self_timing.txt"), "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="default: profiles/check_trajectories_timing.txt (profiles/check_self_timing.txt with --self)")
    ap.add_argument("--lib", default=None, help="another build of the library (default: the product library)")
    ap.add_argument("--self", dest="self_check", action="store_true", help="time the self-collision side instead")
    args = ap.parse_args()
    if args.self_check:
        return main_self(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "check_trajectories_timing.txt")
    pci, start, goal = configs.config1()
    B, T, D = Q * S, pci.basic_info.n_steps, pci.robot.n_dof
    so = len(pci.robot.link_spheres) * len(pci.obstacles)
    sqp, osqp = abi.default_sqp_params(), abi.default_osqp_settings()
    cfg = abi.default_check_config()
    ctx = runtime.Context(0, args.lib)
    lines = ["glass_upright: %d trajectories x %d waypoints, %d link spheres x %d obstacle(s); LVS_CONTINUOUS, margin %g, lvs %g, max_substates %d; "
             "one MI355X, %d runs after one warm-up" % (B, T, len(pci.robot.link_spheres), len(pci.obstacles), cfg.margin,
                                                        cfg.longest_valid_segment_length, cfg.max_substates, args.reps),
             "way                                                          ms (median, spread)   swept sub-segments        items"]

    # (a) the resident batch of one query
    ctx.upload(pci.to_desc(), sqp, osqp)
    ctx.set_x0(configs.seeds_for(1, pci, start, goal, B))
    ctx.run(0)
    res = ctx.results()
    sub, items = item_count(res["x"], D, cfg, so)
    med, spread = timed(lambda: ctx.check_trajectories(cfg), args.reps)
    chk = ctx.check_trajectories(cfg)
    lines.append("%-60s %9.3f  %9.3f   %18d %12d" % ("(a) tmx_check_trajectories, resident batch, 3 outputs", med, spread, sub, items))
    lines.append("    %d of %d trajectories free, %d converged; smallest distance %.6f" %
                 (int(chk["free"].sum()), B, int((res["status"] == abi.OPT_CONVERGED).sum()), float(chk["min_distance"].min())))

    # (c) on the same batch: download, second upload with the check's settings in a collision term, set_x0, evaluate
    k = cfg.max_substates
    while True:
        p2, _, _ = configs.config1(with_collision=False)
        p2.obstacles = list(pci.obstacles)
        p2.cnt_infos.append(CollisionTermInfo(first_step=0, last_step=T - 1, dist_pen=cfg.margin, coeff=1.0, safety_margin_buffer=0.0,
                                              is_constraint=True, fixed_steps=[], evaluator_type=cfg.evaluator_type,
                                              longest_valid_segment_length=cfg.longest_valid_segment_length, max_substates=k))
        desc2 = p2.to_desc()
        try:
            ctx.upload(desc2, sqp, osqp)
            ctx.set_x0(res["x"])
            n_slots = ctx.R
            break
        except runtime.TmxError as e:
            lines.append("    (c) max_substates %d refused: %s" % (k, str(e)[:160]))
            if k <= 2:
                raise
            k //= 2
    desc1 = pci.to_desc()

    def route_c():
        x = res["x"]                      # stands for tmx_sqp_results: timed separately below (the batch must be resident for it)
        ctx.upload(desc2, sqp, osqp)
        ctx.set_x0(x)
        return ctx.evaluate()
    med_c, spread_c = timed(route_c, args.reps)
    c2 = abi.default_check_config(cfg.evaluator_type, cfg.margin, cfg.longest_valid_segment_length, k)
    sub_c, items_c = item_count(res["x"], D, c2, so)
    ctx.upload(desc1, sqp, osqp)
    ctx.set_x0(res["x"])
    med_r, spread_r = timed(ctx.results, args.reps)
    lines.append("%-60s %9.3f  %9.3f   %18d %12d" % ("(c) second upload + set_x0 + tmx_evaluate, max_substates %d" % k, med_c, spread_c, sub_c, items_c))
    lines.append("%-60s %9.3f  %9.3f" % ("    + tmx_sqp_results before it (B x T x D doubles)", med_r, spread_r))
    lines.append("    (c) returns hinge sums per segment only: no distances, no closest contact; max_substates is the row-slot capacity of a term"
                 " (%d accepted here, %d asked for; %d row slots), and the planner's problem has to be uploaded again afterwards" %
                 (k, cfg.max_substates, n_slots))

    # (b) 32 queries x 32 seeds
    goals = goals_for(pci, goal)
    ctx.upload(desc1, sqp, osqp)
    ctx.set_queries(Q)
    ctx.set_query_targets(pci.term_index(pci.cnt_infos[-1]), goals)
    ctx.set_x0(np.concatenate([configs.seeds_for(1, pci, start, goals[q], S, first=q * S) for q in range(Q)]))
    ctx.run(0)
    res = ctx.results()
    conv = res["status"] == abi.OPT_CONVERGED
    sub, items = item_count(res["x"][conv], D, cfg, so)
    med, spread = timed(lambda: ctx.best_trajectories_checked(cfg), args.reps)
    best = ctx.best_trajectories_checked(cfg)
    lines.append("%-60s %9.3f  %9.3f   %18d %12d" % ("(b) tmx_best_trajectories_checked, %d queries x %d seeds" % (Q, S), med, spread, sub, items))
    lines.append("    %d of %d seeds converged (only those are checked); %d of %d queries have a free converged seed" %
                 (int(conv.sum()), B, int(best["found"].sum()), Q))
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times glass_upright (configuration 1) with 1 024 problems on one MI355X three ways and writes profiles/multi_query_timing.txt:

  (a) one query: 1 024 seeds of the description's own goal (the headline batch);
  (b) 32 queries x 32 seeds with 32 distinct reachable goals in ONE batch (tmx_queries_set / tmx_query_set_targets);
  (c) the status quo for those goals: 32 uploads and batches of 32, one after the other on one context.

Run lengths differ with the goal, so next to the batch time the time per SQP iteration (batch time / QP solves of the batch) is
reported.  Every way runs REPS times after one warm-up; median and spread (max - min) are printed.

    python tools/time_multi_query.py [--reps 5] [--out profiles/multi_query_timing.txt]
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

Q, S = 32, 32


def goals_for(pci, goal):
    """32 goals around the configuration's own: the shoulder pan and the elbow move on a grid, inside the joint limits"""
    out = []
    for q in range(Q):
        d = np.zeros_like(goal)
        d[0] = -0.35 + 0.1 * (q % 8)
        d[3] = -0.15 + 0.1 * (q // 8)
        g = np.clip(goal + d, pci.robot.lower + 0.05, pci.robot.upper - 0.05)
        out.append(g)
    return np.stack(out)


def timed(fn, reps):
    fn()   # warm-up
    ts, its = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        n_qp = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        its.append(n_qp)
    return ts, its


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_query_timing.txt"))
    args = ap.parse_args()
    pci, start, goal = configs.config1()
    k_goal = pci.term_index(pci.cnt_infos[-1])
    goals = goals_for(pci, goal)
    sqp, osqp = abi.default_sqp_params(), abi.default_osqp_settings()
    x_one = configs.seeds_for(1, pci, start, goal, Q * S)
    x_q = [configs.seeds_for(1, pci, start, goals[q], S, first=q * S) for q in range(Q)]
    ctx = runtime.Context(0)

    def way_a():
        ctx.upload(pci.to_desc(), sqp, osqp)
        ctx.set_x0(x_one)
        ctx.run(0)
        return int(ctx.counters()["n_qp_solves"])

    def way_b():
        ctx.upload(pci.to_desc(), sqp, osqp)
        ctx.set_queries(Q)
        ctx.set_query_targets(k_goal, goals)
        ctx.set_x0(np.concatenate(x_q))
        ctx.run(0)
        n = int(ctx.counters()["n_qp_solves"])
        ctx.argmin_queries()
        return n

    descs = []
    for q in range(Q):
        p, _, _ = configs.config1()
        p.cnt_infos[-1].targets = list(goals[q])
        descs.append(p.to_desc())

    def way_c():
        n = 0
        for q in range(Q):
            ctx.upload(descs[q], sqp, osqp)
            ctx.set_x0(x_q[q])
            ctx.run(0)
            n += int(ctx.counters()["n_qp_solves"])
            ctx.argmin()
        return n

    lines = ["glass_upright, 1 024 problems, one MI355X: wall time from upload to the best seed(s), %d runs after one warm-up" % args.reps,
             "way                                      batch ms (median, spread)   QP solves   us per QP solve (median)"]
    for name, fn in (("(a) one query x 1024 seeds", way_a), ("(b) 32 queries x 32 seeds, one batch", way_b),
                     ("(c) 32 uploads x 32 seeds, in series", way_c)):
        ts, its = timed(fn, args.reps)
        per = [1e3 * t / n for t, n in zip(ts, its)]
        lines.append("%-40s %9.2f  %9.2f   %9d   %10.3f" % (name, statistics.median(ts), max(ts) - min(ts), its[0], statistics.median(per)))
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times tmx_qp_solve_batched's block-tridiagonal engine on one MI355X and writes profiles/csc_blocks_timing.txt:

  (a) 64 exported first QPs of glass_upright (configuration 1: n = 572, m = 876) through TMX_QP_ENGINE_AUTO, through tmx_qp_solve on
      the same convexification (the term-structured solver), and through the dense engine (one QP first; the batch of 64 only if
      that QP's time says it can end within the leg's time limit - "did not finish" otherwise);
  (b) both engines at the crossover: the exported QPs of the longest glass_upright with at most 448 variables;
  (c) the smallest block size of the partition (TMX_CB_BLOCK_MIN) swept on the batch of (a);
  (d) the phase split of the new kernel from a profiling build (make -C trajopt_amd/csrc OUT=../_build_prof EXTRA=-DTMX_CB_PROF=1),
      when that build exists.

Every leg runs in a process of its own under a time limit of its own.  Times are wall-clock around the call (host stage, upload,
kernel, copy back), median of --reps after one warm-up.

    python tools/time_csc_blocks.py [--reps 5] [--out profiles/csc_blocks_timing.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROF_LIB = os.path.join(ROOT, "trajopt_amd", "_build_prof", "libtrajopt_mi355x.so")
B = 64


def _ctx_with_qps(T, lib=None):
    from trajopt_amd import abi, configs, runtime
    ctx = runtime.Context(0, lib)
    pci, s, g = configs.config1(T)
    x0 = configs.seeds_for(1, pci, s, g, B)
    ctx.upload(pci.to_desc(), abi.default_sqp_params(), abi.default_osqp_settings())
    ctx.set_x0(x0)
    ctx.convexify()
    return ctx


def _median(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), max(ts) - min(ts)


def leg(name, T, reps, count):
    """one leg in this process; prints one JSON line"""
    from trajopt_amd import abi
    ctx = _ctx_with_qps(T, PROF_LIB if name == "prof" else None)
    out = dict(leg=name, T=T)
    xq, cvx, rec = ctx.qp_solve()
    qps = [ctx.export_csc(b) for b in range(B)][:count]
    out.update(n=int(qps[0]["n"]), m=int(qps[0]["m"]), count=len(qps), iters=int(sum(r.osqp_iter for r in rec[:count])))
    if name == "structured":
        out["ms"], out["spread"] = _median(ctx.qp_solve, reps)
    else:
        ctx.qp_engine_set(dict(auto=abi.QP_ENGINE_AUTO, prof=abi.QP_ENGINE_AUTO, blocks=abi.QP_ENGINE_BLOCKS, dense=abi.QP_ENGINE_DENSE)[name])
        res = []
        out["ms"], out["spread"] = _median(lambda: res.append(ctx.qp_solve_batched(qps)), reps)
        last = ctx.qp_engine_last(len(qps))
        out.update(engine=sorted(set(int(e) for e in last["engine"])), block=sorted(set(int(b) for b in last["block"])),
                   n_blocks=sorted(set(int(b) for b in last["n_blocks"])), placement=sorted(set(int(b) for b in last["placement"])),
                   solved=int(sum(r["cvx_status"] == abi.CVX_SOLVED for r in res[-1])),
                   same_iters=int(sum(r["info"].iter == rec[b].osqp_iter for b, r in enumerate(res[-1]))),
                   max_dx=float(max(np.abs(r["x"] - xq[b, :qps[b]["n"]]).max() for b, r in enumerate(res[-1]))))
    ctx.close()
    print("LEG " + json.dumps(out), flush=True)


def run_leg(name, T, reps, count, limit, env=None):
    """the leg in a child process under its own time limit; (record or None, stderr)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--T", str(T), "--reps", str(reps), "--count", str(count)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=dict(os.environ, **(env or {})))
    except subprocess.TimeoutExpired:
        return None, f"did not finish within {limit} s"
    for ln in p.stdout.splitlines():
        if ln.startswith("LEG "):
            return json.loads(ln[4:]), p.stderr
    return None, f"failed (exit code {p.returncode}): {p.stderr[-500:]}"


def find_crossover_T():
    """in this process: the longest glass_upright whose exported first QP has at most 448 variables - n read from tmx_export_csc after
    an upload and a convexification of every candidate; prints one JSON line"""
    from trajopt_amd import abi, configs, runtime
    ctx = runtime.Context(0)
    for T in range(30, 4, -1):
        pci, s, g = configs.config1(T)
        ctx.upload(pci.to_desc(), abi.default_sqp_params(), abi.default_osqp_settings())
        ctx.set_x0(configs.seeds_for(1, pci, s, g, 1))
        ctx.convexify()
        n = int(ctx.export_csc(0)["n"])
        if n <= 448:
            break
    ctx.close()
    print("LEG " + json.dumps(dict(leg="find_T", T=T, n=n)), flush=True)


def fmt(r):
    if r is None:
        return "-"
    s = f"{r['ms']:10.2f} ms (spread {r['spread']:.2f})"
    if "engine" in r:
        s += (f"  engine {r['engine']} block {r['block']} x {r['n_blocks']} placement {r['placement']}  solved {r['solved']}/{r['count']}"
              f"  iterations equal to tmx_qp_solve's {r['same_iters']}/{r['count']}  max |dx| {r['max_dx']:.2e}")
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csc_blocks_timing.txt"))
    ap.add_argument("--leg")
    ap.add_argument("--T", type=int, default=30)
    ap.add_argument("--count", type=int, default=B)
    ap.add_argument("--dense-limit", type=int, default=240, help="time limit of the dense leg, seconds")
    args = ap.parse_args()
    if args.leg == "find_T":
        return find_crossover_T()
    if args.leg:
        return leg(args.leg, args.T, args.reps, args.count)
    lines = ["tools/time_csc_blocks.py on one MI355X: wall-clock per call, median of %d after one warm-up; batch of %d QPs" % (args.reps, B), ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("(a) first QPs of glass_upright, T = 30, 64 seeds")
    st, err = run_leg("structured", 30, args.reps, B, 300)
    say(f"  tmx_qp_solve (term-structured solver)      {fmt(st) if st else err}")
    au, err = run_leg("auto", 30, args.reps, B, 300)
    say(f"  tmx_qp_solve_batched, AUTO                 {fmt(au) if au else err}")
    if st and au:
        say(f"  n = {au['n']}, m = {au['m']}, {au['iters']} ADMM iterations in the batch; AUTO / tmx_qp_solve = {au['ms'] / st['ms']:.2f}")
    d1, err = run_leg("dense", 30, 1, 1, args.dense_limit)
    say(f"  tmx_qp_solve_batched, DENSE, ONE QP        {fmt(d1) if d1 else err}")
    if d1 and 3.0 * d1["ms"] * 2 / 1e3 < args.dense_limit:   # (warm-up + 1 repetition; a batch shares HBM bandwidth: allow three times the one QP)
        d64, err = run_leg("dense", 30, 1, B, args.dense_limit)
        say(f"  tmx_qp_solve_batched, DENSE, 64 QPs        {fmt(d64) if d64 else err}")
    else:
        say(f"  tmx_qp_solve_batched, DENSE, 64 QPs        not started: one QP alone leaves no room in the leg's limit of {args.dense_limit} s")
    say()
    r, err = run_leg("find_T", 0, 1, 1, 300)
    if not r:
        say("(b) the crossover: " + err)
    T = r["T"] if r else 23
    say(f"(b) the crossover: glass_upright with T = {T}, the longest whose exported QP has at most 448 variables (n = {r['n'] if r else '?'})")
    for name in ("structured", "blocks", "dense"):
        r, err = run_leg(name, T, max(1, args.reps // 2 + 1), B, args.dense_limit)
        say(f"  {name:10s} n = {r['n'] if r else '?'}   {fmt(r) if r else err}")
    say()
    say("(c) smallest block size of the partition (TMX_CB_BLOCK_MIN), batch of (a) under AUTO")
    for mn in (4, 16, 24, 32, 48, 64, 96):
        r, err = run_leg("auto", 30, args.reps, B, 300, env={"TMX_CB_BLOCK_MIN": str(mn)})
        say(f"  min {mn:3d}: {fmt(r) if r else err}")
    say()
    say("(d) phase split of k_qp_csc_blocks (profiling build, thread 0's 100 MHz ticks, mean over the 64 QPs of (a))")
    if not os.path.exists(PROF_LIB):
        say("  no profiling build: not measured")
    else:
        r, err = run_leg("prof", 30, 1, B, 300)
        rows = [ln.split() for ln in err.splitlines() if ln.startswith("cb_prof ")]
        if not r or not rows:
            say("  " + (err if not r else "no cb_prof line"))
        else:
            rows = rows[-B:]
            keys = rows[0][3::2]
            mean = {k: statistics.mean(int(row[4 + 2 * i]) for row in rows) * 1e-5 for i, k in enumerate(keys)}   # ms
            tot = mean["total"]
            rest_admm = tot - mean["polish_total"] - mean["admm_assembly"] - mean["admm_factor"] - mean["admm_sweeps"]
            rest_pol = mean["polish_total"] - mean["polish_assembly"] - mean["polish_factor"] - mean["polish_sweeps"]
            say(f"  kernel total per QP {tot:8.2f} ms")
            for k, v in (("ADMM: assembly of K", mean["admm_assembly"]), ("ADMM: factorisation", mean["admm_factor"]), ("ADMM: sweeps", mean["admm_sweeps"]),
                         ("ADMM: sparse products, vector updates, residual checks", rest_admm), ("polish: assembly", mean["polish_assembly"]),
                         ("polish: factorisation", mean["polish_factor"]), ("polish: sweeps", mean["polish_sweeps"]),
                         ("polish: sparse products and the rest", rest_pol)):
                say(f"  {k:58s} {v:8.2f} ms  {100.0 * v / tot:5.1f} %")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

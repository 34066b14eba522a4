#!/usr/bin/env python3
"""Timings of time-parameterised problems on the device (profiles/vel_time_chain_timing.txt):

    python tools/time_vel_time_chain.py --config 52 --waypoints 30 --batch 256 --switch 1          whole SQP runs, three runs, best
    python tools/time_vel_time_chain.py --config 53 --waypoints 30 --batch 256 --with-cost        configuration 53's rows + the squared cost
    python tools/time_vel_time_chain.py --config 53 --waypoints 30 --batch 256 --lib other.so     another build of the library
    python tools/time_vel_time_chain.py --config 52 --waypoints 50 --batch 64 --crossover         first Model::optimize() on both QP engines

--config is a time-parameterised configuration of tests/parity_checks.py (48 .. 53, on the 4-DOF test arm), --with-cost replaces its
first cost by the squared JointVel-with-time cost (coefficients 1, 2, 0.5, 1.5).  --switch sets TMX_VEL_TIME_CHAIN for the upload.
Prints one line per measurement: batch time per SQP run, QP solves, ADMM iterations, batch time per ADMM iteration."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import parity_checks as pc  # noqa: E402
from trajopt_amd import abi, configs, runtime  # noqa: E402

SWITCH = "TMX_VEL_TIME_CHAIN"


def problem(cid, T, B, with_cost):
    from trajopt_amd.problem import JointVelTermInfo
    pci, s, g = pc.cfg(cid, T=T)
    if with_cost:
        n = pci.basic_info.n_steps
        pci.cost_infos[0] = JointVelTermInfo(coeffs=[1.0, 2.0, 0.5, 1.5], targets=[0.0] * 4, first_step=0, last_step=n - 1, use_time=True, name="vel_t")
    x = configs.seeds_for(9, pci, s, g, B)
    tau = 1.3 + 0.3 * np.random.default_rng(1234 + (71 if with_cost else cid)).standard_normal((B, x.shape[1], 1))
    return pci, np.concatenate([x, np.clip(tau, 0.5, 4.0)], axis=2)


def upload(pci, x0, lib, sw):
    os.environ.pop(SWITCH, None)
    if sw is not None:
        os.environ[SWITCH] = sw
    ctx = runtime.Context(0, lib)
    ctx.upload(pci.to_desc(), abi.default_sqp_params(), abi.default_osqp_settings())
    ctx.set_x0(x0)
    return ctx


def whole_runs(args, pci, x0):
    ctx = upload(pci, x0, args.lib, args.switch)
    times = []
    for rep in range(args.reps):
        ctx.set_x0(x0)
        t0 = time.perf_counter()
        ctx.run(0)
        times.append(time.perf_counter() - t0)
    r, c = ctx.results(), ctx.counters()
    best, B = min(times), x0.shape[0]
    print(f"cfg {args.config}{' + squared cost' if args.with_cost else ''} T={pci.basic_info.n_steps} B={B} switch={args.switch} n_max={ctx.n_max} R={ctx.R}: "
          f"runs {[round(t, 4) for t in times]} s, best {best:.4f} s, {best / B * 1e3:.3f} ms per SQP run (batch time / B), QP solves {c['n_qp_solves']}, "
          f"ADMM iterations {c['admm_iters']}, {best / max(1, c['admm_iters']) * 1e9:.1f} ns batch time per ADMM iteration, "
          f"converged {(r['status'] == abi.OPT_CONVERGED).mean():.3f}", flush=True)
    ctx.close()


def crossover(args, pci, x0):
    got = {}
    for name, sw in (("block chain", "1"), ("dense", "0")):
        times = []
        for rep in range(args.reps):
            ctx = upload(pci, x0, args.lib, sw)
            ctx.convexify()
            c0 = ctx.counters()["admm_iters"]
            t0 = time.perf_counter()
            xq, cvx, rec = ctx.qp_solve()
            times.append(time.perf_counter() - t0)
            iters = ctx.counters()["admm_iters"] - c0
            got[name] = (xq.copy(), [(r.osqp_status, r.osqp_iter, r.rho_updates, r.polish_status) for r in rec], min(times))
            n_max = ctx.n_max
            ctx.close()
        print(f"cfg {args.config} T={pci.basic_info.n_steps} B={x0.shape[0]} n_max={n_max} engine {name}: first Model::optimize() of the batch "
              f"{[round(t, 4) for t in times]} s, ADMM iterations {iters}, {min(times) / max(1, iters) * 1e9:.1f} ns batch time per ADMM iteration", flush=True)
    same = sum(a == b for a, b in zip(got["block chain"][1], got["dense"][1]))
    dx = float(np.abs(got["block chain"][0] - got["dense"][0]).max())
    print(f"dense / chain time: {got['dense'][2] / got['block chain'][2]:.1f} x; same (status, iterations, rho updates, polish) on {same} of {x0.shape[0]} seeds, "
          f"max |dx| {dx:.2e} (TOL_TRAJ {pc.TOL_TRAJ:g})", flush=True)
    return 0 if (same == x0.shape[0] and dx <= pc.TOL_TRAJ) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=int, required=True)
    ap.add_argument("--waypoints", type=int, required=True)
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--with-cost", action="store_true")
    ap.add_argument("--switch", default=None, choices=("0", "1"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--crossover", action="store_true")
    args = ap.parse_args()
    pci, x0 = problem(args.config, args.waypoints, args.batch, args.with_cost)
    if args.crossover:
        return crossover(args, pci, x0)
    whole_runs(args, pci, x0)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Timings of squared acceleration / jerk costs next to rows on two waypoints on the device (profiles/band_pair_chain_timing.txt):

    python tools/time_band_pair_chain.py --problem H --batch 256                       whole SQP runs, three runs, best
    python tools/time_band_pair_chain.py --problem H --batch 256 --no-cost --lib X.so  the same rows without the smoothing cost (the
                                                                                       dense-coupling chain with segmented sweeps) on another build
    python tools/time_band_pair_chain.py --crossover --batch 64                        first Model::optimize() on both QP engines

    python tools/time_band_pair_chain.py --problem P2 --batch 256                      acceleration / jerk ROWS next to such rows
                                                                                       (profiles/band_row_pair_chain_timing.txt)

--problem is a problem of tests/test_band_pair_chain.py (E .. K, S1 .. S5) or of tests/test_band_row_pair_chain.py (P1 .. P3, R1 .. R5:
uploaded with TMX_BAND_ROW_PAIR_CHAIN=1; P2 / P1 are H / E with acceleration limits on top); --no-cost drops its squared
acceleration / jerk costs; --switch sets TMX_BAND_PAIR_CHAIN for the upload.  --crossover takes the 4-DOF test arm with the cast collision cost (pc.cfg(17)) plus the
acceleration cost at the largest number of waypoints whose QP stays within the dense engine's 448 variables.
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
import test_band_pair_chain as bp  # noqa: E402
import test_band_row_pair_chain as br  # noqa: E402
from trajopt_amd import abi, runtime  # noqa: E402
from trajopt_amd.problem import JointAccTermInfo, JointJerkTermInfo  # noqa: E402


def upload(pci, x0, lib, sw, rows=False):
    for k in (bp.SWITCH, br.SWITCH, "TMX_DENSE_QP_MAX_N"):  # (an override of the dense engine's limit would change what "switch unset" measures)
        os.environ.pop(k, None)
    if sw is not None:
        os.environ[bp.SWITCH] = sw
    if rows:
        os.environ[br.SWITCH] = "1"
    ctx = runtime.Context(0, lib)
    ctx.upload(pci.to_desc(), abi.default_sqp_params(), abi.default_osqp_settings())
    ctx.set_x0(x0)
    return ctx


def whole_runs(args, pci, x0):
    ctx = upload(pci, x0, args.lib, args.switch, rows=args.problem in br.ALL)
    times = []
    for rep in range(args.reps):
        ctx.set_x0(x0)
        t0 = time.perf_counter()
        ctx.run(0)
        times.append(time.perf_counter() - t0)
    r, c = ctx.results(), ctx.counters()
    best, B = min(times), x0.shape[0]
    route = ctx.band_pairs() if hasattr(ctx.lib, "tmx_debug_band_pairs") else False
    if args.problem in br.ALL:
        assert ctx.band_row_pairs()
    print(f"problem {args.problem}{' without the smoothing costs' if args.no_cost else ''} T={pci.basic_info.n_steps} B={B} switch={args.switch} "
          f"lib={args.lib or 'default'} n_max={ctx.n_max} R={ctx.R} banded route {int(route)} workspace {ctx.workspace_info()}: "
          f"runs {[round(t, 4) for t in times]} s, best {best:.4f} s, {best / B * 1e3:.3f} ms per SQP run (batch time / B), QP solves {c['n_qp_solves']}, "
          f"ADMM iterations {c['admm_iters']}, {best / max(1, c['admm_iters']) * 1e9:.1f} ns batch time per ADMM iteration, "
          f"converged {(r['status'] == abi.OPT_CONVERGED).mean():.3f}", flush=True)
    ctx.close()


def crossover(args):
    T = 30
    while True:  # the largest horizon within the dense engine's limit
        pci, x0 = bp._mini(17, T, True, False, args.batch)
        ctx = upload(pci, x0, args.lib, "1")
        n_max = ctx.n_max
        ctx.close()
        if n_max <= 448:
            break
        T -= 1
    got = {}
    for name, sw in (("banded route", "1"), ("dense", "0")):
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
            ctx.close()
        print(f"cfg 17 + acceleration cost T={T} B={x0.shape[0]} n_max={n_max} engine {name}: first Model::optimize() of the batch "
              f"{[round(t, 4) for t in times]} s, ADMM iterations {iters}, {min(times) / max(1, iters) * 1e9:.1f} ns batch time per ADMM iteration", flush=True)
    same = sum(a == b for a, b in zip(got["banded route"][1], got["dense"][1]))
    dx = float(np.abs(got["banded route"][0] - got["dense"][0]).max())
    print(f"dense / banded time: {got['dense'][2] / got['banded route'][2]:.1f} x; same (status, iterations, rho updates, polish) on {same} of {x0.shape[0]} seeds, "
          f"max |dx| {dx:.2e} (TOL_TRAJ {pc.TOL_TRAJ:g})", flush=True)
    return 0 if (same == x0.shape[0] and dx <= pc.TOL_TRAJ) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--problem", default="H", choices=sorted(bp.ALL) + sorted(br.ALL))
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--no-cost", action="store_true")
    ap.add_argument("--switch", default=None, choices=("0", "1"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--crossover", action="store_true")
    args = ap.parse_args()
    if args.crossover:
        return crossover(args)
    pci, x0 = (br.ALL if args.problem in br.ALL else bp.ALL)[args.problem](args.batch)
    if args.no_cost:
        pci.cost_infos = [ti for ti in pci.cost_infos if not isinstance(ti, (JointAccTermInfo, JointJerkTermInfo))]
    whole_runs(args, pci, x0)
    return 0


if __name__ == "__main__":
    sys.exit(main())

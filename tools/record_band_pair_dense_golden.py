#!/usr/bin/env python3
"""Records tests/golden/band_pair_dense_parent.npz: status, counters, trajectories and total cost of the small shapes S1 (4-DOF test arm,
cast collision cost, acceleration + jerk costs, 14 waypoints) and S3 (glass_upright at 8 waypoints, LVS_CONTINUOUS collision, acceleration
cost) of tests/test_band_pair_chain.py on the dense QP engine, 4 seeds each, from a HOST BUILD of the library (tests/hostemu:
libtmx_hostemu.so).  The test compares the current host build against it byte for byte: squared acceleration / jerk costs next to rows
on two waypoints moved to the banded factorisation above the dense engine's size limit, below it nothing may change.  Run it on the host
build of the commit BEFORE that change (check that commit out into another directory, `make -C tests/hostemu` there):

    python tools/record_band_pair_dense_golden.py --lib <other checkout>/tests/hostemu/_build/libtmx_hostemu.so
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import parity_checks as pc  # noqa: E402
import test_band_pair_chain as bp  # noqa: E402
from trajopt_amd import runtime  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", required=True, help="libtmx_hostemu.so of the commit to record from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "band_pair_dense_parent.npz"))
    args = ap.parse_args()
    for k in ("TMX_BAND_PAIR_CHAIN", "TMX_DENSE_QP_MAX_N"):
        os.environ.pop(k, None)
    out = {}
    for name in ("S1", "S3"):
        pci, x0 = bp.SMALL[name](4)
        ctx = runtime.Context(0, args.lib)
        pc.make_ctx_inputs(ctx, pci, x0)
        assert ctx.n_max <= 448 and ctx.debug_flag("qp_dense") == 1
        ctx.run(0)
        r = ctx.results()
        ctx.close()
        for k in ("status", "n_qp_solves", "n_func_evals", "x", "total_cost"):
            out[f"{name}_{k}"] = np.array(r[k])
        print(f"{name}: status {r['status']}, QP solves {r['n_qp_solves']}")
    np.savez_compressed(args.out, **out)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

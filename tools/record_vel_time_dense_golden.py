#!/usr/bin/env python3
"""Records tests/golden/vel_time_dense_parent.npz: status, counters, trajectories and total cost of configurations 48 and 52 at their
default size (dense QP engine), 4 seeds each, from a HOST BUILD of the library (tests/hostemu: libtmx_hostemu.so).
tests/test_vel_time_chain.py compares the current host build against it byte for byte: squared velocity-with-time costs above the
dense engine's size limit moved to the block chain, below it nothing may change.  Run it on the host build of the commit BEFORE that
change (check that commit out into another directory, `make -C tests/hostemu` there):

    python tools/record_vel_time_dense_golden.py --lib <other checkout>/tests/hostemu/_build/libtmx_hostemu.so
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import parity_checks as pc  # noqa: E402
from trajopt_amd import configs, runtime  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", required=True, help="libtmx_hostemu.so of the commit to record from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "vel_time_dense_parent.npz"))
    args = ap.parse_args()
    for k in ("TMX_VEL_TIME_CHAIN", "TMX_TOTAL_TIME_CHAIN", "TMX_DENSE_QP_MAX_N"):
        os.environ.pop(k, None)
    out = {}
    for cid in (48, 52):
        pci, s, g = pc.cfg(cid)
        x = configs.seeds_for(9, pci, s, g, 4)
        tau = 1.3 + 0.3 * np.random.default_rng(1234 + cid).standard_normal((4, x.shape[1], 1))
        x0 = np.concatenate([x, np.clip(tau, 0.5, 4.0)], axis=2)
        ctx = runtime.Context(0, args.lib)
        pc.make_ctx_inputs(ctx, pci, x0)
        ctx.run(0)
        r = ctx.results()
        ctx.close()
        for k in ("status", "n_qp_solves", "n_func_evals", "x", "total_cost"):
            out[f"cfg{cid}_{k}"] = np.array(r[k])
        print(f"configuration {cid}: status {r['status']}, QP solves {r['n_qp_solves']}")
    np.savez_compressed(args.out, **out)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

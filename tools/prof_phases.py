"""Phase profile (needs a -DTMX_PROFILE build: make -C trajopt_amd/csrc EXTRA=-DTMX_PROFILE).
   python tools/prof_phases.py [B] [full|first] [lib.so] [config[s]]   - first QP solve only (default) or the whole optimize() run
   ("full"); config 1 (default), 2, 3 or 4, or a problem of tests/test_band_pair_chain.py ("H", "H-nocost": without its smoothing
   costs) or of tests/test_band_row_pair_chain.py ("P2", "P1": uploaded with TMX_BAND_ROW_PAIR_CHAIN=1); the word "fine5" anywhere among the arguments names the slots of a -DTMX_PROFILE -DTMX_FINE=5 build, the word "fine2" those of a -DTMX_FINE=2 build"""
import sys, os, ctypes as C, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from trajopt_amd import configs, abi, runtime
fine5 = "fine5" in sys.argv[1:]  # (a word, not a position: taken out before the positional arguments are read)
fine2 = "fine2" in sys.argv[1:]
sys.argv = [a for a in sys.argv if a not in ("fine5", "fine2")]
# a problem of tests/test_band_pair_chain.py in place of the configuration: "H", "F", ... (squared acceleration / jerk costs next to
# pair rows); "H-nocost" drops the smoothing costs (the same rows on the segmented dense-coupling chain)
bp_name = sys.argv[4] if len(sys.argv) > 4 and not sys.argv[4][0].isdigit() else None
smooth = bp_name is None and len(sys.argv) > 4 and sys.argv[4].endswith("s")  # "1s": config 1 + acceleration and jerk smoothing costs (banded path)
cid = int(sys.argv[4].rstrip("s")) if len(sys.argv) > 4 and bp_name is None else 1
pci, s, g = {1: configs.config1, 2: configs.config2, 3: configs.config3, 4: configs.config4}[cid]()
if smooth:
    from trajopt_amd.problem import JointAccTermInfo, JointJerkTermInfo
    nj = len(pci.cost_infos[0].coeffs) if hasattr(pci.cost_infos[0], "coeffs") else 7
    pci.cost_infos.append(JointAccTermInfo(coeffs=[1.0] * nj, targets=[0.0] * nj, first_step=0, last_step=pci.basic_info.n_steps - 1, name="acc"))
    pci.cost_infos.append(JointJerkTermInfo(coeffs=[0.5] * nj, targets=[0.0] * nj, first_step=0, last_step=pci.basic_info.n_steps - 1, name="jerk"))
desc = pci.to_desc()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
full = len(sys.argv) > 2 and sys.argv[2] == "full"
x0 = configs.seeds_for(cid, pci, s, g, B, **({"sigma": 0.05} if cid in (3, 4) else {}))
if bp_name is not None:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import test_band_pair_chain as bp
    from trajopt_amd.problem import JointAccTermInfo, JointJerkTermInfo
    for k in (bp.SWITCH, "TMX_DENSE_QP_MAX_N"):
        os.environ.pop(k, None)
    import test_band_row_pair_chain as br  # ("P1", "P2", ...: acceleration / jerk ROWS next to pair rows)
    os.environ.pop(br.SWITCH, None)
    if bp_name.split("-")[0] in br.ALL:
        os.environ[br.SWITCH] = "1"
    pci, x0 = (br.ALL if bp_name.split("-")[0] in br.ALL else bp.ALL)[bp_name.split("-")[0]](B)
    if bp_name.endswith("-nocost"):
        pci.cost_infos = [ti for ti in pci.cost_infos if not isinstance(ti, (JointAccTermInfo, JointJerkTermInfo))]
    desc = pci.to_desc()
    cid = 0
    print("problem", bp_name, "of tests/test_band_pair_chain.py")
ctx = runtime.Context(0, sys.argv[3] if len(sys.argv) > 3 else None)
ctx.upload(desc, abi.default_sqp_params(), configs.osqp_settings_config4() if cid == 4 else abi.default_osqp_settings())
ctx.set_x0(x0)
ctx.kernel_stats(reset=True)
if full:
    ctx.run(0)
    c = ctx.counters()
    iters, nqp = c["admm_iters"], c["n_qp_solves"]
else:
    ctx.convexify()
    ctx.kernel_stats(reset=True)
    xq, cvx, rec = ctx.qp_solve()
    iters, nqp = sum(rec[b].osqp_iter for b in range(B)), B
st = ctx.kernel_stats()
out = (C.c_longlong * 16)()
ctx.lib.tmx_debug_phase_cycles.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
ctx.lib.tmx_debug_phase_cycles(ctx.h, out)
names = ["setup", "WALL(10ns)", "ADMM loop | generic: phase A", "check_term | generic: phase B", "convexify_terms | generic: chain", "generic: phase C", "residuals+rho", "polish", "burst entry", "burst exit",
         "store", "qp_structure", "eval+update", "f:assemble", "f:G inverses", "f:Schur+Zs"]
# -DTMX_PROFILE -DTMX_FINE=5 builds (pass "fine5" as the last argument): the SQP shell around the QP solve split over the reused slots.
# As with TMX_FINE=1, the reused slots keep their own phases: subtract the rows of a plain -DTMX_PROFILE run of the same commit.
if fine5:
    names[11], names[12] = "qp_structure: P hashes + reduction", "eval+update: decision + log + accept copy"
    # (on a problem of DevProblem::eval_fast slot 13 holds the merged pass of tmx_eval.h, exact evaluation and model values, and slot 14
    #  only its own phase "f:G inverses")
    names[13], names[14] = "f:assemble + eval+update: exact evaluation (eval_fast: + model values)", "f:G inverses + eval+update: model values"
    names[15], names[6] = "f:Schur+Zs + qp_structure: prefix counts + column pointers", "residuals+rho + qp_structure: hashing walks of A"
# -DTMX_PROFILE -DTMX_FINE=2 builds (the word "fine2" anywhere among the arguments): the in-register check of the epoch-resident burst split
# over reused slots - they keep their own phases too, so subtract the rows of a plain -DTMX_PROFILE run of the same commit.  Slot 9
# keeps the re-zeroing and the decision of every check (and the store at the burst's end), slot 4 is free on the fast path.
if fine2:
    names[13], names[14], names[15] = "f:assemble + check: publish", "f:G inverses + check: reciprocals + 14 norms", "f:Schur+Zs + check: certificates"
    names[6], names[4], names[9] = "residuals+rho + check: reduction", "burst: reload of the matrix rows", "check: re-zeroing + decision, burst exit"
out = list(out)
# Slot 5 is a phase TIME only on the generic path ("phase C").  On the dense fast path (config 1 without smoothing costs) the
# epoch-resident burst uses it as a COUNTER (tmx_part.h: pc[5] += 1 + (go_on << 20) per in-register check): decode it and keep it
# out of the cycle totals - rounds 2 / 3 printed it as 1.18 G "cycles" per problem (83 % of a total that then meant nothing).
fast_path = (cid == 1 and not smooth and not ctx.workspace_in_hbm())
if fast_path:
    # (summed over the batch the low field overflows into the high one: every continued check is a check, so the smallest
    #  carry count k with checks >= continued recovers both)
    n_cont = out[5] >> 20
    n_checks = out[5] - (n_cont << 20)
    while n_checks < n_cont:
        n_checks += 1 << 20
        n_cont -= 1
    print(f"in-register checks of the epoch-resident burst: {n_checks / B:.1f} per problem, {n_cont / B:.1f} of them continued without leaving the burst")
    out[5] = 0
tot = sum(out)
print("B", B, "kernel ms", st["admm_ms"], "admm iters", iters, "qp solves", nqp, "iters/qp", iters / nqp)
for n, c in zip(names, out):
    if c:
        print(f"  {n:12s} {c / B:14.0f} cycles/problem  {100.0 * c / tot:5.1f}%   per-iter {c / max(1, iters):9.1f}   per-qp {c / nqp:10.0f}")
wall = out[1]; tot -= wall
# in-step wall time (100 MHz constant-rate counter) against the sum of the phase cycles (shader clock): their ratio is the
# effective shader clock, and the rows above sum to wall x clock by construction of the ticks
print("  wall-clock per problem (ms)", wall / B * 1e-5, " => effective shader clock (GHz)", tot / max(1, wall) / 10.0)
print("  total cycles/problem", tot / B, " => per ADMM iteration (all phases)", tot / iters)
if hasattr(ctx.lib, "tmx_debug_pspk"):
    # segmented sweeps of the dense-coupling chain (pair-row problems): thread-0 cycles of their three parts, per sweep
    sp = (C.c_longlong * 8)()
    ctx.lib.tmx_debug_pspk.argtypes = [C.POINTER(C.c_longlong)]
    if ctx.lib.tmx_debug_pspk(sp) == 0 and sp[3] > 0:
        n = sp[3]
        print(f"  segmented sweeps: {n} sweeps; cycles per sweep: local sweeps {sp[0] / n:.0f}, boundary vectors {sp[1] / n:.0f}, spike correction {sp[2] / n:.0f}"
              f"  (two sweeps per ADMM iteration: {2 * (sp[0] + sp[1] + sp[2]) / n:.0f} cycles)")

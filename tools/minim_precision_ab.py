"""Same-process A/B of the minimization's storage precision of R = A S: the default f64 R against
-msplit_minimization_precision single (R stored as float, every sum f64), on the bench's SMSM block (one
512 x 512 x 256 z-slab, s = 20, configs[2]'s options), the two modes interleaved A/B/A/B in one process.

Per mode one JSON line:
  lsqr            ms per LSQR step and per solve of the block's outer LSQR on the R of a first outer iteration
                  (median of --rounds solves, host clock around a solve that ends in a device synchronise), and the
                  one-pass kernel's event time and TB/s from the library's per-launch events in a solve of its own
                  (algorithmic bytes over event time: 8 n (s + 3) for double, 4 n s + 8 n 3 for single);
  smsm_outer_ms   ms per SMSM outer iteration (s inner GMRES solves, R = A S, LSQR, x = S alpha), median of --rounds;
  hbm_peak_GB     the device-wide hipMemGetInfo peak while that mode's block alone is set up and runs one outer
                  iteration (each mode's block is built, measured and freed in turn for this figure).
single's line also carries its figures relative to double's.

--amam adds, per mode, one interior rank of the 8-block configs[3] run (1024 x 1024 x 128 rows, the replicated R of
all 8 row blocks filled on the device from its own rows, one broadcast slot set by the production rule): peak HBM and
the minimization time of one outer iteration.  The two modes run one after the other there: both do not fit together.

  python tools/minim_precision_ab.py [--mesh 512] [--planes 256] [--s 20] [--rounds 5] [--amam] [--out FILE]
There is no CPU fallback.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
import time
import uuid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MODES = ("double", "single")


def smsm_options(args, mode):
    return (f"-inner1_ksp_type gmres -inner1_ksp_gmres_restart 30 -inner1_ksp_atol 1e-100 "
            f"-inner1_ksp_max_it {args.inner_max_it} -inner1_ksp_rtol 1e-20 -inner1_pc_type none "
            f"-inner1_ksp_norm_type UNPRECONDITIONED "
            f"-outer1_ksp_type lsqr -outer1_ksp_convergence_test default -outer1_ksp_lsqr_exact_mat_norm "
            f"-outer1_ksp_atol 1e-100 -outer1_ksp_max_it {args.outer_max_it} -outer1_ksp_rtol 1e-15 "
            f"-outer1_pc_type none -outer1_ksp_norm_type UNPRECONDITIONED -s {args.s} "
            f"-msplit_minimization_precision {mode}")


class SmsmBlock:
    """The bench's per-GPU SMSM block (bench.py build_smsm) with R in the given precision."""

    def __init__(self, ctx, args, mode):
        from medane_tchakorom_ufc_thesis_repository_amd.comm import LocalComm
        from medane_tchakorom_ufc_thesis_repository_amd.multisplitting import GpuBlock, GpuMinimizer
        from medane_tchakorom_ufc_thesis_repository_amd.petsc import Options
        from medane_tchakorom_ufc_thesis_repository_amd.utils import block_layout
        self.ctx, self.s, self.comm = ctx, args.s, LocalComm()
        o = Options(smsm_options(args, mode))
        L = block_layout(3, args.mesh, args.mesh, args.planes, 1, 0, None)
        self.blk = GpuBlock(ctx, L, o, self.comm, prefix="inner1_")
        self.blk.setup_minimization(args.s)
        assert self.blk.R.get_precision() == mode and self.blk.S.get_precision() == "double"
        self.mini = GpuMinimizer(ctx, [self.blk], self.comm, o, prefix="outer1_")
        self.blk.reset_halo()
        self.rows = L.nrows

    def inner(self):
        for k in range(self.s):
            self.blk.update_rhs()
            self.blk.solve()
            self.comm.exchange([self.blk])
            self.blk.store_column(k)
        self.blk.form_R()

    def lsqr(self):
        """One outer LSQR solve on the current R; (seconds, LSQR steps)."""
        self.ctx.synchronize()
        t0 = time.perf_counter()
        self.mini.lsqr.solve([self.blk.b], self.mini.alpha)
        self.ctx.synchronize()
        return time.perf_counter() - t0, self.mini.lsqr.get_iteration_number()

    def outer(self):
        self.ctx.synchronize()
        t0 = time.perf_counter()
        self.inner()
        self.mini.solve([self.blk])
        self.ctx.synchronize()
        return time.perf_counter() - t0

    def close(self):
        self.mini.close()


def hbm_peak(ctx, args, mode):
    from amam_configs import HbmSampler
    hbm = HbmSampler()
    b = SmsmBlock(ctx, args, mode)
    b.outer()
    mem = hbm.stop()
    b.close()
    del b
    gc.collect()
    ctx.synchronize()
    return mem


def amam_rank(args, mode):
    """tools/amam_configs.py footprint (lsqr) with R, and the replicated R, in the given precision."""
    from amam_configs import HbmSampler, options
    from medane_tchakorom_ufc_thesis_repository_amd.comm import LocalComm
    from medane_tchakorom_ufc_thesis_repository_amd.multisplitting import GpuBlock
    from medane_tchakorom_ufc_thesis_repository_amd.petsc import AsyncBroadcast, Context, Options
    from medane_tchakorom_ufc_thesis_repository_amd.utils import block_layout
    nb, rank, n = 8, 3, 1024
    ctx = Context(0)
    hbm = HbmSampler()
    opts = Options(options(nb, args.s, args.inner_max_it, "lsqr") + f" -msplit_minimization_precision {mode}")
    blk = GpuBlock(ctx, block_layout(3, n, n, n, nb, rank, None), opts, LocalComm())
    blk.setup_global_async_minimization(args.s)
    assert all(R.get_precision() == mode for R in blk.R_rep)
    bc = AsyncBroadcast(f"/msplit_mp_{os.getpid()}_{uuid.uuid4().hex[:8]}_R", nb, rank, blk.bcast_cap(), True)
    nbuf = bc.enable_device(ctx, 0)
    blk.reset_halo()
    for k in range(args.s):
        blk.update_rhs()
        blk.solve()
        blk.store_column(k)
    for j, R in enumerate(blk.R_rep):                  # the peers' rows of R: this block's own product, on the device
        if j != rank:
            blk.A_ext.mat_mult_dense(blk.S, R)
    ctx.synchronize()
    t0 = time.perf_counter()
    rn, lits, reason = blk.global_async_minimize(bc)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    mem = hbm.stop()
    bc.close_peers()
    bc.destroy()
    out = {"tool": "minim_precision_ab", "what": "configs[3] rank (block 3 of 8 of 1024^3)", "s": args.s,
           "minimization_precision": mode, "nbuf": nbuf, "minimize_s": dt, "lsqr_its": lits, "lsqr_reason": reason,
           "lsqr_rnorm": rn, "hbm": mem,
           "replicated_R_GB": 8 * blk.R.shape[0] * args.s * (4 if mode == "single" else 8) / 1e9}
    del blk, bc
    gc.collect()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=512)
    ap.add_argument("--planes", type=int, default=256)
    ap.add_argument("--s", type=int, default=20)
    ap.add_argument("--inner-max-it", type=int, default=20)
    ap.add_argument("--outer-max-it", type=int, default=70)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--amam", action="store_true", help="also the configs[3] rank, one mode after the other")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    from medane_tchakorom_ufc_thesis_repository_amd.petsc import Context, device_count
    if device_count() == 0:
        raise SystemExit("minim_precision_ab.py: no GPU visible; this measurement has no CPU fallback")
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    peaks = {mode: hbm_peak(ctx, args, mode) for mode in MODES}      # each mode's block alone
    B = {mode: SmsmBlock(ctx, args, mode) for mode in MODES}
    for mode in MODES:                                               # a first outer iteration: S, R and x of step 1
        B[mode].outer()
        B[mode].inner()                                              # the R the timed LSQR solves read
    for _ in range(args.warmup):
        for mode in MODES:
            B[mode].lsqr()
    lsqr_dt = {mode: [] for mode in MODES}
    lsqr_its = {}
    for _ in range(args.rounds):
        for mode in MODES:                                           # interleaved: A B A B ...
            dt, its = B[mode].lsqr()
            lsqr_dt[mode].append(dt)
            lsqr_its[mode] = its
    outer_dt = {mode: [] for mode in MODES}
    for _ in range(args.rounds):
        for mode in MODES:
            outer_dt[mode].append(B[mode].outer())
    rec = {}
    for mode in MODES:
        B[mode].inner()
        ctx.set_timing(True, 1)                                      # per-launch events: a solve of its own
        ctx.reset_kernel_stats()
        B[mode].lsqr()
        st = ctx.kernel_stats()
        ctx.set_timing(False)
        n, s = B[mode].rows, args.s
        step_bytes = n * ((4 if mode == "single" else 8) * s + 8 * 3)
        ms_solve = 1e3 * float(np.median(lsqr_dt[mode]))
        rec[mode] = {
            "tool": "minim_precision_ab", "block": f"{args.mesh}x{args.mesh}x{args.planes}", "rows": n, "s": s,
            "minimization_precision": mode,
            "lsqr": {"its": lsqr_its[mode], "ms_per_solve": ms_solve, "ms_per_step": ms_solve / max(lsqr_its[mode], 1),
                     "ms_min": 1e3 * min(lsqr_dt[mode]), "ms_max": 1e3 * max(lsqr_dt[mode]),
                     "alg_bytes_per_step": step_bytes,
                     "TB_per_s_host_clock": step_bytes * lsqr_its[mode] / (ms_solve * 1e-3) / 1e12,
                     "kernels": {name: {"launches": k["launches"], "ms": k["ms"],
                                        "ms_per_launch": k["ms"] / k["launches"],
                                        "TB_per_s": k["bytes"] / (k["ms"] * 1e-3) / 1e12}
                                 for name, k in st.items() if k["launches"] and k["ms"] > 0}},
            "smsm_outer_ms": 1e3 * float(np.median(outer_dt[mode])),
            "smsm_outer_ms_min": 1e3 * min(outer_dt[mode]), "smsm_outer_ms_max": 1e3 * max(outer_dt[mode]),
            "rounds": args.rounds, "hbm_peak_GB": peaks[mode]["peak_GB"],
            "hbm_before_GB": peaks[mode]["before_GB"],
        }
    d, sg = rec["double"], rec["single"]
    sg["vs_double"] = {"lsqr_ms_per_step": sg["lsqr"]["ms_per_step"] / d["lsqr"]["ms_per_step"],
                       "smsm_outer_ms": sg["smsm_outer_ms"] / d["smsm_outer_ms"]}
    for mode in MODES:
        emit(rec[mode])
        B[mode].close()
    del B
    gc.collect()
    if args.amam:
        for mode in MODES:
            emit(amam_rank(args, mode))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

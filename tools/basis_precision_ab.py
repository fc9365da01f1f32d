"""Same-process A/B of the Krylov basis precision on the flagship step (configs[1]: 3D 7-pt Poisson 256^3, GMRES(30),
pc none, 300 iterations per solve from x0 = 0): the default f64 basis against -msplit_basis_precision single and
block16, on the same operator and right-hand side, interleaved A/B/C/A/B/C, for each matrix storage asked for (dv,
csr).

Per mode one JSON line: ms_per_step (median of --rounds timed solves, host clock around a solve that ends in a device
synchronise, after --warmup untimed solves of that mode; graphs on, timing off), the true ||b - A x|| / ||b|| after
the step (f64 MatResidual and norms on the device), and per kernel class the TB/s of a separate solve with the
library's per-launch events on (algorithmic bytes over event time; that solve runs eagerly, so its sum is not the
step time) and every timed solve (ms_rounds: the spread).  Every line but double's also carries ms_per_step relative
to double's, and block16's relative to single's.

  python tools/basis_precision_ab.py [--mesh 256] [--storages dv,csr] [--modes double,single,block16] [--rounds 7]
                                     [--warmup 2] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL_MODES = ("double", "single", "block16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=256)
    ap.add_argument("--storages", default="dv,csr")
    ap.add_argument("--modes", default=",".join(ALL_MODES))
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--max-it", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    MODES = tuple(args.modes.split(","))
    if not MODES or any(m not in ALL_MODES for m in MODES):
        raise SystemExit(f"basis_precision_ab.py: --modes takes words of {ALL_MODES}")
    import numpy as np
    import torch
    from medane_tchakorom_ufc_thesis_repository_amd.petsc import KSP, Context, Mat, Options, Vec, device_count
    if device_count() == 0:
        raise SystemExit("basis_precision_ab.py: no GPU visible; this measurement has no CPU fallback")
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    n = args.mesh
    rows = n * n * n
    lines = []
    for storage in args.storages.split(","):
        A = Mat.box_convdiff(ctx, 3, n, n, n, False, False, (0.0, 0.0, 0.0))
        A.set_storage(storage)
        ones = Vec(ctx, rows)
        ones.set(1.0)
        b = Vec(ctx, rows)
        A.mult(ones, b)
        bnorm = b.norm()
        x, r = Vec(ctx, rows), Vec(ctx, rows)
        ksp = {}
        for mode in MODES:
            k = KSP(ctx)
            k.set_operators(A)
            k.set_from_options(Options(f"-ksp_type gmres -ksp_gmres_restart {args.restart} -pc_type none "
                                       f"-ksp_norm_type unpreconditioned -ksp_rtol 1e-30 -ksp_max_it {args.max_it} "
                                       f"-msplit_basis_precision {mode}"))
            k.set_up()
            ksp[mode] = k

        def solve(mode):
            ctx.synchronize()
            t0 = time.perf_counter()
            ksp[mode].solve(b, x)
            ctx.synchronize()
            return time.perf_counter() - t0

        for mode in MODES:
            for _ in range(args.warmup):
                solve(mode)
        dts = {mode: [] for mode in MODES}
        for _ in range(args.rounds):
            for mode in MODES:            # interleaved: A B C A B C ...
                dts[mode].append(solve(mode))
        rec = {}
        for mode in MODES:
            solve(mode)
            its = ksp[mode].get_iteration_number()
            A.residual(b, x, r)
            true = r.norm() / bnorm
            ctx.set_timing(True, 1)       # per-launch events: eager launches, a run of its own
            ctx.reset_kernel_stats()
            ksp[mode].solve(b, x)
            ctx.synchronize()
            st = ctx.kernel_stats()
            ctx.set_timing(False)
            ms = 1e3 * float(np.median(dts[mode]))
            rec[mode] = {
                "tool": "basis_precision_ab", "mesh": n, "storage": A.get_storage(), "spmv_kernel": A.spmv_kernel(),
                "restart": args.restart, "its": its, "basis_precision": mode, "ms_per_step": ms,
                "ms_min": 1e3 * min(dts[mode]), "ms_max": 1e3 * max(dts[mode]), "rounds": args.rounds,
                "ms_rounds": [1e3 * t for t in dts[mode]],
                "dof_updates_per_s": rows * its / (ms * 1e-3), "true_residual_rel": true,
                "work_bytes": ksp[mode].get_work_bytes(),
                "kernels": {name: {"launches": s["launches"], "ms": s["ms"], "bytes_per_row_per_it": s["bytes"] / rows / its,
                                   "TB_per_s": s["bytes"] / (s["ms"] * 1e-3) / 1e12}
                            for name, s in st.items() if s["launches"] and s["ms"] > 0},
            }
        for mode, base in (("single", "double"), ("block16", "double"), ("block16", "single")):
            if mode in rec and base in rec:
                rec[mode][f"ms_per_step_vs_{base}"] = rec[mode]["ms_per_step"] / rec[base]["ms_per_step"]
        for mode in MODES:
            lines.append(json.dumps(rec[mode]))
            print(lines[-1], flush=True)
        for k in ksp.values():
            k.destroy()
        del A, b, x, r, ones
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Same-process measurement of KSPCG (-msplit_ksp_type cg) next to GMRES(30) on two symmetric positive definite
operators: the --mesh^3 Poisson box (DV storage, PCNONE) and the --mesh^3 variable-coefficient diffusion operator
(Mat.box_diffusion, STENCIL storage, -pc_type none and jacobi).  Every solve runs --max-it iterations at rtol 1e-30
from x0 = 0 on b = A 1; the modes of one operator are interleaved, --rounds timed solves each after --warmup untimed
ones (host clock around a solve that ends in a device synchronise; graphs on, timing off).

Per mode one JSON line: ms_per_iteration (mean over the rounds) with every round, the spread (max - min) and the
KSP's work bytes.  "cg" takes the library's own route (k_cg_aypx, then the operator's fused MatMult + self-dot); "cg_march" forces
the AYPX folded into the chunk-tile march (k_box_cg_march, DV boxes), "cg_two_kernels" AYPX, MatMult and dot as three
kernels (the route hook mspi_ksp_cg_set_route).  One more line gives k_cg_update's rate on that box: --reps launches of
mspi_cg_update (a = 0, so the vectors keep their values) between two synchronises, 6 x 8n bytes per launch (x, p, r, w
read, x and r written; 7 x 8n with dinv), and a last one the work bytes of both types on a --mem-box block
(set-up only, nothing solved).

  python tools/cg_measure.py [--mesh 256] [--max-it 300] [--rounds 3] [--warmup 1] [--mem-box 512,512,256] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=256)
    ap.add_argument("--max-it", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--mem-box", default="512,512,256")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    from medane_tchakorom_ufc_thesis_repository_amd import _lib
    from medane_tchakorom_ufc_thesis_repository_amd.petsc import KSP, Context, Mat, Options, Vec, device_count
    if device_count() == 0:
        raise SystemExit("cg_measure.py: no GPU visible; this measurement has no CPU fallback")
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    n = args.mesh
    rows = n * n * n
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def make_ksp(A, mode, pc):
        k = KSP(ctx)
        k.set_operators(A)
        route = {"cg_two_kernels": 0, "cg_march": 2}.get(mode, -1)
        assert L.mspi_ksp_cg_set_route(k.h, route) == 0
        k.set_from_options(Options(f"-msplit_ksp_type {'gmres' if mode == 'gmres' else 'cg'} -ksp_gmres_restart 30 "
                                   f"-pc_type {pc} -ksp_rtol 1e-30 -ksp_max_it {args.max_it}"))
        k.set_up()
        return k

    def measure(A, name, modes):
        ones, b, x = (Vec(ctx, rows) for _ in range(3))
        ones.set(1.0)
        A.mult(ones, b)
        ksp = {m: make_ksp(A, *m) for m in modes}

        def solve(m):
            ctx.synchronize()
            t0 = time.perf_counter()
            ksp[m].solve(b, x)
            ctx.synchronize()
            return time.perf_counter() - t0

        for m in modes:
            for _ in range(args.warmup):
                solve(m)
        dts = {m: [] for m in modes}
        for _ in range(args.rounds):
            for m in modes:              # interleaved: A B C A B C ...
                dts[m].append(solve(m))
        for m in modes:
            its = ksp[m].get_iteration_number()
            per = [1e3 * t / its for t in dts[m]]
            emit({"tool": "cg_measure", "operator": name, "mesh": n, "storage": A.get_storage(),
                  "spmv_kernel": A.spmv_kernel(), "mode": m[0], "pc_type": m[1], "its": its,
                  "reason": ksp[m].get_converged_reason(), "ms_per_iteration": float(np.mean(per)),
                  "ms_per_iteration_rounds": per, "spread_ms": max(per) - min(per),
                  "work_bytes": ksp[m].get_work_bytes()})
            ksp[m].destroy()

    L = _lib.load()
    vp = C.c_void_p
    L.mspi_ksp_cg_set_route.argtypes = [vp, C.c_int]
    A = Mat.box_stencil(ctx, 3, n, n, n)
    measure(A, "poisson", [("gmres", "none"), ("cg", "none"), ("cg_march", "none"), ("cg_two_kernels", "none")])

    # k_cg_update alone, on the same box
    L.mspi_cg_update.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int64, vp]
    L.mspi_reserve_partial.argtypes = [vp, C.c_int64]
    vecs = [Vec(ctx, rows) for _ in range(5)]
    for v in vecs:
        v.set(1.0)
    st = Vec(ctx, 64)                     # a zeroed state block: stop = 0, a = na = 0
    assert L.mspi_reserve_partial(ctx.h, rows) == 0
    for dinv in (None, vecs[4]):
        def launch():
            rc = L.mspi_cg_update(ctx.h, vecs[0].device_ptr(), vecs[1].device_ptr(), vecs[2].device_ptr(),
                                  vecs[3].device_ptr(), dinv.device_ptr() if dinv else None, 0, rows, st.device_ptr())
            assert rc == 0
        for _ in range(5):
            launch()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            launch()
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / args.reps
        nb = 8.0 * rows * (7 if dinv else 6)
        emit({"tool": "cg_measure", "kernel": "k_cg_update", "jacobi": dinv is not None, "mesh": n,
              "ms_per_launch": 1e3 * dt, "bytes_per_launch": nb, "TB_per_s": nb / dt / 1e12, "reps": args.reps})
    del vecs, A

    kap = Vec(ctx, rows)
    kap.set_cell_coefficients(0, 9)
    A = Mat.box_diffusion(ctx, 3, n, n, n, False, False, kap)
    measure(A, "box_diffusion", [("gmres", "none"), ("cg", "none"), ("gmres", "jacobi"), ("cg", "jacobi")])
    del A, kap

    bx, by, bz = (int(v) for v in args.mem_box.split(","))
    A = Mat.box_stencil(ctx, 3, bx, by, bz)
    for mode in ("gmres", "cg"):
        k = KSP(ctx)
        k.set_operators(A)
        k.set_from_options(Options(f"-msplit_ksp_type {mode} -ksp_gmres_restart 30"))
        k.set_up()
        emit({"tool": "cg_measure", "memory": mode, "box": [bx, by, bz], "work_bytes_after_set_up": k.get_work_bytes(),
              "note": "a forced march route allocates a fourth vector (p's second buffer) at its first solve"})
        k.destroy()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

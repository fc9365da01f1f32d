"""Measurements of the device-assembled diffusion operator (Mat.box_diffusion), one JSON line each; the numbers
and commands of profiles/box_diffusion/README.md.  There is no CPU fallback.

  python tools/box_diffusion_measure.py assembly [--mesh 256] [--reps 5]
      The whole mesh^3 box by two routes, each timed from the call to the first completed MatMult (host clock
      around a device synchronise), median of --reps in one process, with the process's peak host RSS after each
      route (resource.getrusage; the device route runs first, since the peak only grows):
        device  Vec.set_cell_coefficients + Mat.box_diffusion
        host    utils.heterogeneous_poisson3d + Mat.from_csr
      then the kernel each matrix reports and one GMRES(30) cycle (30 steps) on each, alternating, median of --reps.

  python tools/box_diffusion_measure.py smsm [--kappa-seed S] [--its 3]
      One SMSM-global outer iteration on a 512 x 512 x 256 block (s = 20, the options of tools/smsm_phase_times.py):
      the Poisson block, or with --kappa-seed the diffusion block; phase times in ms.
"""
import argparse
import json
import os
import resource
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["assembly", "smsm"])
ap.add_argument("--mesh", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--kappa-seed", type=int, default=None)
ap.add_argument("--its", type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from medane_tchakorom_ufc_thesis_repository_amd.comm import LocalComm  # noqa: E402
from medane_tchakorom_ufc_thesis_repository_amd.multisplitting import GpuBlock, GpuMinimizer  # noqa: E402
from medane_tchakorom_ufc_thesis_repository_amd.petsc import KSP, Context, Mat, Options, Vec, device_count  # noqa: E402
from medane_tchakorom_ufc_thesis_repository_amd.utils import block_layout, heterogeneous_poisson3d  # noqa: E402

if device_count() == 0:
    raise SystemExit("box_diffusion_measure.py: no GPU visible; this measurement has no CPU fallback")
ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
SEED = 20251121


def tick():
    ctx.synchronize()
    return time.perf_counter()


def peak_rss_mib():
    return round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, 1)


def assembly():
    n = args.mesh
    N = n ** 3
    x, y = Vec(ctx, N), Vec(ctx, N)
    x.set(1.0)

    def device_route():
        kap = Vec(ctx, N)
        kap.set_cell_coefficients(0, SEED)
        A = Mat.box_diffusion(ctx, 3, n, n, n, False, False, kap)
        A.mult(x, y)
        return A

    def host_route():
        A = Mat.from_csr(ctx, N, N, *heterogeneous_poisson3d(n))
        A.mult(x, y)
        return A

    out = {"mesh": n, "rss_mib_at_start": peak_rss_mib()}
    mats = {}
    for name, route in (("device", device_route), ("host", host_route)):
        times = []
        for _ in range(args.reps):
            mats.pop(name, None)
            t0 = tick()
            mats[name] = route()
            times.append(tick() - t0)
            print(f"{name} route: {times[-1]:.3f} s", file=sys.stderr, flush=True)
        out[name] = {"seconds": [round(t, 4) for t in times], "median_s": round(statistics.median(times), 4),
                     "peak_rss_mib": peak_rss_mib(), "kernel": mats[name].spmv_kernel(),
                     "storage": mats[name].get_storage()}
    ksps = {}
    b = Vec(ctx, N)
    mats["device"].mult(x, b)
    for name, A in mats.items():
        k = KSP(ctx)
        k.set_operators(A)
        k.set_from_options(Options("-ksp_type gmres -pc_type none -ksp_gmres_restart 30 -ksp_max_it 30 -ksp_rtol 1e-30"))
        ksps[name] = k
    sol = Vec(ctx, N)
    cyc = {name: [] for name in ksps}
    for rep in range(args.reps + 1):                      # the first pass warms both up
        for name, k in ksps.items():
            sol.set(0.0)
            t0 = tick()
            k.solve(b, sol)
            t = tick() - t0
            if rep:
                cyc[name].append(t)
    for name in cyc:
        out[name]["gmres30_cycle_ms"] = [round(1e3 * t, 3) for t in cyc[name]]
        out[name]["gmres30_step_ms_median"] = round(1e3 * statistics.median(cyc[name]) / 30, 4)
    print(json.dumps(out))


def smsm():
    s = 20
    o = Options("-inner1_ksp_type gmres -inner1_ksp_gmres_restart 30 -inner1_ksp_atol 1e-100 -inner1_ksp_max_it 20 "
                "-inner1_ksp_rtol 1e-20 -inner1_pc_type none -inner1_ksp_norm_type UNPRECONDITIONED -outer1_ksp_type "
                "lsqr -outer1_ksp_convergence_test default -outer1_ksp_lsqr_exact_mat_norm -outer1_ksp_atol 1e-100 "
                "-outer1_ksp_max_it 70 -outer1_ksp_rtol 1e-15 -outer1_pc_type none -outer1_ksp_norm_type "
                "UNPRECONDITIONED -s 20")
    comm = LocalComm()
    t0 = tick()
    blk = GpuBlock(ctx, block_layout(3, 512, 512, 256, 1, 0, None, args.kappa_seed), o, comm, prefix="inner1_")
    setup = tick() - t0
    blk.setup_minimization(s)
    mini = GpuMinimizer(ctx, [blk], comm, o, prefix="outer1_")
    blk.reset_halo()
    T = {"inner": [], "form_R": [], "lsqr": [], "apply": [], "total": []}
    for it in range(1 + args.its):
        t0 = tick()
        for k in range(s):
            blk.update_rhs()
            blk.solve()
            comm.exchange([blk])
            blk.store_column(k)
        t1 = tick()
        blk.form_R()
        t2 = tick()
        mini.lsqr.solve([blk.b], mini.alpha)
        t3 = tick()
        blk.apply_alpha(mini.alpha)
        t4 = tick()
        if it:
            for k, v in zip(T, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
                T[k].append(round(1e3 * v, 3))
    mini.close()
    print(json.dumps({"operator": "poisson" if args.kappa_seed is None else f"diffusion seed {args.kappa_seed}",
                      "kernel": blk.A.spmv_kernel(), "block_setup_s": round(setup, 3),
                      "peak_rss_mib": peak_rss_mib(), **T}))


assembly() if args.mode == "assembly" else smsm()

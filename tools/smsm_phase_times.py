"""Phase times of the bench's SMSM block (512 x 512 x 256, s = 20, configs[2]'s options, default precision): the s
inner solves, R = A S, the outer LSQR solve and x = S alpha of each outer iteration, a device synchronise between
them, one JSON line (ms; --its timed outer iterations after one warm-up).

  python tools/smsm_phase_times.py [TREE] [--label NAME] [--its 3]

TREE is the root of the checkout whose package and library are measured (default: this one), so that two builds --
say a parent commit's and a change's -- can be run in fresh processes, alternating, from one place.  There is no CPU
fallback.
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("tree", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default=None)
ap.add_argument("--its", type=int, default=3)
args = ap.parse_args()
root = os.path.abspath(args.tree)
sys.path.insert(0, root)

import torch  # noqa: E402

import medane_tchakorom_ufc_thesis_repository_amd as pkg  # noqa: E402
from medane_tchakorom_ufc_thesis_repository_amd.comm import LocalComm  # noqa: E402
from medane_tchakorom_ufc_thesis_repository_amd.multisplitting import GpuBlock, GpuMinimizer  # noqa: E402
from medane_tchakorom_ufc_thesis_repository_amd.petsc import Context, Options, device_count  # noqa: E402
from medane_tchakorom_ufc_thesis_repository_amd.utils import block_layout  # noqa: E402

assert os.path.abspath(pkg.__file__).startswith(root + os.sep), pkg.__file__
if device_count() == 0:
    raise SystemExit("smsm_phase_times.py: no GPU visible; this measurement has no CPU fallback")
s = 20
o = Options("-inner1_ksp_type gmres -inner1_ksp_gmres_restart 30 -inner1_ksp_atol 1e-100 -inner1_ksp_max_it 20 "
            "-inner1_ksp_rtol 1e-20 -inner1_pc_type none -inner1_ksp_norm_type UNPRECONDITIONED -outer1_ksp_type lsqr "
            "-outer1_ksp_convergence_test default -outer1_ksp_lsqr_exact_mat_norm -outer1_ksp_atol 1e-100 "
            "-outer1_ksp_max_it 70 -outer1_ksp_rtol 1e-15 -outer1_pc_type none -outer1_ksp_norm_type UNPRECONDITIONED "
            "-s 20")
ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
comm = LocalComm()
blk = GpuBlock(ctx, block_layout(3, 512, 512, 256, 1, 0, None), o, comm, prefix="inner1_")
blk.setup_minimization(s)
mini = GpuMinimizer(ctx, [blk], comm, o, prefix="outer1_")
blk.reset_halo()
T = {"inner": [], "form_R": [], "lsqr": [], "apply": [], "total": []}


def tick():
    ctx.synchronize()
    return time.perf_counter()


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
print(json.dumps({"tree": args.label or args.tree, **T}))

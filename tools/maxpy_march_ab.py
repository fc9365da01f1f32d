"""Same-process A/B of the W-free CGS MAXPY (k_box_maxpy_march) per basis size nv, against its yardsticks.

One process, one allocation: the Poisson operator of a box in DV storage and a basis of --restart + 1 vectors laid
out as msp_ksp_set_up lays it out (stride = n rounded up to 512 doubles, the recurrence block behind the state).  A
real Arnoldi cycle fills the basis once (the step's own launchers, one call at a time); the recurrence block is
saved before every step and put back before every timed launch, so each repetition runs exactly the solve's step
`it = nv - 1` on the solve's data.  For every nv the forms alternate, --reps timed repetitions each after --warmup
untimed ones, each launch bracketed by the library's own HIP events (msp_ctx_set_timing):

  march_pf<k>  mspi_maxpy_norm_update_march with msk_set_maxpy_prefetch(k): 0 the marched kernel as it was, 2 the
               one-plane form with a 4-vector burst, 3 with an 8-vector burst, 1 the launcher's own choice
               (only where the library has the switch)
  stored       mspi_maxpy_norm_update on a stored W: the same streams plus one W read (k_maxpy_chunk)
  spmv_mdot    the fused mspi_spmv_mdot with y = NULL, which precedes every MAXPY form as it does in the solve (so
               each form meets the cache state the solve gives it)

One JSON line per (shape, nv): median, minimum and maximum in microseconds per form, the algorithmic bytes and the
rate they give, and same_bits: whether every MAXPY form left the same ||VV(nv)||^2 and the same VV(nv).

  python tools/maxpy_march_ab.py [--shapes 256x256x256 512x512x256] [--nv 1 .. 30] [--reps 20] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# mspi_gmres_state / mspi_gmres_dev, field for field (csrc/msplit_internal.h)
STATE_INTS = ("stop", "skip_build", "it", "its", "reason", "nhist", "nbuild", "guess_zero", "m", "max_it", "uirnorm",
              "hist_cap")
STATE_DOUBLES = ("res", "rnorm", "rnorm0", "ttol", "gm_rnorm0", "scale", "bnorm", "rtol", "abstol", "divtol",
                 "haptol", "breakdowntol")
DEV_FIELDS = ("st", "hh", "cc", "ss", "grs", "h", "sc", "hist")


class GmresState(C.Structure):
    _fields_ = [(f, C.c_int32) for f in STATE_INTS] + [(f, C.c_double) for f in STATE_DOUBLES]


class GmresDev(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in DEV_FIELDS]


def bind(L):
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    basis = [i, vp, i64, vp]
    sigs = {"mspi_reserve_partial": [vp, i64],
            "mspi_norm2sq": [vp, vp, i64, vp],
            "mspi_gm_cycle_start": [vp, GmresDev, vp],
            "mspi_spmv_mdot": [vp, vp, vp, vp] + basis + [vp, vp],
            "mspi_maxpy_norm_update": [vp, vp, vp] + basis + [i64, GmresDev, i, i, vp],
            "mspi_maxpy_norm_update_march": [vp, vp, vp, vp] + basis + [GmresDev, i, vp],
            "mspi_gm_wfree": [vp]}
    for name, args in sigs.items():
        f = getattr(L, name)
        f.argtypes, f.restype = args, C.c_int
    has_switch = hasattr(L, "msk_set_maxpy_prefetch")
    if has_switch:
        L.msk_set_maxpy_prefetch.argtypes, L.msk_set_maxpy_prefetch.restype = [i], None
        L.msk_get_maxpy_prefetch.restype = i
    return has_switch


def run_shape(ctx, L, shape, args, forms, has_switch, emit):
    import numpy as np
    from medane_tchakorom_ufc_thesis_repository_amd.petsc import Mat, Vec
    nx, ny, nz = shape
    A = Mat.box_stencil(ctx, 3, nx, ny, nz)
    assert A.get_storage() == "dv" and L.mspi_gm_wfree(A.h) == 1, "the W-free step must take this box"
    n, m = A.shape[0], args.restart + 2            # m: two more than the cycle, so that no step ends it
    stride = (n + 511) // 512 * 512
    basis = Vec(ctx, (args.restart + 2) * stride)
    w = Vec(ctx, stride)
    base = basis.device_ptr()
    assert base % 4096 == 0
    # the recurrence block in msp_ksp_set_up's order: state (to 64 bytes), hh, cc, ss, grs, h, sc, hist
    stw = (C.sizeof(GmresState) + 63) // 64 * 8
    m2, hist_cap = m + 2, m + 2
    counts = (("state", stw), ("hh", m2 * (m + 1)), ("cc", m2), ("ss", m2), ("grs", m2), ("h", m2), ("sc", m2),
              ("hist", hist_cap))
    rec = Vec(ctx, sum(c for _, c in counts))
    off, at = 0, {}
    for name, cnt in counts:
        at[name] = off
        off += cnt
    ptr = {k: rec.device_ptr() + 8 * v for k, v in at.items()}
    g = GmresDev(*[ptr[f if f != "st" else "state"] for f in DEV_FIELDS])
    p_stop = ptr["state"] + GmresState.stop.offset
    st = GmresState()
    st.rnorm, st.guess_zero, st.m, st.max_it, st.hist_cap = -1.0, 1, m, 10 ** 6, hist_cap
    st.rtol, st.abstol, st.divtol, st.haptol, st.breakdowntol, st.scale = 1e-30, 1e-50, 1e4, 1e-30, 0.1, 1.0
    img = np.zeros(rec.n)
    img.view(np.uint8)[:C.sizeof(st)] = np.frombuffer(bytes(st), np.uint8)
    rec.set_values(img)
    basis.set_values(np.random.default_rng(20261021).uniform(-1, 1, n))   # VV(0) = b, zero guess
    assert L.mspi_reserve_partial(ctx.h, n) == 0
    assert L.mspi_norm2sq(ctx.h, base, n, ptr["h"]) == 0
    assert L.mspi_gm_cycle_start(ctx.h, g, ptr["h"]) == 0

    def vv(j):
        return base + 8 * j * stride

    def products(it, y):
        return L.mspi_spmv_mdot(A.h, vv(it), ptr["sc"] + 8 * it, w.device_ptr() if y else None, it + 1, base, stride,
                                ptr["sc"], ptr["h"], p_stop)

    def march(it):
        return L.mspi_maxpy_norm_update_march(A.h, vv(it), ptr["sc"] + 8 * it, vv(it + 1), it + 1, base, stride,
                                              ptr["sc"], g, m, p_stop)

    def stored(it):
        return L.mspi_maxpy_norm_update(ctx.h, w.device_ptr(), vv(it + 1), it + 1, base, stride, ptr["sc"], n, g, it,
                                        m, p_stop)

    # the cycle that fills the basis; the block as it stood before every step
    before = []
    for it in range(args.restart):
        ctx.synchronize()
        before.append(rec.get_array())
        assert products(it, False) == 0 and march(it) == 0
    ctx.synchronize()
    state = GmresState.from_buffer_copy(rec.get_array(0, stw).tobytes()[:C.sizeof(GmresState)])
    assert state.it == args.restart and state.stop == 0, (state.it, state.stop, state.reason)

    def timed(call, it, cls):
        ctx.set_timing(True, 1)
        ctx.reset_kernel_stats()
        assert call(it) == 0
        ctx.synchronize()
        s = ctx.kernel_stats()[cls]
        ctx.set_timing(False)
        assert s["launches"] == 1, s
        return 1e3 * s["ms"], s["bytes"]

    def one(form, it):
        """The step `it` on the saved block: the fused products, then the MAXPY form; microseconds of both."""
        rec.set_values(before[it])
        if form == "stored":
            assert products(it, True) == 0
            t_mdot = None
            t, by = timed(stored, it, "maxpy")
        else:
            if has_switch:
                L.msk_set_maxpy_prefetch(int(form[8:]))
            t_mdot, by_mdot = timed(lambda i: products(i, False), it, "spmvdot")
            bytes_["spmv_mdot"] = by_mdot
            t, by = timed(march, it, "maxpy")
        bytes_[form] = by
        ctx.synchronize()
        q = rec.get_array(at["h"] + it + 1, 1).view(np.uint64)[0]
        return t, t_mdot, int(q)

    for nv in args.nv:
        it = nv - 1
        bytes_ = {}
        for _ in range(args.warmup):
            for f in forms:
                one(f, it)
        t = {f: [] for f in forms + ["spmv_mdot"]}
        bits, ref = set(), None
        for rep in range(args.reps):                  # interleaved
            for f in forms:
                a, b, q = one(f, it)
                t[f].append(a)
                if b is not None:
                    t["spmv_mdot"].append(b)
                bits.add(q)
                if nv in (1, 4, 5, 30) and rep == 0:    # the whole vector, once per form, at four group shapes
                    v = basis.get_array((it + 1) * stride, n).view(np.uint64)
                    ref = v if ref is None else ref
                    bits.add(q if np.array_equal(v, ref) else -1)
        row = {"tool": "maxpy_march_ab", "shape": list(shape), "n": n, "nv": nv, "reps": args.reps}
        for f, v in t.items():
            med = float(np.median(v))
            row[f] = {"us": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2), "bytes": bytes_[f],
                      "TB_per_s": round(bytes_[f] / med * 1e-6, 3)}
        row["same_bits"] = len(bits) == 1
        emit(row)
    if has_switch:
        L.msk_set_maxpy_prefetch(args.default_pf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["256x256x256", "512x512x256"])
    ap.add_argument("--nv", type=int, nargs="+", default=list(range(1, 31)))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--prefetch", type=int, nargs="+", default=[0, 2, 3],
                    help="msk_set_maxpy_prefetch values to time (ignored by a library without the switch)")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    assert max(args.nv) <= args.restart <= 30 and min(args.nv) >= 1
    import torch
    from medane_tchakorom_ufc_thesis_repository_amd import _lib
    from medane_tchakorom_ufc_thesis_repository_amd.petsc import Context, device_count
    if device_count() == 0:
        raise SystemExit("maxpy_march_ab.py: no GPU visible; this measurement has no CPU fallback")
    ctx = Context(0, stream=torch.cuda.current_stream().cuda_stream)
    L = _lib.load()
    has_switch = bind(L)
    if has_switch:
        args.default_pf = L.msk_get_maxpy_prefetch()
        forms = ["march_pf%d" % k for k in args.prefetch] + ["stored"]
    else:
        forms = ["march_pf0", "stored"]
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for s in args.shapes:
        run_shape(ctx, L, tuple(int(v) for v in s.split("x")), args, forms, has_switch, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

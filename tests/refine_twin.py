"""A Python KSPGMRES in the DBR order with PETSc's CGS iterative refinement (helper, not a test).

TEST INFRASTRUCTURE ONLY.  It is tests/basis_twin.py's gmres (KSPSolve_GMRES / KSPGMRESCycle, PCNONE, vector work
through pyoracle's Mat.mult, Mat.residual, mdot, maxpy and norm2 in REDUCE_DBR) with the orthogonalisation of
KSPGMRESClassicalGramSchmidtOrthogonalization restated as include/msplit.h states it (msp_ksp_set_cgs_refinement).
With v_j the normalised basis and W = A v_it:

  1. h_j = W . v_j                                   (mdot)
  2. u = W - sum h_j v_j, wnrm = ||u||               (maxpy, norm2)
  3. refine = 1 for "always"; for "ifneeded" refine = (wnrm < hnrm) with hnrm = sqrt(sum_j h_j h_j), summed in
     j order from 0.0; a non-finite wnrm there is KSPCheckNorm inside the orthogonalisation: DIVERGED_NANORINF, the
     column left zero, the loop left, BuildSoln over the earlier columns (what a non-finite h_j does)
  4. if refine: c_j = u . v_j (a non-finite c_j as in 3), u' = u - sum c_j v_j
  5. hh_j = 0.0; hh_j -= -h_j; if refined hh_j -= -c_j; tt = ||u'|| if refined else wnrm; the rest is unchanged.

cgs = "never" is basis_twin.gmres with rnd = identity, statement for statement.
"""
from __future__ import annotations

import numpy as np
import pyoracle as po

CONVERGED_RTOL, CONVERGED_ATOL = 2, 3
DIVERGED_NULL, DIVERGED_ITS, DIVERGED_DTOL, DIVERGED_BREAKDOWN, DIVERGED_NANORINF = -2, -3, -4, -5, -9
MODES = ("never", "ifneeded", "always")


def _bad(v):
    return bool(np.isnan(v) or np.isinf(v))


def gmres(A, b, x0=None, cgs="never", restart=30, max_it=10000, rtol=1e-5, abstol=1e-50, divtol=1e4,
          haptol=1e-30, breakdowntol=0.1, uirnorm=0, guess_nonzero=0, keep_basis=False):
    """Returns (x, {"its", "reason", "rnorm", "hist", "refined"}): refined is the list of per-step decisions (one
    bool per Arnoldi step whose decision was taken); keep_basis adds "basis", the last cycle's normalised vectors."""
    assert cgs in MODES
    D = po.REDUCE_DBR
    f = np.float64
    n = A.shape[0]
    m = restart
    b = np.ascontiguousarray(b, np.float64)
    guess_zero = not guess_nonzero
    orig_guess_zero = guess_zero
    x = np.zeros(n) if (x0 is None or guess_zero) else np.array(x0, np.float64, copy=True)
    st = dict(its=0, reason=0, rnorm=f(-1.0), rnorm0=f(0.0), ttol=f(0.0), gm_rnorm0=f(0.0))
    hist, refined, V = [], [], []

    def converged(nn, rn):
        st["reason"] = 0
        if nn == 0:
            if not orig_guess_zero and not uirnorm:
                sn = f(po.norm2(b, D))
                st["rnorm0"] = rn if sn == 0.0 else sn
            else:
                st["rnorm0"] = rn
            t = f(rtol) * st["rnorm0"]
            st["ttol"] = f(abstol) if t < abstol else t
        if _bad(rn):
            st["reason"] = DIVERGED_NANORINF
        elif rn <= st["ttol"]:
            st["reason"] = CONVERGED_ATOL if rn < abstol else CONVERGED_RTOL
        elif rn >= f(divtol) * st["rnorm0"]:
            st["reason"] = DIVERGED_DTOL

    def scale_of(t):   # VecNormalize, deferred: the factor every reader of the vector multiplies by
        return f(1.0) / t if (t != 0.0 and not _bad(t)) else f(1.0)

    itcount = 0
    with np.errstate(all="ignore"):
        while not st["reason"]:
            r = A.residual(b, x) if not guess_zero else b.copy()   # KSPInitialResidual
            res = f(po.norm2(r, D))
            V = [r * scale_of(res)]
            HH = np.zeros((m + 2, m + 1))
            cc, ss, grs = np.zeros(m + 2), np.zeros(m + 2), np.zeros(m + 2)
            it, hapend, cyc, build = 0, False, 0, False
            if _bad(res):
                st["reason"] = DIVERGED_NANORINF
            elif st["rnorm"] > 0.0 and abs(res - st["rnorm"]) > f(breakdowntol) * st["gm_rnorm0"]:
                st["reason"] = DIVERGED_BREAKDOWN
            else:
                grs[0] = st["gm_rnorm0"] = res
                st["rnorm"] = res
                hist.append(res)
                if res == 0.0:
                    st["reason"] = CONVERGED_ATOL
                else:
                    converged(st["its"], res)
                    build = True
                    while not st["reason"] and it < m and st["its"] < max_it:
                        if it:
                            hist.append(res)
                        w = A.mult(V[it])                           # W = A v_it
                        h = po.mdot(w, V[: it + 1], D)              # 1.
                        if any(_bad(v) for v in h):
                            st["reason"] = DIVERGED_NANORINF
                            break
                        u = po.maxpy(w, -h, V[: it + 1])            # 2.
                        tt = f(po.norm2(u, D))
                        refine = False                              # 3.
                        if cgs == "always":
                            refine = True
                        elif cgs == "ifneeded":
                            hsq = f(0.0)
                            for j in range(it + 1):
                                hsq = hsq + h[j] * h[j]
                            hnrm = np.sqrt(hsq)
                            if _bad(tt):
                                st["reason"] = DIVERGED_NANORINF
                                break
                            refine = bool(tt < hnrm)
                        if cgs != "never":
                            refined.append(refine)
                        c = None
                        if refine:                                  # 4.
                            c = po.mdot(u, V[: it + 1], D)
                            if any(_bad(v) for v in c):
                                st["reason"] = DIVERGED_NANORINF
                                break
                            u = po.maxpy(u, -c, V[: it + 1])
                            tt = f(po.norm2(u, D))
                        for j in range(it + 1):                     # 5.
                            hh = f(0.0)
                            hh = hh - (-h[j])
                            if refine:
                                hh = hh - (-c[j])
                            HH[j, it] = hh
                        if _bad(tt):
                            st["reason"] = DIVERGED_NANORINF
                            build = False                           # KSPCheckNorm: return before BuildSoln
                            break
                        V.append(u * scale_of(tt))
                        HH[it + 1, it] = tt
                        hapbnd = abs(tt / grs[it])
                        if hapbnd > haptol:
                            hapbnd = f(haptol)
                        if tt < hapbnd:
                            hapend = True
                        for j in range(1, it + 1):                  # KSPGMRESUpdateHessenberg
                            t0 = HH[j - 1, it]
                            HH[j - 1, it] = cc[j - 1] * t0 + ss[j - 1] * HH[j, it]
                            HH[j, it] = cc[j - 1] * HH[j, it] - (ss[j - 1] * t0)
                        if not hapend:
                            t2 = np.sqrt(HH[it, it] * HH[it, it] + HH[it + 1, it] * HH[it + 1, it])
                            if t2 == 0.0:
                                st["reason"] = DIVERGED_NULL
                            else:
                                cc[it] = HH[it, it] / t2
                                ss[it] = HH[it + 1, it] / t2
                                grs[it + 1] = -(ss[it] * grs[it])
                                grs[it] = cc[it] * grs[it]
                                HH[it, it] = cc[it] * HH[it, it] + ss[it] * HH[it + 1, it]
                                res = abs(grs[it + 1])
                        else:
                            res = f(0.0)
                        it += 1
                        st["its"] += 1
                        st["rnorm"] = res
                        if st["reason"]:
                            break
                        converged(st["its"], res)
                        if hapend and not st["reason"]:
                            st["reason"] = DIVERGED_BREAKDOWN
                            break
                    if build:
                        if it and (st["reason"] or st["its"] >= max_it):
                            hist.append(res)
                        cyc = it
                        k_it = it - 1                               # KSPGMRESBuildSoln(it - 1), nrs aliases grs
                        if k_it >= 0:
                            nrs, ok = grs, True
                            if HH[k_it, k_it] != 0.0:
                                nrs[k_it] = grs[k_it] / HH[k_it, k_it]
                            else:
                                st["reason"], ok = DIVERGED_BREAKDOWN, False
                            for ii in range(1, k_it + 1):
                                if not ok:
                                    break
                                k = k_it - ii
                                t3 = grs[k]
                                for j in range(k + 1, k_it + 1):
                                    t3 = t3 - HH[k, j] * nrs[j]
                                if HH[k, k] == 0.0:
                                    st["reason"], ok = DIVERGED_BREAKDOWN, False
                                    break
                                nrs[k] = t3 / HH[k, k]
                            if ok:
                                tmp = po.maxpy(np.zeros(n), nrs[: k_it + 1].copy(), V[: k_it + 1])
                                x = x + 1.0 * tmp
            itcount += cyc
            if itcount >= max_it:
                if not st["reason"]:
                    st["reason"] = DIVERGED_ITS
                break
            guess_zero = False
    cap = max_it + 2
    info = {"its": st["its"], "reason": st["reason"], "rnorm": float(st["rnorm"]),
            "hist": np.array(hist[:cap], np.float64), "refined": refined}
    if keep_basis:
        info["basis"] = V
    return x, info

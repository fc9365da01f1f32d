"""A Python KSPGMRES in the DBR order with an optional rounding of the stored basis (helper, not a test).

TEST INFRASTRUCTURE ONLY.  The structure is oracle/twin.py:gmres (KSPSolve_GMRES / KSPGMRESCycle, classical
Gram-Schmidt without refinement, PCNONE); the vector work goes through pyoracle's primitives -- Mat.mult,
Mat.residual, mdot, maxpy, norm2 in REDUCE_DBR -- so with rnd = identity it is the C oracle's DBR solve bit for bit
(tests/test_basis_twin.py pins that).

rnd is applied at the two places where compressed-basis GMRES (MSP_BASIS_F32) stores a basis vector:
  * the initial residual:  s_0 = rnd(b - A x), res = ||s_0||;
  * every Arnoldi step:    s_{it+1} = rnd(W - sum_j h_j v_j), its norm taken of the rounded values.
Vectors are kept as the device keeps them: stored unnormalised (s_j) with the scale sc[j] = 1/||s_j|| beside them,
every use reading v_j = s_j * sc[j] (one rounding per element, VecScale's).  Everything else is f64.
"""
from __future__ import annotations

import numpy as np
import pyoracle as po

CONVERGED_RTOL, CONVERGED_ATOL = 2, 3
DIVERGED_NULL, DIVERGED_ITS, DIVERGED_DTOL, DIVERGED_BREAKDOWN, DIVERGED_NANORINF = -2, -3, -4, -5, -9


def identity(v):
    return v


def f32(v):
    """rnd(v) = (double)(float)v: round to nearest even, gradual underflow, overflow to +-inf."""
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def _bad(v):
    return bool(np.isnan(v) or np.isinf(v))


def gmres(A: po.Mat, b, x0=None, rnd=identity, restart=30, max_it=10000, rtol=1e-5, abstol=1e-50, divtol=1e4,
          haptol=1e-30, breakdowntol=0.1, uirnorm=0, guess_nonzero=0):
    """Returns (x, {"its", "reason", "rnorm", "hist"}) like pyoracle.gmres."""
    D = po.REDUCE_DBR
    f = np.float64
    n = A.shape[0]
    m = restart
    b = np.ascontiguousarray(b, np.float64)
    guess_zero = not guess_nonzero
    orig_guess_zero = guess_zero
    x = np.zeros(n) if (x0 is None or guess_zero) else np.array(x0, np.float64, copy=True)
    st = dict(its=0, reason=0, rnorm=f(-1.0), rnorm0=f(0.0), ttol=f(0.0), gm_rnorm0=f(0.0))
    hist = []

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
            r = A.residual(b, x) if not guess_zero else b.copy()   # KSPInitialResidual, f64
            S = [rnd(r)]                                            # VV(0) as stored
            res = f(po.norm2(S[0], D))
            V = [S[0] * scale_of(res)]
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
                        w = A.mult(V[it])                           # W = A (sc[it] s_it)
                        lhh = po.mdot(w, V[: it + 1], D)
                        if any(_bad(v) for v in lhh):
                            st["reason"] = DIVERGED_NANORINF
                            break
                        lhh = -lhh
                        s_new = rnd(po.maxpy(w, lhh, V[: it + 1]))   # VV(it+1) as stored
                        for j in range(it + 1):
                            HH[j, it] = f(0.0) - lhh[j]
                        tt = f(po.norm2(s_new, D))                  # the norm of what is in memory
                        if _bad(tt):
                            st["reason"] = DIVERGED_NANORINF
                            build = False                           # KSPCheckNorm: return before BuildSoln
                            break
                        S.append(s_new)
                        V.append(s_new * scale_of(tt))
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
    return x, {"its": st["its"], "reason": st["reason"], "rnorm": float(st["rnorm"]),
               "hist": np.array(hist[:cap], np.float64)}

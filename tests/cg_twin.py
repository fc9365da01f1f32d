"""The numpy twin of the library's KSPCG: the definition the device solver is held to, bit for bit.

PETSc 3.22.1's KSPSolve_CG restated (KSP_CG_SYMMETRIC, left PC, the norm taken every iteration), with PCNONE or
Jacobi's dinv.  PETSc itself is not available to the tests, so parity with it is unpinned, as for GMRES.  Every
reduction goes through pyoracle's DBR primitives; every element operation is one numpy operation, so one rounding
(numpy never contracts a multiply and an add).

cg(A, b, ...) returns (x, {"its", "reason", "rnorm", "hist"}).  A is a pyoracle.Mat (mult / residual).
"""
from __future__ import annotations

import numpy as np

import pyoracle as po

CONVERGED_RTOL, CONVERGED_ATOL = 2, 3
DIVERGED_ITS, DIVERGED_DTOL, DIVERGED_INDEFINITE_PC, DIVERGED_NANORINF, DIVERGED_INDEFINITE_MAT = -3, -4, -8, -9, -10

DBR = po.REDUCE_DBR


def dot(x, y) -> float:
    return float(po.mdot(x, [y], DBR)[0])


def _bad(v) -> bool:
    return bool(np.isnan(v) or np.isinf(v))


def _sign(v) -> float:  # PetscSign
    return -1.0 if v < 0.0 else 1.0


class _Conv:
    """KSPConvergedDefault, the statements msplit_gmres.hip restates."""

    def __init__(self, rtol, abstol, divtol, guess_zero, uirnorm, bnorm):
        self.rtol, self.abstol, self.divtol = rtol, abstol, divtol
        self.guess_zero, self.uirnorm, self.bnorm = guess_zero, uirnorm, bnorm
        self.rnorm0 = self.ttol = 0.0

    def __call__(self, n, rnorm) -> int:
        if n == 0:
            if not self.guess_zero and not self.uirnorm:
                snorm = self.bnorm
                if snorm == 0.0:
                    snorm = rnorm
                self.rnorm0 = snorm
            else:
                self.rnorm0 = rnorm
            self.ttol = max(self.rtol * self.rnorm0, self.abstol)
        if _bad(rnorm):
            return DIVERGED_NANORINF
        if rnorm <= self.ttol:
            return CONVERGED_ATOL if rnorm < self.abstol else CONVERGED_RTOL
        if rnorm >= self.divtol * self.rnorm0:
            return DIVERGED_DTOL
        return 0


def cg(A, b, x0=None, dinv=None, norm="preconditioned", max_it=10000, rtol=1e-5, abstol=1e-50, divtol=1e4,
       uirnorm=False):
    """One KSPSolve.  x0 None: zero guess.  dinv None: PCNONE (z is r)."""
    assert norm in ("preconditioned", "unpreconditioned")
    b = np.ascontiguousarray(b, np.float64)
    n = len(b)
    with np.errstate(all="ignore"):
        if x0 is None:
            x = np.zeros(n)
            r = b.copy()
        else:
            x = np.array(x0, np.float64, copy=True)
            r = A.residual(b, x)
        pc = (lambda v: v) if dinv is None else (lambda v: dinv * v)

        def sums(z, r):
            """beta = z . r and dp (the one or two sums the update sweep leaves)."""
            beta = dot(z, r)
            if dinv is None:
                return beta, float(np.sqrt(beta))  # norm2 is sqrt(mdot(x, [x])): one reduction serves both
            return beta, float(po.norm2(z if norm == "preconditioned" else r, DBR))

        bnorm = 0.0
        if x0 is not None and not uirnorm:
            bnorm = float(po.norm2(pc(b), DBR))
        conv = _Conv(rtol, abstol, divtol, x0 is None, uirnorm, bnorm)
        z = pc(r)
        beta, dp = sums(z, r)
        hist = [dp]
        res = {"its": 0, "rnorm": dp}
        reason = conv(0, dp)
        if not reason and _bad(beta):  # KSPCheckDot
            reason = DIVERGED_NANORINF
        p = np.zeros(n)
        betaold = dpi = dpiold = 0.0
        i = 0
        while not reason and i < max_it:
            res["its"] = i + 1
            if beta == 0.0:
                reason = CONVERGED_ATOL
                break
            if i > 0 and beta * betaold < 0.0:
                reason = DIVERGED_INDEFINITE_PC
                break
            if i == 0:
                p = z.copy()
            else:
                bk = beta / betaold
                p = z + bk * p  # VecAYPX
            dpiold = dpi
            w = A.mult(p)
            dpi = dot(p, w)
            betaold = beta
            if _bad(dpi):
                reason = DIVERGED_NANORINF
                break
            if dpi == 0.0 or (i > 0 and _sign(dpi) * _sign(dpiold) < 0.0):
                reason = DIVERGED_INDEFINITE_MAT
                break
            a = beta / dpi
            x = x + a * p  # VecAXPY
            r = r + (-a) * w
            z = pc(r)
            beta, dp = sums(z, r)
            res["rnorm"] = dp
            hist.append(dp)
            reason = conv(i + 1, dp)
            if reason:
                break
            if _bad(beta):
                reason = DIVERGED_NANORINF
                break
            i += 1
        if not reason:
            reason = DIVERGED_ITS
    res["reason"] = reason
    res["hist"] = np.array(hist)
    return x, res

"""A Python KSPGMRES with PETSc's left Jacobi preconditioner, in the DBR order (helper, not a test).

TEST INFRASTRUCTURE ONLY.  The solver is tests/basis_twin.py's gmres (KSPSolve_GMRES / KSPGMRESCycle, classical
Gram-Schmidt without refinement, vector work through pyoracle's primitives in REDUCE_DBR) with rnd = identity; the
preconditioner enters at the three places of the contract (include/msplit.h, MSP_PC_JACOBI), each one numpy f64
multiply per element, applied to an already rounded vector:

  * KSPInitialResidual:   VV(0) = dinv .* (b - A x), or dinv .* b for a zero guess;
  * every Arnoldi step:   W = dinv .* (A v), the MatMult's result rounded first, then the pointwise multiply;
  * KSPConvergedDefault at its = 0 with a nonzero guess and no uirnorm:  rnorm0 = ||dinv .* b||.

Left preconditioning with the preconditioned norm changes nothing else: h, the MAXPY, the norms, the Hessenberg,
the rotations, the tests and BuildSoln are the unpreconditioned solver's, run on those vectors.  So the twin hands
basis_twin.gmres an operator whose mult and residual end with the multiply, and dinv .* b as the right-hand side --
which that solver copies for a zero guess, takes the norm of for rnorm0, and otherwise only passes back to
residual(), where the raw b is used.

dinv comes from the CSR arrays by PCSetUp's rule (jacobi_dinv): 1 / a_ii by one f64 division; 1.0 where row i
stores no diagonal entry or a_ii is +-0.0; the first occurrence of the diagonal counts; no other special case (a
subnormal a_ii whose reciprocal overflows gives inf).
"""
from __future__ import annotations

import numpy as np

import basis_twin as bt


def diagonal(rowptr, col, val) -> np.ndarray:
    """MatGetDiagonal: a_ii as stored (first occurrence), 0.0 where row i stores none."""
    n = len(rowptr) - 1
    d = np.zeros(n)
    for i in range(n):
        lo, hi = int(rowptr[i]), int(rowptr[i + 1])
        hit = np.flatnonzero(np.asarray(col[lo:hi]) == i)
        if hit.size:
            d[i] = val[lo + int(hit[0])]
    return d


def jacobi_dinv(rowptr, col, val) -> np.ndarray:
    """PCSetUp of PCJACOBI (diagonal): 1 / a_ii, and 1.0 where a_ii is +-0.0 or absent."""
    d = diagonal(rowptr, col, val)
    zero = d == 0.0                              # +0.0 and -0.0
    with np.errstate(over="ignore", divide="ignore"):
        return np.where(zero, np.float64(1.0), np.float64(1.0) / np.where(zero, np.float64(1.0), d))


class _LeftJacobi:
    """A with PCApply behind every product: mult(v) = dinv .* (A v), residual(., x) = dinv .* (b - A x)."""

    def __init__(self, A, b, dinv):
        self.A, self.b, self.dinv = A, b, dinv
        self.shape = A.shape

    def mult(self, v):
        return self.A.mult(v) * self.dinv         # the product rounded, then one multiply per element

    def residual(self, pb, x):                    # pb is dinv .* b: the true residual needs the raw b
        return self.A.residual(self.b, x) * self.dinv


def gmres(A, b, dinv, x0=None, **opts):
    """Left-Jacobi GMRES of A x = b; returns (x, {"its", "reason", "rnorm", "hist"}) like pyoracle.gmres, the norms
    those of the preconditioned residual.  dinv = ones is the unpreconditioned DBR solve bit for bit."""
    b = np.ascontiguousarray(b, np.float64)
    dinv = np.ascontiguousarray(dinv, np.float64)
    with np.errstate(all="ignore"):
        pb = b * dinv
        return bt.gmres(_LeftJacobi(A, b, dinv), pb, x0=x0, rnd=bt.identity, **opts)

"""The operator of compressed-operator GMRES (MSP_OPER_F32) for the Python twins (helper, not a test).

TEST INFRASTRUCTURE ONLY.  The contract (include/msplit.h): the Arnoldi products read a copy of the CSR operator
whose values are a~ = (float)a, every row summed in f64 in CSR order -- the f64 MatMult on the matrix
(double)(float)a, bit for bit; KSPInitialResidual at every restart, the diagonal and Jacobi's dinv read the f64
values.  RoundedOperator is exactly that pair: mult is pyoracle's Mat.mult on the rounded values, residual is the f64
matrix's.  The existing twin solvers take it in place of a pyoracle Mat and stay untouched:

  basis_twin.gmres(Op, b, rnd=identity | f32)     double and single basis
  basis_b16.gmres(Op, b)                          block16 basis
  pc_twin.gmres(Op, b, dinv)                      left Jacobi, dinv from the f64 values
"""
from __future__ import annotations

import numpy as np
import pyoracle as po


def round_values(val) -> np.ndarray:
    """(double)(float)a per entry: round to nearest even, gradual underflow, overflow to +-inf, -0.0 kept."""
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(val, np.float64).astype(np.float32).astype(np.float64)


def overflow_count(val) -> int:
    """The finite values whose float is not finite: what MSP_OPER_F32 refuses a matrix for."""
    val = np.asarray(val, np.float64)
    return int(np.count_nonzero(np.isfinite(val) & ~np.isfinite(round_values(val))))


class RoundedOperator:
    """mult(v) = A~ v with a~ = (double)(float)a, residual(b, x) = b - A x with the f64 values."""

    def __init__(self, n, rowptr, col, val):
        self.A = po.Mat.from_arrays(n, n, rowptr, col, val)
        self.At = po.Mat.from_arrays(n, n, rowptr, col, round_values(val))
        self.shape = self.A.shape

    def mult(self, v):
        return self.At.mult(v)

    def residual(self, b, x):
        return self.A.residual(b, x)

"""The Python twin of compressed-operator GMRES (tests/oper_twin.py), on the CPU.

1. On float-exact values (the Poisson boxes of BOX_CASES: -1, 4, 6) rounding changes no bit, so the twin is the C
   oracle's DBR solve bit for bit -- its, reason, history, rnorm, x -- which pins the twin's structure.
2. The rounding rule against hand-computed floats: ties to even, a value that lands in the float subnormals, -0.0,
   and 1e39 -> inf (counted as an overflow; NaN and inf themselves are not).
3. On values that are not float-exact the twin's history differs from the f64 oracle's: without this a GPU test
   could pass with the option ignored.
4. For a solve that restarts, the first history entry of the second cycle is the f64 residual of the twin's x --
   not the rounded operator's.
"""
import numpy as np
import pytest

import basis_twin as bt
import oper_twin as ot
from test_gpu_basis_f32 import BOX_CASES
from test_gpu_pc_jacobi import _variable_diagonal_csr


@pytest.mark.parametrize("name", list(BOX_CASES))
def test_float_exact_twin_is_the_dbr_oracle(oracle, name):
    dim, (nx, ny, nz), o, nonzero = BOX_CASES[name]
    O = oracle.poisson3d_rows(nx, ny, nz, 0, nz) if dim == 3 else oracle.poisson2d_rows(nx, ny, 0, nx * ny)
    n = O.shape[0]
    rp, col, val = O.arrays()
    assert np.array_equal(ot.round_values(val), val)
    Op = ot.RoundedOperator(n, rp, col, val)
    b = O.mult(np.ones(n))
    x0 = np.random.default_rng(7).uniform(-1, 1, n) if nonzero else None
    kw = dict(o, guess_nonzero=1 if nonzero else 0)
    xo, ro = oracle.gmres(O, b, x0=x0, reduce_mode=oracle.REDUCE_DBR, **kw)
    xt, rt = bt.gmres(Op, b, x0=x0, **kw)
    assert (rt["its"], rt["reason"]) == (ro["its"], ro["reason"])
    assert np.array_equal(rt["hist"], ro["hist"])
    assert rt["rnorm"] == ro["rnorm"]
    assert np.array_equal(xt, xo)


def test_rounding_rule():
    e = 2.0 ** -24                                   # half a float ulp at 1.0
    flt_max = (2.0 - 2.0 ** -23) * 2.0 ** 127
    v = np.array([1.0 + e, 1.0 + 3 * e, 1.0 + e + 2.0 ** -50, 1e-40, -0.0, 1e39, -1e39,
                  (2.0 - 2.0 ** -24) * 2.0 ** 127, (2.0 - 2.0 ** -24 - 2.0 ** -40) * 2.0 ** 127, 0.1, 5e-324])
    want = np.array([1.0, 1.0 + 4 * e, 1.0 + 2 * e,                 # ties to even (down, up), just above a tie
                     np.rint(1e-40 * 2.0 ** 149) * 2.0 ** -149,      # a float subnormal: a multiple of 2^-149
                     -0.0, np.inf, -np.inf,
                     np.inf, flt_max,                                # the tie at the top goes to 2^128, below it stays
                     float(np.float32(0.1)), 0.0])
    got = ot.round_values(v)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.signbit(got[4]) and 0.0 < got[3] < 2.0 ** -126 and got[3] != 1e-40
    assert ot.overflow_count(v) == 3                                 # 1e39, -1e39 and the tie at the top
    special = np.array([np.nan, np.inf, -np.inf])
    assert ot.overflow_count(special) == 0                           # they pass through as they are
    assert np.array_equal(ot.round_values(special), special, equal_nan=True)


def _variable_problem():
    rp, col, val = _variable_diagonal_csr()
    n = len(rp) - 1
    return n, rp, col, val, np.random.default_rng(5).uniform(-1, 1, n)


def test_rounded_values_change_the_solve(oracle):
    n, rp, col, val, b = _variable_problem()
    assert not np.array_equal(ot.round_values(val), val)
    o = dict(restart=30, max_it=60, rtol=1e-8)
    xo, ro = oracle.gmres(oracle.Mat.from_arrays(n, n, rp, col, val), b, reduce_mode=oracle.REDUCE_DBR, **o)
    xt, rt = bt.gmres(ot.RoundedOperator(n, rp, col, val), b, **o)
    assert rt["hist"][0] == ro["hist"][0]                             # ||b||: no product yet
    assert rt["hist"][1] != ro["hist"][1]
    assert not np.array_equal(xt, xo)


def test_restart_takes_the_f64_residual(oracle):
    n, rp, col, val, b = _variable_problem()
    Op = ot.RoundedOperator(n, rp, col, val)
    m = 5
    o = dict(restart=m, rtol=1e-30)
    x1, r1 = bt.gmres(Op, b, max_it=m, **o)                           # exactly the first cycle
    _, r2 = bt.gmres(Op, b, max_it=2 * m, **o)
    assert r1["its"] == m and r2["its"] == 2 * m
    assert np.array_equal(r2["hist"][:m], r1["hist"][:m])
    D = oracle.REDUCE_DBR
    assert r2["hist"][m] == oracle.norm2(Op.A.residual(b, x1), D)    # the true residual of the cycle's x
    assert r2["hist"][m] != oracle.norm2(Op.At.residual(b, x1), D)   # not the rounded operator's

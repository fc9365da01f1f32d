"""The Python twin of left-Jacobi GMRES (tests/pc_twin.py), on the CPU.

1. With dinv = ones the twin is the C oracle's DBR solve bit for bit on the six BOX_CASES of test_gpu_basis_f32.py
   (a multiply by 1.0 changes no bit), which pins the twin's structure.
2. The scaling identity.  On an operator whose diagonal is the constant 4.0 (2D Poisson), dinv = 0.25 everywhere and
   every multiply by it is exact, so the Jacobi solve is the unpreconditioned one with every residual-sized
   quantity scaled by 2^-2: same its, reason and x bits as the C oracle, history exactly 0.25 x the oracle's.
   That pins the three places where dinv enters independently of the twin itself -- with a nonzero guess, with
   uirnorm (rnorm0 from the initial residual) and without it (rnorm0 = ||dinv .* b||).
3. PCSetUp's rule: a stored 0.0, a stored -0.0 and an absent diagonal give 1.0; a negative diagonal its reciprocal.
"""
import numpy as np
import pytest

import pc_twin as pt
from test_gpu_basis_f32 import BOX_CASES


def _box(oracle, dim, nx, ny, nz):
    O = oracle.poisson3d_rows(nx, ny, nz, 0, nz) if dim == 3 else oracle.poisson2d_rows(nx, ny, 0, nx * ny)
    return O, O.mult(np.ones(O.shape[0]))


@pytest.mark.parametrize("name", list(BOX_CASES))
def test_unit_dinv_twin_is_the_dbr_oracle(oracle, name):
    dim, (nx, ny, nz), o, nonzero = BOX_CASES[name]
    O, b = _box(oracle, dim, nx, ny, nz)
    n = O.shape[0]
    x0 = np.random.default_rng(7).uniform(-1, 1, n) if nonzero else None
    kw = dict(o, guess_nonzero=1 if nonzero else 0)
    xo, ro = oracle.gmres(O, b, x0=x0, reduce_mode=oracle.REDUCE_DBR, **kw)
    xt, rt = pt.gmres(O, b, np.ones(n), x0=x0, **kw)
    assert (rt["its"], rt["reason"]) == (ro["its"], ro["reason"])
    assert np.array_equal(rt["hist"], ro["hist"])
    assert rt["rnorm"] == ro["rnorm"]
    assert np.array_equal(xt, xo)


def poisson2d_identity_problem(oracle):
    """33 x 40 2D Poisson, diagonal asserted to be the constant 4.0; b = A 1, a seeded nonzero guess."""
    O = oracle.poisson2d_rows(33, 40, 0, 33 * 40)
    rp, col, val = O.arrays()
    assert np.array_equal(pt.diagonal(rp, col, val), np.full(O.shape[0], 4.0))
    dinv = pt.jacobi_dinv(rp, col, val)
    assert np.array_equal(dinv, np.full(O.shape[0], 0.25))
    b = O.mult(np.ones(O.shape[0]))
    x0 = np.random.default_rng(7).uniform(-1, 1, O.shape[0])
    return O, b, x0, dinv


IDENTITY_OPTS = dict(restart=30, max_it=500, rtol=1e-6, guess_nonzero=1)


@pytest.mark.parametrize("uirnorm", [0, 1])
def test_scaling_identity_against_the_c_oracle(oracle, uirnorm):
    O, b, x0, dinv = poisson2d_identity_problem(oracle)
    kw = dict(IDENTITY_OPTS, uirnorm=uirnorm)
    xo, ro = oracle.gmres(O, b, x0=x0, reduce_mode=oracle.REDUCE_DBR, **kw)
    xt, rt = pt.gmres(O, b, dinv, x0=x0, **kw)
    assert ro["its"] > 30 and ro["reason"] == 2               # more than one cycle, CONVERGED_RTOL
    assert (rt["its"], rt["reason"]) == (ro["its"], ro["reason"])
    assert np.array_equal(rt["hist"], 0.25 * ro["hist"])
    assert rt["rnorm"] == 0.25 * ro["rnorm"]
    assert np.array_equal(xt, xo)


def test_pcsetup_rule():
    # row 0: stored 0.0; row 1: stored -0.0; row 2: no diagonal entry; row 3: negative; row 4: 8.0; row 5: empty
    rp = np.array([0, 2, 4, 5, 7, 8, 8], np.int32)
    col = np.array([0, 3, 0, 1, 0, 2, 3, 4], np.int32)
    val = np.array([0.0, 1.0, 2.0, -0.0, 3.0, 5.0, -0.5, 8.0])
    d = pt.diagonal(rp, col, val)
    assert np.array_equal(d, [0.0, -0.0, 0.0, -0.5, 8.0, 0.0]) and np.signbit(d[1])
    assert np.array_equal(pt.jacobi_dinv(rp, col, val), [1.0, 1.0, 1.0, -2.0, 0.125, 1.0])
    # no other special case: a subnormal diagonal whose reciprocal overflows gives inf
    assert pt.jacobi_dinv(np.array([0, 1], np.int32), np.array([0], np.int32), np.array([5e-324]))[0] == np.inf

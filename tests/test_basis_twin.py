"""The Python twin of compressed-basis GMRES (tests/basis_twin.py), on the CPU.

1. With rnd = identity the twin is the C oracle's DBR solve bit for bit on the seven CASES of test_gpu_gmres.py,
   which pins the twin's structure (and so what the f32 variant changes: the two roundings only).
2. With rnd = f32 the solve behaves as the f64 one: CONVERGED_RTOL, the same iteration count within one, and a
   true residual ||b - A x|| / ||b|| <= rtol, at GMRES(30) with rtol 1e-4 and 1e-10 (every restart recomputes the
   residual in f64, so the rounded basis does not limit the attainable tolerance).
"""
import numpy as np
import pytest

import basis_twin as bt
from test_gpu_gmres import CASES


def _problem(oracle, dim, nx, ny, nz):
    O = oracle.poisson3d_rows(nx, ny, nz, 0, nz) if dim == 3 else oracle.poisson2d_rows(nx, ny, 0, nx * ny)
    return O, O.mult(np.ones(O.shape[0]))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_identity_twin_is_the_dbr_oracle(oracle, case):
    dim, (nx, ny, nz), o, nonzero = CASES[case]
    O, b = _problem(oracle, dim, nx, ny, nz)
    x0 = np.random.default_rng(7).uniform(-1, 1, O.shape[0]) if nonzero else None
    kw = dict(o, guess_nonzero=1 if nonzero else 0)
    xo, ro = oracle.gmres(O, b, x0=x0, reduce_mode=oracle.REDUCE_DBR, **kw)
    xt, rt = bt.gmres(O, b, x0=x0, rnd=bt.identity, **kw)
    assert (rt["its"], rt["reason"]) == (ro["its"], ro["reason"])
    assert np.array_equal(rt["hist"], ro["hist"])
    assert rt["rnorm"] == ro["rnorm"]
    assert np.array_equal(xt, xo)


@pytest.mark.parametrize("rtol", [1e-4, 1e-10])
@pytest.mark.parametrize("grid", [(16, 16, 16), (16, 16, 33)])
def test_f32_basis_converges_like_f64(oracle, grid, rtol):
    O, b = _problem(oracle, 3, *grid)
    kw = dict(restart=30, max_it=10000, rtol=rtol)
    x64, r64 = bt.gmres(O, b, rnd=bt.identity, **kw)
    x32, r32 = bt.gmres(O, b, rnd=bt.f32, **kw)
    true = np.linalg.norm(b - O.mult(x32)) / np.linalg.norm(b)
    true64 = np.linalg.norm(b - O.mult(x64)) / np.linalg.norm(b)
    print(f"{grid} rtol {rtol:g}: its f64 {r64['its']} f32 {r32['its']}; true residual / rtol: f64 {true64 / rtol:.3f} "
          f"f32 {true / rtol:.3f}")
    assert r64["reason"] == bt.CONVERGED_RTOL and r32["reason"] == bt.CONVERGED_RTOL
    assert abs(r32["its"] - r64["its"]) <= 1
    assert true <= rtol
    assert not np.array_equal(x32, x64)   # the rounding is applied: the two solves are different computations

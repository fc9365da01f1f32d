"""The Python twin of the SMSM-global loop (tests/minim_twin.py), on the CPU.

With rnd = identity the twin is the C oracle's orc_smsm_solve (DBR) bit for bit: outer count, norm0, every outer
residual, the LSQR iteration counts and reasons, every inner iteration count, x, the final norm and the error.  That
pins the twin's structure, and so what rnd = f32 changes: the one rounding of R = A S only.  With rnd = f32 the run
is a different computation whose stop test reads the LSQR residual of the rounded R.
"""
import numpy as np
import pytest

import minim_twin as mt

INNER = dict(restart=30, max_it=20, rtol=1e-20, abstol=1e-100)
OUTER = dict(max_it=70, rtol=1e-15, abstol=1e-100, exact_norm=1, conv_test=0)
CASES = [(3, 8, 8, 12, 1, 4), (3, 8, 8, 12, 2, 4), (3, 8, 8, 12, 3, 4), (2, 32, 32, 1, 2, 4)]


@pytest.mark.parametrize("dim,nx,ny,nz,nb,s", CASES)
def test_identity_twin_is_the_smsm_oracle(oracle, dim, nx, ny, nz, nb, s):
    ro = oracle.smsm_solve(dim, nx, ny, nz, nb, s, 1e-6, dict(INNER, reduce_mode=oracle.REDUCE_DBR),
                           dict(OUTER, reduce_mode=oracle.REDUCE_DBR), max_outer=100)
    rt = mt.smsm_global(oracle, dim, nx, ny, nz, nb, s, 1e-6, INNER, OUTER, max_outer=100, rnd=mt.identity)
    assert rt["outer_its"] == ro["outer_its"]
    assert rt["norm0"] == ro["norm0"]
    assert np.array_equal(rt["hist"], ro["hist"])
    assert np.array_equal(rt["lsqr_its"], ro["lsqr_its"])
    assert np.array_equal(rt["lsqr_reason"], ro["lsqr_reason"])
    assert np.array_equal(rt["inner_its"], ro["inner_its"])
    assert np.array_equal(rt["x"], ro["x"])
    assert rt["final_norm"] == ro["final_norm"]
    assert rt["error"] == ro["error"]


def test_f32_twin_rounds_r_and_still_converges(oracle):
    dim, nx, ny, nz, nb, s = CASES[2]
    r64 = mt.smsm_global(oracle, dim, nx, ny, nz, nb, s, 1e-6, INNER, OUTER, max_outer=100, rnd=mt.identity)
    r32 = mt.smsm_global(oracle, dim, nx, ny, nz, nb, s, 1e-6, INNER, OUTER, max_outer=100, rnd=mt.f32)
    print(f"outer its f64 {r64['outer_its']} f32 {r32['outer_its']}; final norm f64 {r64['final_norm']:.3e} "
          f"f32 {r32['final_norm']:.3e}")
    assert not np.array_equal(r32["x"], r64["x"])          # the rounding is applied
    assert r32["hist"][-1] <= 1e-6 * r32["norm0"]           # the stop test was met, not the outer cap
    assert r32["outer_its"] < 100

"""The block16 rounding (tests/basis_b16.py) and its GMRES twin, on the CPU.

1. Unit checks of block16(v) against the rule of include/msplit.h: the clamp, ties to even, zero chunks, signed
   zeros, a subnormal maximum, non-finite entries poisoning exactly their own chunk, a partial last chunk and odd n,
   idempotence.
2. The twin with rnd = block16 converges as the f64 one does at GMRES(30), within the documented one-cycle limit:
   inside one restart cycle the recurrence residual can run ahead of the true residual by about 2^-13 of the cycle's
   initial residual, so a tolerance reached inside the first cycle (rtol 1e-4 here) is held to 3 * rtol, and one
   reached across restarts (1e-10) to rtol itself.  These bounds state that limit; the device is held to bits
   (tests/test_gpu_basis_b16.py).
"""
import numpy as np
import pytest

import basis_b16 as b16
import basis_twin as bt

C = b16.CHUNK


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_clamp_is_reachable():
    """max = 1 - 2^-20 = m 2^0 with m >= 32767.5/32768: it scales to 32767.97, rounds to 32768 and is clamped."""
    v = np.zeros(C)
    v[3], v[5], v[7] = 1.0 - 2.0 ** -20, 0.5, -(1.0 - 2.0 ** -20)
    s = b16.block16(v)
    assert s[3] == 32767.0 / 32768.0 and s[7] == -32767.0 / 32768.0
    assert s[5] == 0.5
    q, E = b16.quantise(v)
    assert E == [0] and q[3] == 32767 and q[7] == -32767 and q[5] == 16384


def test_ties_go_to_even():
    v = np.zeros(C)
    v[0] = 0.75                               # E = 0: one unit is 2^-15
    u = 2.0 ** -15
    v[1:7] = [0.5 * u, 1.5 * u, 2.5 * u, -0.5 * u, -1.5 * u, -2.5 * u]
    s = b16.block16(v)
    assert np.array_equal(s[1:7], [0.0, 2 * u, 2 * u, 0.0, -2 * u, -2 * u])
    assert s[0] == 0.75


def test_zero_chunks_and_signed_zeros():
    v = np.zeros(3 * C)
    v[:C] = 1.0
    v[C:2 * C] = -0.0                         # an all-zero chunk between two others
    v[2 * C] = 3.0
    v[2 * C + 1] = -0.0
    v[2 * C + 2] = -2.0 ** -40                # rounds to a zero
    s = b16.block16(v)
    assert np.all(_bits(s[C:2 * C]) == 0)     # +0.0
    assert s[2 * C + 1] == 0.0 and s[2 * C + 2] == 0.0
    assert np.all(s[:C] == 1.0) and s[2 * C] == 3.0
    assert b16.chunk_exponents(v) == [1, 0, 2]


def test_subnormal_maximum():
    tiny = 2.0 ** -1074
    v = np.zeros(C)
    v[0], v[1] = tiny, -tiny
    assert b16.chunk_exponents(v) == [-1073]
    assert np.array_equal(_bits(b16.block16(v)), _bits(v))
    v[0], v[1], v[2] = 3 * 2.0 ** -1060, 2.0 ** -1074, -2.0 ** -1065
    s = b16.block16(v)
    assert s[0] == v[0] and s[1] == 0.0 and s[2] == v[2]
    huge = np.full(C, 2.0 ** 1023)
    huge[1] = -1.5 * 2.0 ** 1023
    assert np.array_equal(b16.block16(huge), huge)    # the top of the range: no overflow


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_entry_poisons_exactly_its_chunk(bad):
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, 2 * C + 17)
    want = b16.block16(v)
    for k in range(3):
        w = v.copy()
        w[min(k * C + 11, w.size - 1)] = bad
        s = b16.block16(w)
        lo, hi = k * C, min((k + 1) * C, w.size)
        assert np.all(np.isnan(s[lo:hi]))
        keep = np.ones(w.size, bool)
        keep[lo:hi] = False
        assert np.array_equal(_bits(s[keep]), _bits(want[keep]))
        assert [e is None for e in b16.chunk_exponents(w)] == [j == k for j in range(3)]


@pytest.mark.parametrize("n", [1, 1001, C - 1, C, C + 1, 2 * C + 1])
def test_partial_chunk_odd_n_error_bound_and_idempotence(n):
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    s = b16.block16(v)
    assert s.shape == (n,)
    for lo in range(0, n, C):
        M = np.max(np.abs(v[lo:lo + C]))
        unit = 2.0 ** (np.frexp(M)[1] - 15)
        err = np.abs(s[lo:lo + C] - v[lo:lo + C])
        assert np.all(err <= unit)                                   # the clamp costs up to one unit
        assert np.all(err[np.abs(v[lo:lo + C]) < M * (1 - 2.0 ** -15)] <= unit / 2)
    assert np.array_equal(_bits(b16.block16(s)), _bits(s))


def test_idempotent_on_the_clamped_chunk():
    v = np.zeros(C)
    v[0], v[1] = 1.0 - 2.0 ** -20, 0.3
    s = b16.block16(v)
    assert np.array_equal(_bits(b16.block16(s)), _bits(s))


def _problem(oracle, nx, ny, nz):
    O = oracle.poisson3d_rows(nx, ny, nz, 0, nz)
    return O, O.mult(np.ones(O.shape[0]))


@pytest.mark.parametrize("rtol", [1e-4, 1e-10])
@pytest.mark.parametrize("grid", [(16, 16, 16), (16, 16, 33)])
def test_block16_basis_converges_within_the_one_cycle_limit(oracle, grid, rtol):
    O, b = _problem(oracle, *grid)
    kw = dict(restart=30, max_it=10000, rtol=rtol)
    x64, r64 = bt.gmres(O, b, rnd=bt.identity, **kw)
    x32, r32 = bt.gmres(O, b, rnd=bt.f32, **kw)
    x16, r16 = b16.gmres(O, b, **kw)
    true = np.linalg.norm(b - O.mult(x16)) / np.linalg.norm(b)
    print(f"{grid} rtol {rtol:g}: its f64 {r64['its']} f32 {r32['its']} block16 {r16['its']}; "
          f"true residual / rtol: block16 {true / rtol:.3f}")
    assert r16["reason"] == bt.CONVERGED_RTOL and r64["reason"] == bt.CONVERGED_RTOL
    assert not np.array_equal(x16, x64) and not np.array_equal(x16, x32)
    assert r16["its"] <= 1.5 * r64["its"]
    assert true <= (3 * rtol if rtol == 1e-4 else rtol)

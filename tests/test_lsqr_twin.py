"""The launcher-by-launcher twin of KSPLSQR (tests/lsqr_twin.py) against the C oracle (CPU only).

Chaining the twin's calls as msp_lsqr_solve chains the launchers must give oracle.lsqr's record bit for bit --
x, its, reason, rnorm, arnorm, anorm, the history -- in both step forms, with and without the exact norm, under
the three convergence tests, over 1, 2 and 3 row blocks and on every crafted branch input; and each branch input
must end with the reason it is named for.  Only then may the GPU tests take the twin as the reference of a
single call.
"""
import numpy as np
import pytest

import _lsqr_branch_cases as bc
from guarded import assert_same_bits


def _same_record(x, r, xo, ro, what):
    assert (r["its"], r["reason"]) == (ro["its"], ro["reason"]), what
    for f in ("rnorm", "arnorm", "anorm", "hist"):
        assert_same_bits(r[f], ro[f], f"{what}: {f}")
    assert_same_bits(x, xo, f"{what}: x")


@pytest.mark.parametrize("cuts", [(4100,), (4096, 4), (3000, 1, 1099)], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("onepass", [0, 1])
@pytest.mark.parametrize("name,conv", bc.RUNS)
def test_twin_chain_is_the_oracle_on_every_branch(oracle, name, conv, onepass, cuts):
    import lsqr_twin as lt
    R, b, o, want = bc.case(name)
    Rs, bs = bc.blocks(R, b, cuts)
    for exact in (0, 1):
        kw = dict(o, conv_test=conv, exact_norm=exact)
        xo, ro = oracle.lsqr(Rs, bs, reduce_mode=oracle.REDUCE_DBR, onepass=onepass, **kw)
        assert ro["reason"] == want[conv], f"{name} does not reach its branch: reason {ro['reason']}"
        x, r = lt.solve(Rs, bs, onepass_step=onepass, **kw)
        _same_record(x, r, xo, ro, f"{name} conv {conv} onepass {onepass} exact {exact}")


@pytest.mark.parametrize("onepass", [0, 1])
@pytest.mark.parametrize("s", [1, 5, 33])
def test_twin_chain_mixed_precision_blocks(oracle, s, onepass):
    """A float block is the oracle over the promoted values; n = 9000 over three blocks, one of one row."""
    import lsqr_twin as lt
    rng = np.random.default_rng(5)
    cuts = (4097, 1, 4902)
    R = rng.standard_normal((sum(cuts), s)) @ np.diag(np.geomspace(1, 1e-2, s))
    Rs, bs = bc.blocks(R, rng.standard_normal(sum(cuts)), cuts)
    prec = ["single", "double", "single"]
    kw = dict(max_it=8, rtol=1e-15, abstol=1e-100, exact_norm=1, conv_test=0)
    x, r = lt.solve(Rs, bs, precisions=prec, onepass_step=onepass, **kw)
    xo, ro = oracle.lsqr([lt.promote(M, p) for M, p in zip(Rs, prec)], bs, reduce_mode=oracle.REDUCE_DBR,
                         onepass=onepass, **kw)
    assert ro["reason"] == (-3 if s > 1 else -9)    # one column: V1 is rounding noise or 0 after a step, then 0 / 0
    _same_record(x, r, xo, ro, f"s {s}")
    assert not np.array_equal(x, oracle.lsqr(Rs, bs, reduce_mode=oracle.REDUCE_DBR, onepass=onepass, **kw)[0])


def test_dense_twins_skip_the_axpy_and_scale_as_stored(oracle):
    """nal == 0 or no U: no VecAXPY (a NaN in U stays out); usc: U * usc is rounded before nal multiplies it."""
    import lsqr_twin as lt
    rng = np.random.default_rng(6)
    R, V, U = rng.standard_normal((50, 3)), rng.standard_normal(3), rng.standard_normal(50)
    rows = oracle.dense_mult(R, V)
    bad = U.copy()
    bad[3] = np.nan
    for nal in (0.0, -0.0):
        assert_same_bits(lt.onepass(R, V, nal, bad, 0.5)[0], rows)
        assert_same_bits(lt.gemv(R, V, nal, bad, None)[0], rows)
    assert_same_bits(lt.onepass(R, V, -1.5, None, None)[0], rows)
    y, out = lt.onepass(R, V, -1.5, U, 1 / 3)
    assert_same_bits(y, rows + (-1.5) * (U * (1 / 3)))
    assert out[0] == oracle.dot(y, y, oracle.REDUCE_DBR) and out[2] == oracle.dot(R[:, 1], y, oracle.REDUCE_DBR)
    w, d = lt.scaled_dots(U, 1 / 3, R, True)
    assert_same_bits(w, U * (1 / 3))
    assert lt.scaled_dots(U, 1 / 3, R, False)[0] is None and lt.scaled_dots(U, None, R, True)[0] is None
    assert_same_bits(d, [oracle.dot(R[:, j], U * (1 / 3), oracle.REDUCE_DBR) for j in range(3)])
    assert_same_bits(lt.colsumsq(R), [oracle.dot(R[:, j], R[:, j], oracle.REDUCE_DBR) for j in range(3)])
    assert_same_bits(lt.onepass(R[:0], V, -1.0, U[:0], None)[1], np.zeros(4))       # no rows: +0.0

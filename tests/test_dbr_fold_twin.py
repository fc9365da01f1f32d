"""The NumPy twin of the stage-2 DBR fold (tests/dbr_fold.py) against the C oracle, on the CPU.

For partials p of length nch the vector x = zeros(nch * 4096) with x[c * 4096] = p[c] has exact stage-1 partials: in
chunk c lane 0 adds p[c] * 1.0 to +0.0 and every other sum is +0.0, so the chunk's butterfly and wave sum return
p[c] itself (a -0.0 comes out as +0.0, which the fold cannot tell apart: every lane starts at +0.0).  The oracle's
DBR dot of x with ones is then the fold of p, and must equal dbr_fold.fold(p) bit for bit -- at every chunk count up
to 4097 where a lane's trip count changes, and with a ragged last chunk.  Larger counts (the GPU tests go to 20225)
rest on the twin alone: its statements do not depend on the count.
"""
import numpy as np
import pytest

import dbr_fold as df
from guarded import assert_same_bits

PINNED = [1, 2, 255, 256, 257, 1792, 1793, 3840, 3841, 4097]


def _oracle_fold(oracle, p, n=None):
    n = p.size * df.CHUNK if n is None else n
    x = np.zeros(n)
    x[::df.CHUNK] = p
    return oracle.dot(x, np.ones(n), oracle.REDUCE_DBR)


@pytest.mark.parametrize("nch", PINNED)
def test_fold_is_the_oracles_stage_two(oracle, nch):
    for name, p in df.data_sets(nch, 100 + nch).items():
        assert_same_bits(df.fold(p), _oracle_fold(oracle, p), f"{name}, {nch} partials")


def test_fold_with_a_ragged_last_chunk(oracle):
    n = 299 * df.CHUNK + 7
    for name, p in df.data_sets(300, 7).items():
        assert_same_bits(df.fold(p), _oracle_fold(oracle, p, n), f"{name}, n = {n}")


def test_fold_is_not_a_plain_sum():
    """The order matters on this data: the twin differs from the left-to-right sum and from NumPy's pairwise one, so a
    kernel that folded in another order would be caught."""
    differs = 0
    for nch in (257, 1793, 4097):
        p = df.data_sets(nch, 100 + nch)["mixed"]
        seq = np.float64(0.0)
        for v in p:
            seq = seq + v
        differs += int(df.fold(p) != seq) + int(df.fold(p) != np.sum(p))
    assert differs >= 4
    assert np.signbit(df.fold(np.full(300, -0.0))) == False  # noqa: E712  (+0.0, not -0.0)

"""The stage-2 DBR fold as NumPy statements (helper, not a test).

TEST INFRASTRUCTURE ONLY.  Stage 1 of a DBR dot leaves one partial per 4096-row chunk; stage 2 folds the nchunks
partials of a vector in one workgroup of 256 lanes (four waves of 64).  The library holds three hand-written copies
of that fold -- k_dot_stage2 (msplit_k_dot.hip), fold_partials (msplit_gmres.hip) and fold (msplit_k_cg.hip) -- and
each promises the order restated here:

  lane t     acc = +0.0; acc = acc + p[t]; acc = acc + p[t + 256]; ...            (ascending, one add per partial)
  wave       v[l] = v[l] + v[l ^ off] for off = 32, 16, 8, 4, 2, 1                 (every lane ends with the wave's sum)
  workgroup  (w0 + w1) + (w2 + w3)

How many loads a kernel keeps in flight (16, 8, one) is not part of the order.  tests/test_dbr_fold_twin.py pins
fold() to the C oracle's DBR dot up to 4097 partials; beyond that the GPU tests rest on fold() alone.

  fold(p)            the folded sum of the partials p (a float64 scalar)
  data_sets(nch, .)  the partial vectors the fold tests use, by name
"""
from __future__ import annotations

import numpy as np

LANES, WAVE = 256, 64
CHUNK = 4096

# every chunk count at which a lane's trip structure changes: one trip, the second trip (257), the 8-deep loop
# (1793 .. 3840), the 16-deep loop (3841 ..), a 16-deep trip followed by an 8-deep one, by a tail, by both, several
# 16-deep trips (the 512 x 512 x 256 block's 16384 chunks) and those followed by 8-deep and tail trips
NCH = [1, 255, 256, 257, 1792, 1793, 2049, 3840, 3841, 4096, 4097, 4096 + 1793, 4096 + 2048 + 257, 16384,
       16384 + 3841]
NCH_THIN = [257, 1793, 3841, 4096 + 1793, 16384]


def fold(p) -> np.float64:
    p = np.ascontiguousarray(p, np.float64)
    trips = -(-p.size // LANES)
    padded = np.zeros(trips * LANES)                      # a lane past the end adds nothing on its last trip
    padded[:p.size] = p
    present = np.arange(trips * LANES).reshape(trips, LANES) < p.size
    acc = np.zeros(LANES)                                 # +0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for row, there in zip(padded.reshape(trips, LANES), present):
            acc = np.where(there, acc + row, acc)         # an absent partial is no add at all (+0.0 + -0.0 stays apart)
        v = acc.reshape(LANES // WAVE, WAVE)
        lane = np.arange(WAVE)
        off = WAVE // 2
        while off >= 1:
            v = v + v[:, lane ^ off]
            off >>= 1
        w = v[:, 0]
        return np.float64((w[0] + w[1]) + (w[2] + w[3]))


def order_set(nch: int, lane: int) -> np.ndarray:
    """Partials whose fold changes with ANY change of the order of one lane's adds that crosses a group of eight
    trips, whatever the other lanes do: only lane `lane` holds values (the others add +0.0, so the fold is that
    lane's sum exactly), and they are 1.0, then per trip k half an ulp of 1.0 (2^-53) or, where k % 8 == 0, a whole
    one (2^-52).  Added to a sum in [1, 2), half an ulp is a tie: it is dropped when the sum's last bit is even and
    rounds up when it is odd, and a whole ulp flips that bit -- so a group of eight taken backwards ends one ulp
    away from the group taken forwards, from either parity, and the first group (1.0 last instead of first) ends
    at 1 + 4 ulp instead of 1.0.  With mixed magnitudes a reordered lane changes the folded sum only now and then
    (one lane in 256, one rounding among many); with this set it always does."""
    lane = min(lane, nch - 1)
    p = np.zeros(nch)
    idx = np.arange(lane, nch, LANES)
    p[idx] = np.where(np.arange(idx.size) % 8 == 0, 2.0 ** -52, 2.0 ** -53)
    p[lane] = 1.0
    return p


NAMES = ("mixed", "negzero", "inf", "nan", "order0", "order255")


def data_sets(nch: int, seed: int, signed: bool = True) -> dict:
    """name -> nch partials.  mixed: magnitudes 1e-3 .. 1e3 (signs mixed unless signed is False: squares' partials);
    negzero: all -0.0 (the fold is +0.0: every lane starts at +0.0); inf: one +inf among the mixed ones; nan: one NaN
    among them (compared as NaN on both sides, guarded.assert_same_bits); order0, order255: order_set() in the
    first lane (the first to reach a deeper loop as the count grows) and in the last."""
    rng = np.random.default_rng(seed)
    mixed = 10.0 ** rng.uniform(-3, 3, nch)
    if signed:
        mixed *= rng.choice([-1.0, 1.0], nch)
    inf, nan = mixed.copy(), mixed.copy()
    inf[int(rng.integers(nch))] = np.inf
    nan[int(rng.integers(nch))] = np.nan
    return {"mixed": mixed, "negzero": np.full(nch, -0.0), "inf": inf, "nan": nan,
            "order0": order_set(nch, 0), "order255": order_set(nch, LANES - 1)}

"""The block16 rounding of a stored Krylov basis vector (MSP_BASIS_B16) and its GMRES twin (helper, not a test).

TEST INFRASTRUCTURE ONLY.  block16(v) is the rule of include/msplit.h in numpy -- frexp, ldexp, rint, clip, ldexp
per DBR chunk of 4096 elements -- and gmres is tests/basis_twin.py's solve with that rounding at the two places
where a basis vector is stored.  The device (msplit_cgs_basis.hip) is held to both bit for bit.
"""
from __future__ import annotations

from functools import partial

import numpy as np

import basis_twin as bt

CHUNK = 4096          # the DBR chunk (pyoracle's, MSK_DBR_CHUNK)
QMAX = 32767


def chunk_exponents(v):
    """Per chunk: frexp's exponent of max |v_i| (0 for a zero chunk), None where the chunk holds a NaN or an inf."""
    v = np.asarray(v, np.float64)
    out = []
    for lo in range(0, v.size, CHUNK):
        c = v[lo:lo + CHUNK]
        if not np.all(np.isfinite(c)):          # not through the maximum: fmax drops NaN
            out.append(None)
            continue
        M = np.max(np.abs(c))
        out.append(0 if M == 0.0 else int(np.frexp(M)[1]))
    return out


def quantise(v):
    """(q, E): the int16 values and the per-chunk exponents (None: non-finite chunk, q = 0) block16 stores."""
    v = np.asarray(v, np.float64)
    q = np.zeros(v.size, np.int16)
    E = chunk_exponents(v)
    with np.errstate(all="ignore"):
        for k, e in enumerate(E):
            lo = k * CHUNK
            if e is None:
                continue
            q[lo:lo + CHUNK] = np.clip(np.rint(np.ldexp(v[lo:lo + CHUNK], 15 - e)), -QMAX, QMAX).astype(np.int16)
    return q, E


def dequantise(q, E):
    s = np.empty(q.size, np.float64)
    with np.errstate(all="ignore"):
        for k, e in enumerate(E):
            lo = k * CHUNK
            s[lo:lo + CHUNK] = np.nan if e is None else np.ldexp(q[lo:lo + CHUNK].astype(np.float64), e - 15)
    return s


def block16(v):
    """rnd16(v): what a vector reads back as after being stored as block16.  The integers go through int16, as on
    the device, so a zero is +0.0 whatever the sign of the entry it came from."""
    return dequantise(*quantise(v))


gmres = partial(bt.gmres, rnd=block16)

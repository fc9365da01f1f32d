"""Crafted least-squares problems that send KSPLSQR down each of its termination branches (helper, not a test).

One definition for the CPU tests (oracle against the twins) and the GPU test (device against the oracle):
n = 4100 rows in the blocks [4096, 4] -- a full DBR chunk and a ragged one -- and s = 3 columns.  Each case is
(R, b, options, reasons): reasons[conv_test] is the KSPConvergedReason the case is named for, per convergence
test (0 default, 1 lsqr, 2 skip) it is run with.
"""
import numpy as np

from lsqr_names import ATOL, ATOL_NORMAL, DTOL, ITS, ITS_DIV, NANORINF, RTOL, RTOL_NORMAL

N, S, CUTS = 4100, 3, (4096, 4)


def _random():
    rng = np.random.default_rng(20261020)
    return rng.standard_normal((N, S)) @ np.diag([1.0, 0.3, 0.05]), rng.standard_normal(N)


def _units():
    R = np.zeros((N, S))
    R[0, 0] = R[1, 1] = R[4097, 2] = 1.0      # the third unit column sits in the ragged block
    return R


def case(name):
    R, b = _random()
    o = dict(max_it=12, rtol=1e-5, abstol=1e-50, divtol=1e4, exact_norm=0)
    if name == "nan_b":
        b[4098] = np.nan
        want = {0: NANORINF, 1: NANORINF}
    elif name == "inf_b":
        b[7] = -np.inf
        want = {0: NANORINF, 1: NANORINF}
    elif name == "nan_R":
        R[5, 1] = np.nan
        want = {0: NANORINF, 1: NANORINF}
    elif name == "inf_R":
        R[4099, 2] = np.inf
        want = {0: NANORINF, 1: NANORINF}
    elif name == "zero_R":                       # V = 0, alpha = 0, V * (1 / 0) = NaN
        R[:] = 0.0
        want = {0: NANORINF, 1: NANORINF}
    elif name == "orth_b":                       # R = two unit columns (and a zero one), b a third unit vector
        R = _units()
        R[:, 2] = 0.0
        b = np.zeros(N)
        b[4097] = 1.0
        want = {0: NANORINF, 1: NANORINF}
    elif name == "exact_one_step":               # beta == 0 after one step: phibar = 0 < abstol; skip goes on
        R = _units()
        b = np.zeros(N)
        b[0] = 2.0
        o.update(max_it=3)
        want = {0: ATOL, 1: ATOL, 2: NANORINF}
    elif name == "consistent":
        b = R @ np.array([1.0, -2.0, 0.5])
        o.update(max_it=50, rtol=1e-10)
        want = {0: RTOL}
    elif name == "atol_at_zero":
        o.update(abstol=1e3)
        want = {0: ATOL, 1: ATOL}
    elif name == "atol_normal":
        o.update(abstol=1e-3, rtol=0.0, max_it=50)
        want = {1: ATOL_NORMAL}
    elif name == "rtol_normal":
        o.update(max_it=50)
        want = {1: RTOL_NORMAL}
    elif name == "dtol_at_zero":
        o.update(divtol=0.5)
        want = {0: DTOL, 1: DTOL}
    elif name == "overflowing_norm":
        R, b = R * 1e200, b * 1e200
        want = {0: NANORINF, 1: NANORINF}
    elif name == "skip_its":
        o.update(max_it=5)
        want = {2: ITS}
    elif name == "max_it":
        o.update(max_it=4, rtol=1e-30)
        want = {0: ITS_DIV}
    else:
        raise KeyError(name)
    return R, b, o, want


NAMES = ("nan_b", "inf_b", "nan_R", "inf_R", "zero_R", "orth_b", "exact_one_step", "consistent", "atol_at_zero",
         "atol_normal", "rtol_normal", "dtol_at_zero", "overflowing_norm", "skip_its", "max_it")
RUNS = [(name, conv) for name in NAMES for conv in sorted(case(name)[3])]


def blocks(R, b, cuts=CUTS):
    e = np.cumsum((0,) + tuple(cuts))
    return [R[a:c] for a, c in zip(e[:-1], e[1:])], [b[a:c] for a, c in zip(e[:-1], e[1:])]

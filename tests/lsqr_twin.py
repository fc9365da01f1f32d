"""One KSPLSQR step, launcher by launcher, restated on the CPU (helper, not a test).

TEST INFRASTRUCTURE ONLY.  msp_lsqr_solve (ksp_lsqr.c) is a chain of launchers: the dense products of
msplit_dense.hip (mspi_dense_lsqr_onepass_p, mspi_dense_gemv_p, mspi_dense_scaled_dots_p, mspi_dense_colsumsq_p,
mspi_norm2sq) and the one-lane recurrence kernels of msplit_lsqr.hip (mspi_ls_start / first / beta / step /
onepass_step).  This module restates each of them in numpy from the oracle's primitives, independently of the
kernels:

  rows          oracle.dense_mult: per row ((0 + c0 a0) + c1 a1) + ...
  element-wise  numpy, one rounding per operation (numpy never contracts a * b + c)
  sums          oracle.dot(.., REDUCE_DBR), the device's reduction order, block sums added in block order from 0.0
  scalars       numpy float64 (IEEE: 1 / 0 = inf, 0 * inf = NaN), one statement per PETSc operation of
                KSPSolve_LSQR, KSPConvergedDefault, KSPLSQRConvergedDefault and KSPConvergedSkip

solve() chains them exactly as msp_lsqr_solve does and must give oracle.lsqr's record bit for bit
(tests/test_lsqr_twin.py); a GPU test hands solve() a callback and compares the device with the twin after every
single call (tests/test_gpu_lsqr_step.py).  A float block is promoted first (promote): (double)f is exact, so
every sum is the f64 sum over the promoted values.
"""
from __future__ import annotations

import functools

import numpy as np
import pyoracle as po

from lsqr_names import (ATOL, ATOL_NORMAL, CONV_LSQR, CONV_SKIP, DTOL, ITS, ITS_DIV, NANORINF, RTOL, RTOL_NORMAL,
                        STATE_DOUBLES, STATE_INTS, VECTORS)

F = np.float64
UNSET = F(np.nan)        # what a never-written output holds in the twin (the device: guarded.UNWRITTEN_BITS)


def _ieee(f):
    @functools.wraps(f)
    def g(*a, **k):
        with np.errstate(all="ignore"):
            return f(*a, **k)
    return g


@_ieee
def promote(R, precision="double"):
    """The values a block of this precision holds: "single" rounds each entry to float once."""
    R = np.asarray(R, np.float64)
    return R.astype(np.float32).astype(np.float64) if precision == "single" else R


def _dot(x, y):
    return F(po.dot(x, y, po.REDUCE_DBR)) if len(x) else F(0.0)


def _rows(R, coef):
    return po.dense_mult(R, coef) if R.shape[0] else np.zeros(0)


@_ieee
def _vecaxpy(y, nal, U, usc):
    """y + nal * (U * usc): VecAXPY over the stored-unscaled U, skipped for nal == 0 (PETSc) or no U."""
    if U is None or nal == 0.0:
        return y
    return y + F(nal) * (np.asarray(U, np.float64) * (F(1.0) if usc is None else F(usc)))


# ------------------------------------------------------------------------------------------- the dense launchers
def gemv(R, coef, nal=None, U=None, usc=None):
    """mspi_dense_gemv_p: (y, ||y||^2) with y = R coef + nal (U usc)."""
    y = _vecaxpy(_rows(R, coef), nal, U, usc)
    return y, _dot(y, y)


def onepass(R, V, nal, U, usc):
    """mspi_dense_lsqr_onepass_p: (U1, [||U1||^2, R^T U1]) with U1 = R V + nal (U usc), stored unscaled."""
    u1 = _vecaxpy(_rows(R, V), nal, U, usc)
    return u1, np.array([_dot(u1, u1)] + [_dot(R[:, v], u1) for v in range(R.shape[1])])


@_ieee
def scaled_dots(w, sc, R, write_back):
    """mspi_dense_scaled_dots_p: (wout, R^T w') with w' = w * sc when sc is given (VecScale); wout is w' with
    write_back, None in the deferred form (the next reader rescales)."""
    w = np.asarray(w, np.float64)
    ws = w if sc is None else w * F(sc)
    out = np.array([_dot(R[:, v], ws) for v in range(R.shape[1])])
    return (ws if sc is not None and write_back else None), out


def colsumsq(R):
    """mspi_dense_colsumsq_p: ||column j||^2."""
    return np.array([_dot(R[:, j], R[:, j]) for j in range(R.shape[1])])


def norm2sq(x):
    return _dot(x, x)


# ----------------------------------------------------------------------------------- the one-lane recurrence
def new_state(s, nblk, max_it=10000, rtol=1e-5, abstol=1e-50, divtol=1e4, exact_norm=0, conv_test=CONV_LSQR,
              hist_cap=None, **over):
    """The state msp_lsqr_solve pushes (zeroed but for the options), V, V1, W, hist never written, X as given to
    the solve (here: never written; mspi_ls_start zeroes it)."""
    st = {f: 0 for f in STATE_INTS}
    st.update({f: F(0.0) for f in STATE_DOUBLES})
    st.update(max_it=int(max_it), conv_test=int(conv_test), exact_norm=int(exact_norm), s=int(s), nblk=int(nblk),
              hist_cap=int(max_it) + 2 if hist_cap is None else int(hist_cap), rtol=F(rtol), abstol=F(abstol),
              divtol=F(divtol))
    for v in ("V", "V1", "W", "X"):
        st[v] = np.full(s, UNSET)
    st["hist"] = np.full(st["hist_cap"], UNSET)
    for k, v in over.items():
        assert k in st, k
        st[k] = np.array(v, np.float64) if k in VECTORS else (int(v) if k in STATE_INTS else F(v))
    return st


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def _bad(v):
    return bool(np.isnan(v) or np.isinf(v))


def _bsum(g, j):
    t = F(0.0)
    for b in range(g.shape[0]):
        t = t + g[b, j]
    return t


def _snorm(v):
    t = F(0.0)
    for a in v:
        t = t + a * a
    return np.sqrt(t)


def _scale(v, a):          # VecScale
    if a == 0.0:
        return np.zeros(len(v))
    return v if a == 1.0 else v * a


def _axpy(y, a, x):        # VecAXPY
    return y if a == 0.0 else y + a * x


def _aypx(y, a, x):        # VecAYPX
    if a == 0.0:
        return x.copy()
    return y + x if a == 1.0 else x + a * y


def _log(st, r):
    if st["nhist"] < st["hist_cap"]:
        st["hist"][st["nhist"]] = r
    st["nhist"] += 1


def _converged(st, n, rnorm):
    st["reason"] = 0
    if st["conv_test"] == CONV_SKIP:                                     # KSPConvergedSkip
        if n >= st["max_it"]:
            st["reason"] = ITS
        return
    if n == 0:                                                           # KSPConvergedDefault, zero guess
        st["rnorm0"] = rnorm
        t = st["rtol"] * rnorm
        st["ttol"] = st["abstol"] if t < st["abstol"] else t             # PetscMax
    if _bad(rnorm):
        st["reason"] = NANORINF
    elif rnorm <= st["ttol"]:
        st["reason"] = ATOL if rnorm < st["abstol"] else RTOL
    elif rnorm >= st["divtol"] * st["rnorm0"]:
        st["reason"] = DTOL
    if st["conv_test"] != CONV_LSQR or n == 0 or st["reason"]:
        return
    if st["arnorm"] < st["abstol"]:                                      # KSPLSQRConvergedDefault
        st["reason"] = ATOL_NORMAL
    elif st["arnorm"] < st["rtol"] * st["anorm"] * rnorm:
        st["reason"] = RTOL_NORMAL


def _g(g, nblk, m):
    return np.asarray(g, np.float64).reshape(nblk, m)


def _stop(st, reason=None):
    if reason is not None:
        st["reason"] = reason
    st["stop"] = 1


@_ieee
def ls_start(st, g):
    """mspi_ls_start: g = ||b_k||^2 per block.  x = 0, rnorm = ||b||, the n = 0 test, U's scale 1 / beta."""
    if st["stop"]:
        return
    st["X"] = np.zeros(st["s"])
    rnorm = np.sqrt(_bsum(_g(g, st["nblk"], 1), 0))
    st["rnorm"] = rnorm
    if _bad(rnorm):                                                      # KSPCheckNorm: before the history entry
        return _stop(st, NANORINF)
    st["its"] = 0
    _log(st, rnorm)
    _converged(st, 0, rnorm)
    if st["reason"]:
        return _stop(st)
    st["beta"] = rnorm
    st["uscale"] = F(1.0) / rnorm


@_ieee
def ls_first(st, g, gfrob=None):
    """mspi_ls_first: g = R_k^T u per block, gfrob = the blocks' column sums of squares (exact_norm)."""
    if st["stop"]:
        return
    s, nb = st["s"], st["nblk"]
    g = _g(g, nb, s)
    V = np.array([_bsum(g, j) for j in range(s)])
    alpha = _snorm(V)
    V = _scale(V, F(1.0) / alpha)
    st["V"], st["W"] = V, V.copy()
    if st["exact_norm"] and gfrob is not None:                           # MatNorm(NORM_FROBENIUS), DBR order
        gf = _g(gfrob, nb, s)
        t = F(0.0)
        for b in range(nb):
            tb = F(0.0)
            for j in range(s):
                tb = tb + gf[b, j]
            t = t + tb
        st["anorm"] = np.sqrt(t)
    else:
        st["anorm"] = F(0.0)
    st["arnorm"] = alpha * st["beta"]
    st["phibar"], st["rhobar"] = st["beta"], alpha
    st["alpha"], st["nalpha"] = alpha, -alpha
    st["i"] = 0


def _beta(st, bsq):
    """beta = ||U1|| from its squared norm; False when the solve ends here."""
    beta = np.sqrt(bsq)
    if _bad(beta):
        _stop(st, NANORINF)
        return False
    st["beta"] = beta
    if beta > 0.0:
        st["uscale"] = F(1.0) / beta
        if not st["exact_norm"]:
            st["anorm"] = np.sqrt(st["anorm"] * st["anorm"] + st["alpha"] * st["alpha"] + beta * beta)
    else:
        st["uscale"] = F(1.0)                                            # VecScale skipped
    return True


def _rest_of_step(st, V1):
    """From V1 = R^T U1 (scaled one way or the other) to the convergence test: KSPSolve_LSQR's loop body."""
    beta = st["beta"]
    V1 = _axpy(V1, -beta, st["V"])
    st["V1"] = V1
    alpha = _snorm(V1)
    if _bad(alpha):
        return _stop(st, NANORINF)
    V1 = _scale(V1, F(1.0) / alpha)
    st["V1"] = V1
    rhobar = st["rhobar"]
    rho = np.sqrt(rhobar * rhobar + beta * beta)
    c = rhobar / rho
    sn = beta / rho
    theta = sn * alpha
    st["rhobar"] = -c * alpha
    phi = c * st["phibar"]
    st["phibar"] = sn * st["phibar"]
    tau = sn * phi
    st["X"] = _axpy(st["X"], phi / rho, st["W"])
    st["W"] = _aypx(st["W"], -theta / rho, V1)
    st["arnorm"] = alpha * np.abs(tau)
    rnorm = st["phibar"]
    st["rnorm"] = rnorm
    st["its"] += 1
    _log(st, rnorm)
    _converged(st, st["i"] + 1, rnorm)
    st["alpha"] = alpha
    if st["reason"]:
        return _stop(st)
    st["V"] = V1.copy()                                                  # SWAP(V1, V)
    st["i"] += 1
    st["nalpha"] = -alpha
    if st["i"] >= st["max_it"]:
        _stop(st, ITS_DIV)


@_ieee
def ls_beta(st, g):
    """mspi_ls_beta: g = ||U1_k||^2 per block."""
    if st["stop"]:
        return
    _beta(st, _bsum(_g(g, st["nblk"], 1), 0))


@_ieee
def ls_step(st, g):
    """mspi_ls_step: g = R_k^T (U1_k / beta) per block (PETSc's order: VecScale, then MatMultTranspose)."""
    if st["stop"]:
        return
    g = _g(g, st["nblk"], st["s"])
    _rest_of_step(st, np.array([_bsum(g, j) for j in range(st["s"])]))


@_ieee
def ls_onepass_step(st, g):
    """mspi_ls_onepass_step: g = [||U1_k||^2 | R_k^T U1_k] per block; V1 = (R^T U1) * (1 / beta), left unscaled
    when beta == 0."""
    if st["stop"]:
        return
    s = st["s"]
    g = _g(g, st["nblk"], s + 1)
    if not _beta(st, _bsum(g, 0)):
        return
    V1 = np.array([_bsum(g, 1 + j) for j in range(s)])
    st["V1"] = V1
    if st["beta"] > 0.0:
        V1 = _scale(V1, st["uscale"])
    _rest_of_step(st, V1)


# ----------------------------------------------------------------------------------------------- the whole solve
def solve(Rs, bs, precisions=None, onepass_step=1, on=None, max_steps=None, **opts):
    """msp_lsqr_solve's chain of launchers (DBR order, deferred VecScale) over the row blocks Rs, bs.  Returns
    (x, record) in oracle.lsqr's form plus "state".  on(call, k, st, writes, i) is called after every twin
    call: call names the launcher, k the block (None for a one-lane kernel), st the twin's state after it, i the
    step (None before the loop) and writes
    what the call stored, {name: array} with names "U<slot>_<k>", "g", "frob" (g and frob: (offset, values)).
    max_steps cuts the loop short (a test that walks only a few steps)."""
    nb = len(Rs)
    prec = list(precisions or ["double"] * nb)
    Rs = [promote(R, p) for R, p in zip(Rs, prec)]
    bs = [np.asarray(b, np.float64) for b in bs]
    s = Rs[0].shape[1]
    st = new_state(s, nb, **opts)
    on_ = on or (lambda *a: None)
    step = [None]
    on = lambda call, k, st_, writes: on_(call, k, st_, writes, step[0])   # noqa: E731
    live = lambda: not st["stop"]                                        # noqa: E731

    g = np.zeros(nb)
    for k in range(nb):                                                  # mspi_norm2sq takes no stop flag
        g[k] = norm2sq(bs[k])
        on("norm2sq", k, st, {"g": (k, g[k:k + 1])})
    ls_start(st, g)
    on("start", None, st, {})
    frob = None
    if st["exact_norm"]:
        frob = np.zeros((nb, s))
        for k in range(nb):                                              # nor does mspi_dense_colsumsq_p
            frob[k] = colsumsq(Rs[k])
            on("colsumsq", k, st, {"frob": (k * s, frob[k])})
    U = [[None] * nb, [None] * nb]
    g = np.zeros((nb, s))
    for k in range(nb):
        w = {}
        if live():
            U[0][k], g[k] = scaled_dots(bs[k], st["uscale"], Rs[k], True)
            w = {f"U0_{k}": U[0][k], "g": (k * s, g[k])}
        on("dots0", k, st, w)
    ls_first(st, g, frob)
    on("first", None, st, {})

    nsteps = st["max_it"] if st["max_it"] > 0 else 1
    if max_steps is not None:
        nsteps = min(nsteps, max_steps)
    for i in range(nsteps):
        step[0] = i
        a, a1 = i & 1, 1 - (i & 1)
        usc = (lambda: st["uscale"]) if i > 0 else (lambda: None)
        if onepass_step:
            g = np.zeros((nb, s + 1))
            for k in range(nb):
                w = {}
                if live():
                    U[a1][k], g[k] = onepass(Rs[k], st["V"], st["nalpha"], U[a][k], usc())
                    w = {f"U{a1}_{k}": U[a1][k], "g": (k * (s + 1), g[k])}
                on("onepass", k, st, w)
            ls_onepass_step(st, g)
            on("onepass_step", None, st, {})
        else:
            g = np.zeros(nb)
            for k in range(nb):
                w = {}
                if live():
                    U[a1][k], g[k] = gemv(Rs[k], st["V"], st["nalpha"], U[a][k], usc())
                    w = {f"U{a1}_{k}": U[a1][k], "g": (k, g[k:k + 1])}
                on("gemv", k, st, w)
            ls_beta(st, g)
            on("beta", None, st, {})
            g = np.zeros((nb, s))
            for k in range(nb):
                w = {}
                if live():
                    _, g[k] = scaled_dots(U[a1][k], st["uscale"], Rs[k], False)
                    w = {"g": (k * s, g[k])}
                on("dots", k, st, w)
            ls_step(st, g)
            on("step", None, st, {})
        if st["stop"] and ((i + 1) % 8 == 0 or max_steps is None):       # the host looks once per chunk of 8
            break
    n = min(st["nhist"], st["hist_cap"])
    return st["X"].copy(), {"its": st["its"], "reason": st["reason"], "rnorm": float(st["rnorm"]),
                            "arnorm": float(st["arnorm"]), "anorm": float(st["anorm"]),
                            "hist": st["hist"][:n].copy(), "state": st}

"""A Python restatement of the SMSM-global loop (synchronous-multisplitting-synchronous-minimization-global.c:288-363)
from the oracle's primitives, with a hook on R = A S.

The oracle's own orc_smsm_solve runs the loop in C and cannot round R.  This twin runs the same steps -- s times
{rhs_i = b_i - A_ij x_j, inner GMRES, exchange, S(:, k) = x}, R = A S, alpha = LSQR(R, b), x = S alpha, the stop test
on the LSQR residual -- with pyoracle's gmres / Mat.mult / Mat.residual / lsqr / dense_mult / final_residual_norm in
DBR mode, and applies rnd to R before the LSQR reads it.  rnd = identity must reproduce orc_smsm_solve bit for bit
(tests/test_minim_twin.py pins that); rnd = f32 is what -msplit_minimization_precision single computes: R stored as
float, every sum f64 over the promoted values.
"""
import numpy as np


def identity(R):
    return R


def f32(R):
    """Each entry rounded to float once (nearest even, gradual underflow, overflow to +-inf) and promoted."""
    with np.errstate(over="ignore"):
        return R.astype(np.float32).astype(np.float64)


def _block_rows(po, dim, nx, ny, nz, nb, b):
    N = nx * ny * nz
    rows = N // nb
    if dim == 3:
        ppb = nz // nb
        return po.poisson3d_rows(nx, ny, nz, b * ppb, (b + 1) * ppb)
    return po.poisson2d_rows(nx, ny, b * rows, (b + 1) * rows)


def smsm_global(po, dim, nx, ny, nz, nb, s, rtol, inner: dict, outer: dict, atol=1e-100, max_outer=1000,
                rnd=identity):
    """The record of pyoracle.smsm_solve (DBR), with R = rnd(A S)."""
    mode = po.REDUCE_DBR
    nz = nz if dim == 3 else 1
    N = nx * ny * nz
    rows = N // nb
    blocks = []
    for b in range(nb):
        r0, r1 = b * rows, (b + 1) * rows
        Ab = _block_rows(po, dim, nx, ny, nz, nb, b)
        Aii, Aoff = po.split(Ab, r0, r1)
        blocks.append(dict(r0=r0, r1=r1, Ab=Ab, Aii=Aii, Aoff=Aoff, b=Ab.mult(np.ones(N))))
    Abs = [blk["Ab"] for blk in blocks]
    bs = [blk["b"] for blk in blocks]
    x = np.zeros(N)
    norm0 = po.final_residual_norm(Abs, x, bs, mode)                                  # :280
    iopts = dict(inner, guess_nonzero=1, uirnorm=1, reduce_mode=mode)
    oopts = dict(outer, reduce_mode=mode)
    hist, lsqr_its, lsqr_reason, inner_its = [], [], [], []
    outer_its = 0
    while True:
        S = np.zeros((N, s), order="F")
        its_outer = []
        for k in range(s):
            rhs = [blk["Aoff"].residual(blk["b"], x) for blk in blocks]                # updateLocalRHS
            its = []
            xn = x.copy()
            for blk, r in zip(blocks, rhs):
                xb, g = po.gmres(blk["Aii"], r, x0=x[blk["r0"]:blk["r1"]], **iopts)    # inner_solver
                xn[blk["r0"]:blk["r1"]] = xb
                its.append(g["its"])
            x = xn                                                                     # the exchange
            its_outer.append(its)
            S[:, k] = x                                                                # MatSetValuesLocal(S, .., k, x)
        Rs = []
        for blk in blocks:                                                             # R = A S (:325-327)
            R = np.stack([blk["Ab"].mult(np.ascontiguousarray(S[:, k])) for k in range(s)], axis=1)
            Rs.append(rnd(R))
        alpha, lr = po.lsqr(Rs, bs, **oopts)                                           # outer_solver_norm_equation
        x = po.dense_mult(S, alpha)                                                    # x_minimized = S alpha
        norm = lr["rnorm"]
        hist.append(norm)
        lsqr_its.append(lr["its"])
        lsqr_reason.append(lr["reason"])
        inner_its.append(its_outer)
        outer_its += 1
        if norm <= max(atol, rtol * norm0):                                            # :342-347
            break
        if max_outer > 0 and outer_its >= max_outer:
            break
    return {"outer_its": outer_its, "norm0": norm0, "hist": np.array(hist), "lsqr_its": np.array(lsqr_its),
            "lsqr_reason": np.array(lsqr_reason), "inner_its": np.array(inner_its).reshape(outer_its, s, nb), "x": x,
            "final_norm": po.final_residual_norm(Abs, x, bs, mode), "error": po.norm2(-1.0 * np.ones(N) + x, mode)}

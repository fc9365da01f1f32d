"""IEEE edge values through the product routes and the vector kernels, bit for bit against the oracle.

The routes and kernels of test_gpu_guarded.py at one lead, with values planted into the SEED data: -0.0 (a whole
vector, and in runs), the subnormals 5e-324, -5e-324 and 1e-310, +-1e308 (so that sums overflow), +-inf and one
NaN.  The oracle runs the same statements under -ffp-contract=off, so it defines the expected bits; where both
sides are NaN only that is compared (same_bits).  For the box routes each inf / NaN is placed, in turn, at a row
one of whose neighbours is absent -- i = 0, i = nx - 1, the first and last y line, the first and last plane,
row 0, row n - 1: a neighbour read across a line or plane edge, or a mask applied by multiplication instead of
selection, then shows as a NaN or an inf in a row where the oracle has a number.

Every case generator below needs no GPU, and every case asserts that its reference holds at least one finite
entry: a reference that is all NaN would prove nothing.
"""
import numpy as np
import pytest

from guarded import Guarded, assert_same_bits, check_all
from medane_tchakorom_ufc_thesis_repository_amd.petsc import Mat
from test_gpu_guarded import (ROUTES, build_route, products_guarded, rows_guarded, rows_oracle, rows_problem)
from test_gpu_kernels import rng

pytestmark = pytest.mark.gpu

LEAD = 514                       # 16-byte aligned only: the stricter of the two
TINY = (5e-324, -5e-324, 1e-310)
HUGE = (1e308, -1e308)
SINGLES = (np.inf, -np.inf, np.nan)


def planted(base, r):
    """{name: vector}: base with -0.0 (everywhere, and in runs of five), subnormals and +-1e308 planted."""
    n = base.size
    out = {"negzero-all": np.full(n, -0.0)}
    v = base.copy()
    v[(np.arange(n) // 5) % 3 == 0] = -0.0
    out["negzero-runs"] = v
    v = base.copy()
    at = r.choice(n, max(1, n // 4), replace=False)
    v[at] = r.choice(TINY, at.size)
    out["subnormal"] = v
    v = base.copy()
    at = r.choice(n, max(1, n // 8), replace=False)
    v[at] = r.choice(HUGE, at.size)
    if n > 2:
        v[n // 2:n // 2 + 2] = 1e308          # two neighbours of one sign: their sum overflows
    out["huge"] = v
    return out


def with_one(base, at, value):
    v = base.copy()
    v[at] = value
    return v


def _finite(*refs):
    return all(np.isfinite(np.atleast_1d(a)).any() for a in refs)


# ------------------------------------------------------------------------------------------------ product routes
def edge_rows(nx, ny, nz):
    """Rows of an nx x ny x nz box one of whose neighbours is absent."""
    at = lambda i, j, k: (k * ny + j) * nx + i                                             # noqa: E731
    return {"i=0": at(0, ny // 2, nz // 2), "i=nx-1": at(nx - 1, ny // 2, nz // 2),
            "first-line": at(nx // 2, 0, nz // 2), "last-line": at(nx // 2, ny - 1, nz // 2),
            "first-plane": at(nx // 2, ny // 2, 0), "last-plane": at(nx // 2, ny // 2, nz - 1),
            "row-0": 0, "row-n-1": nx * ny * nz - 1}


def product_cases(route, O):
    """(name, x, b) of every planted case of a route."""
    r = rng()
    nr, nc = O.shape
    x, b = r.uniform(-1, 1, nc), r.uniform(-1, 1, nr)
    pb = planted(b, r)
    for name, px in planted(x, r).items():
        yield name, px, pb[name] if name.startswith("negzero") else b
    if route.box:
        nx, ny, nz, off = route.box
        where = {k: off + v for k, v in edge_rows(nx, ny, nz).items()}
    else:
        where = {"col-0": 0, "col-mid": nc // 2, "col-last": nc - 1}
    for k, at in where.items():
        for value in SINGLES:
            yield f"{value} at {k}", with_one(x, at, value), b


@pytest.mark.parametrize("route", list(ROUTES))
def test_products_edge_values(ctx, oracle, route, monkeypatch):
    rt, A, O = build_route(ctx, oracle, route, monkeypatch)
    for name, x, b in product_cases(rt, O):
        refs = products_guarded(ctx, A, O, x, b, LEAD, rt.flags, f"{route}, {name}:")
        assert _finite(*refs), name


def rows_cases():
    n, m, rows, rp, col, val, b, h = rows_problem()
    r = rng()
    pb = planted(b, r)
    for name, ph in planted(h, r).items():
        yield name, pb[name] if name.startswith("negzero") else b, ph
    for k, at in (("first", col[0]), ("last", col[-1])):
        for value in SINGLES:
            yield f"{value} at the {k} listed row's column", b, with_one(h, at, value)
    yield "inf and -0.0 in b", with_one(with_one(b, rows[0], np.inf), rows[1], -0.0), h


def test_row_compressed_edge_values(ctx, oracle):
    n, m, rows, rp, col, val, _, _ = rows_problem()
    A = Mat.from_csr_rows(ctx, n, m, rows, rp, col, val)
    O = rows_oracle(oracle, n, m, rows, rp, col, val)
    for name, b, h in rows_cases():
        refs = rows_guarded(ctx, A, O, rows, b, h, LEAD)
        assert _finite(*refs), name


# ------------------------------------------------------------------------------------------------ vector kernels
def vector_variants(n, r):
    """{name: vector}: the planted vectors and one inf / -inf / NaN each at the first, a middle and the last entry."""
    base = r.uniform(-1, 1, n)
    out = planted(base, r)
    for value, at in zip(SINGLES, (0, n // 2, n - 1)):
        out[f"{value} at {at}"] = with_one(base, at, value)
    return base, out


ALPHAS = (0.37, -0.0, 5e-324, 1e308)   # an inf or NaN factor leaves no number in the result


def blas1_cases(n):
    """(name, op, x, y, alpha, reference): op(w, X, Y, alpha) runs on Vecs, w the output or the in-place vector."""
    r = rng()
    base, xs = vector_variants(n, r)
    ys = planted(r.uniform(-1, 1, n), r)
    ys["plain"] = r.uniform(-1, 1, n)
    with np.errstate(all="ignore"):
        for xn, x in xs.items():
            y = ys[xn] if xn in ys else ys["plain"]
            yield f"copy {xn}", "copy", x, y, None, x
            for a in ALPHAS:
                yield f"scale {xn} by {a}", "scale", x, y, a, x * a
                yield f"aypx {a}, {xn}", "aypx", x, y, a, x + a * y
                if a != 0.0:   # daxpy returns for da == 0 and VecWAXPY copies y (msp_vec_axpy, msp_vec_waxpy)
                    yield f"axpy {a}, {xn}", "axpy", x, y, a, y + a * x
                    yield f"waxpy {a}, {xn}", "waxpy", x, y, a, y + a * x
            yield f"waxpy 1, {xn}", "waxpy", x, y, 1.0, y + x
            yield f"waxpy -1, {xn}", "waxpy", x, y, -1.0, y - x
            yield f"waxpy -0.0, {xn}", "waxpy", x, y, -0.0, y


def _run_blas1(ctx, op, x, y, alpha):
    X, Y = Guarded.input(ctx, x, LEAD), Guarded.input(ctx, y, LEAD)
    W = Guarded.output(ctx, x.size, LEAD)
    if op == "copy":
        X.vec.copy(W.vec)
    elif op == "scale":
        X.vec.scale(alpha)
        W = X
    elif op == "aypx":                      # y <- x + alpha y
        Y.vec.aypx(alpha, X.vec)
        W = Y
    elif op == "axpy":                      # y <- y + alpha x
        Y.vec.axpy(alpha, X.vec)
        W = Y
    else:                                   # w <- y + alpha x
        W.vec.waxpy(alpha, X.vec, Y.vec)
    check_all(X, Y, W)
    return W.get_array()


@pytest.mark.parametrize("n", [257, 4097])
def test_blas1_edge_values(ctx, n):
    for name, op, x, y, alpha, ref in blas1_cases(n):
        assert _finite(ref), name
        assert_same_bits(_run_blas1(ctx, op, x, y, alpha), ref, name)


def dot_cases(oracle, n):
    """(name, x, y, dot, norm): every pair of variants that leaves the norm or the dot finite or not -- the oracle
    says which; x = y for the self-dot."""
    r = rng()
    _, xs = vector_variants(n, r)
    y = r.uniform(-1, 1, n)
    for xn, x in xs.items():
        yield xn, x, y, oracle.dot(x, y, oracle.REDUCE_DBR), oracle.norm2(x, oracle.REDUCE_DBR)
    x = xs["subnormal"]
    yield "subnormal twice", x, xs["negzero-runs"], oracle.dot(x, xs["negzero-runs"], oracle.REDUCE_DBR), \
        oracle.norm2(x, oracle.REDUCE_DBR)


@pytest.mark.parametrize("n", [3, 4097, 8192 + 77])
def test_dot_norm_edge_values(ctx, oracle, n):
    finite = 0
    for name, x, y, d, nrm in dot_cases(oracle, n):
        X, Y = Guarded.input(ctx, x, LEAD), Guarded.input(ctx, y, LEAD)
        assert_same_bits(X.vec.dot(Y.vec), d, f"dot, {name}")
        assert_same_bits(X.vec.norm(), nrm, f"norm, {name}")
        check_all(X, Y)
        finite += int(np.isfinite(d)) + int(np.isfinite(nrm))
    assert finite >= 8       # the -0.0 and subnormal cases at the least


def _spread(V, variants):
    """V with the variants planted over its vectors, spread over the groups of four (the first one wins a vector)."""
    Vp, taken = list(V), set()
    for k, name in zip(np.linspace(0, len(V) - 1, len(variants)).astype(int).tolist(), variants):
        if k not in taken:
            Vp[k] = variants[name]
            taken.add(k)
    return Vp


def mdot_cases(oracle, n, nv):
    """(name, w, V, reference): planted values in w with plain V, and in single vectors of V with a plain w, so the
    other dots of the same launch stay numbers."""
    r = rng()
    wbase, ws = vector_variants(n, r)
    V = [r.uniform(-1, 1, n) for _ in range(nv)]
    for name in ("negzero-all", "negzero-runs", "subnormal"):
        yield f"w {name}", ws[name], V, oracle.mdot(ws[name], V, oracle.REDUCE_DBR)
    # +-1e308 at four places only: some of the nv sums overflow and some do not (a w with hundreds of them leaves
    # no finite dot at all)
    at = r.choice(n, min(n, 4), replace=False)
    wh = with_one(wbase, at, r.choice(HUGE, at.size))
    yield "w huge", wh, V, oracle.mdot(wh, V, oracle.REDUCE_DBR)
    _, vs = vector_variants(n, r)
    Vp = _spread(V, vs)
    yield "V planted", wbase, Vp, oracle.mdot(wbase, Vp, oracle.REDUCE_DBR)


@pytest.mark.parametrize("nv", [1, 5, 33])
@pytest.mark.parametrize("n", [1, 4097])
def test_mdot_edge_values(ctx, oracle, n, nv):
    for name, w, V, ref in mdot_cases(oracle, n, nv):
        assert _finite(ref), name
        W, Vg = Guarded.input(ctx, w, LEAD), [Guarded.input(ctx, v, LEAD) for v in V]
        assert_same_bits(W.vec.mdot([g.vec for g in Vg]), ref, f"mdot, {name}")
        check_all(W, *Vg)


def maxpy_cases(oracle, n, nv):
    """(name, w, a, V, reference): planted w, planted vectors of V (an inf or a NaN reaches one entry each), and
    coefficients -0.0, 5e-324 and 1e308."""
    r = rng()
    wbase, ws = vector_variants(n, r)
    V = [r.uniform(-1, 1, n) for _ in range(nv)]
    a = r.standard_normal(nv)
    with np.errstate(all="ignore"):
        for name, w in ws.items():
            yield f"w {name}", w, a, V, oracle.maxpy(w, a, V)
        _, vs = vector_variants(n, r)
        Vp = _spread(V, vs)
        yield "V planted", wbase, a, Vp, oracle.maxpy(wbase, a, Vp)
        ap = a.copy()
        ks = sorted(set(np.linspace(0, nv - 1, 3).astype(int).tolist()))
        ap[ks] = (-0.0, 5e-324, 1e308)[:len(ks)]
        yield "coefficients planted", ws["negzero-runs"], ap, V, oracle.maxpy(ws["negzero-runs"], ap, V)
        yield "coefficients planted, V planted", wbase, ap, Vp, oracle.maxpy(wbase, ap, Vp)


@pytest.mark.parametrize("nv", [1, 3, 5, 33])
@pytest.mark.parametrize("n", [7, 4099])
def test_maxpy_edge_values(ctx, oracle, n, nv):
    for name, w, a, V, ref in maxpy_cases(oracle, n, nv):
        assert _finite(ref), name
        W, Vg = Guarded.input(ctx, w, LEAD), [Guarded.input(ctx, v, LEAD) for v in V]
        W.vec.maxpy(a, [g.vec for g in Vg])
        assert_same_bits(W.get_array(), ref, f"maxpy, {name}")
        check_all(W, *Vg)

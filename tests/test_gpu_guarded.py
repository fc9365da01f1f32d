"""Every kernel family through the public API on guarded operands (tests/guarded.py).

Each Vec operand is a Guarded window at both leads -- 4 KiB aligned (512) and 16-byte but not 32-byte aligned (514),
all that msp_vec_create_with_array promises --, inputs with NaN guards around the window, outputs with a NaN
pattern in every word of it; dense blocks have their pad rows n .. lda poisoned.  The window holds the usual
uniform(-1, 1) data under SEED, so the result must be the oracle's bit for bit (same_bits) and whatever differs
comes from the guards alone: a store outside [0, n) (check), a read outside it that reaches a result (a NaN where
the oracle has a number), or an output word that was never written (assert_written).  The shapes are the smallest
that reach each path; every product route asserts the kernel or storage it was meant to reach.
"""
import numpy as np
import pytest

import basis_twin as bt
from guarded import LEADS, UNWRITTEN_BITS, DenseGuard, Guarded, assert_same_bits, check_all
from medane_tchakorom_ufc_thesis_repository_amd.petsc import KSP, LSQR, DenseMat, Mat, Options
from medane_tchakorom_ufc_thesis_repository_amd.utils import heterogeneous_poisson3d
from test_gpu_dv import MARCH_OFF, _banded, _unsymmetric
from test_gpu_gmres import _opts_str
from test_gpu_gmres import _random_csr as _dominant_csr
from test_gpu_kernels import _random_csr, rng, tuning
from test_gpu_lsqr import CASES as LSQR_CASES
from test_gpu_wfree import _L as _wfree_lib

pytestmark = pytest.mark.gpu

# msplit_kernels.h (MSK_TUNE_DV_NOELL, MSK_TUNE_GM_SPMV_MDOT): the two flags no test module names yet
DV_NOELL, GM_SPMV_MDOT = 32768, 2048
CHUNK = 4096


# ------------------------------------------------------------------------------------------------ vector kernels
@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4096, 4097])
def test_blas1_guarded(ctx, n, lead):
    """The eight msk_blas1 operations (set, copy, scale, axpy, aypx, waxpy with alpha 1, -1 and general) against
    numpy, as test_blas1_bitwise; the operations that write every entry start from an unwritten window."""
    r = rng()
    x, y = r.uniform(-1, 1, n), r.uniform(-1, 1, n)
    X, Y0 = Guarded.input(ctx, x, lead), Guarded.input(ctx, y, lead)

    def out_of(op, ref):
        W = Guarded.output(ctx, n, lead)
        op(W.vec)
        W.assert_written()
        assert_same_bits(W.get_array(), ref)
        W.check()

    def in_place(op, ref):
        Y = Guarded.input(ctx, y, lead)
        op(Y.vec)
        assert_same_bits(Y.get_array(), ref)
        Y.check()

    out_of(lambda w: w.set(-4.0), np.full(n, -4.0))
    out_of(lambda w: X.vec.copy(w), x)
    in_place(lambda v: v.scale(0.3), y * 0.3)
    in_place(lambda v: v.axpy(0.37, X.vec), y + 0.37 * x)
    in_place(lambda v: v.aypx(-1.25, X.vec), x + (-1.25) * y)
    out_of(lambda w: w.waxpy(1.0, X.vec, Y0.vec), y + x)
    out_of(lambda w: w.waxpy(-1.0, X.vec, Y0.vec), y - x)
    out_of(lambda w: w.waxpy(2.5, X.vec, Y0.vec), y + 2.5 * x)
    check_all(X, Y0)
    assert_same_bits(X.get_array(), x)
    assert_same_bits(Y0.get_array(), y)


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4096, 4097])
def test_copy_range_guarded(ctx, n, lead):
    """msp_vec_copy_range at even and odd source and destination offsets (an odd offset is 8-byte aligned only):
    the range arrives, every other word of the destination keeps its bits."""
    x = rng().uniform(-1, 1, n)
    X = Guarded.input(ctx, x, lead)
    for so, do in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 3), (3, 2), (2, 2)):
        m = n - max(so, do)
        if m < 1:
            continue
        W = Guarded.output(ctx, n, lead)
        X.vec.copy_range_to(so, W.vec, do, m)
        want = np.full(n, UNWRITTEN_BITS, np.uint64)
        want[do:do + m] = x[so:so + m].view(np.uint64)
        assert np.array_equal(W.get_array().view(np.uint64), want), (so, do, m)
        W.check()
    X.check()


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("n", [1, 2, 3, 511, 4095, 4096, 4097, 8192 + 77])
def test_dot_norm_guarded(ctx, oracle, n, lead):
    r = rng()
    x, y = r.uniform(-1, 1, n), r.uniform(-1, 1, n)
    X, Y = Guarded.input(ctx, x, lead), Guarded.input(ctx, y, lead)
    assert_same_bits(X.vec.dot(Y.vec), oracle.dot(x, y, oracle.REDUCE_DBR), "dot")
    assert_same_bits(X.vec.norm(), oracle.norm2(x, oracle.REDUCE_DBR), "norm")
    check_all(X, Y)


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("nv", [1, 3, 4, 5, 32, 33])
@pytest.mark.parametrize("n", [1, 4097])
def test_mdot_guarded(ctx, oracle, n, nv, lead):
    r = rng()
    w = r.uniform(-1, 1, n)
    V = [r.uniform(-1, 1, n) for _ in range(nv)]
    W, Vg = Guarded.input(ctx, w, lead), [Guarded.input(ctx, v, lead) for v in V]
    assert_same_bits(W.vec.mdot([g.vec for g in Vg]), oracle.mdot(w, V, oracle.REDUCE_DBR), "mdot")
    check_all(W, *Vg)


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("nv", [1, 2, 3, 4, 5, 8, 32, 33])
@pytest.mark.parametrize("n", [1, 7, 4096, 4098, 4099])
def test_maxpy_guarded(ctx, oracle, n, nv, lead):
    """n = 4098 and 4099: a partial chunk that ends on an even and on an odd element (the lane's two store guards,
    e < n and e + 1 < n, are each the last one taken)."""
    r = rng()
    w = r.uniform(-1, 1, n)
    V = [r.uniform(-1, 1, n) for _ in range(nv)]
    a = r.standard_normal(nv)
    W, Vg = Guarded.input(ctx, w, lead), [Guarded.input(ctx, v, lead) for v in V]
    W.vec.maxpy(a, [g.vec for g in Vg])
    assert_same_bits(W.get_array(), oracle.maxpy(w, a, V), "maxpy")
    check_all(W, *Vg)
    for g, v in zip(Vg, V):
        assert_same_bits(g.get_array(), v, "a MAXPY input")


# ------------------------------------------------------------------------------------------------ product routes
class Route:
    """One MatMult / MatResidual route: host(oracle) builds the oracle operator without a GPU, device(ctx, O) the
    library's; reached(A) asserts the kernel or storage the route is about.  assembly / flags: MSPLIT tuning
    flags while the matrix is built / while it is used; box = (nx, ny, nz, rows before the box in the column space)
    for the routes whose rows have stencil neighbours."""

    def __init__(self, host, device, reached, flags=0, assembly=0, box=None, env=None):
        self.host, self.device, self.reached = host, device, reached
        self.flags, self.assembly, self.box, self.env = flags, assembly, box, env or {}


def _from_csr(ctx, O):
    return Mat.from_csr(ctx, O.shape[0], O.shape[1], *O.arrays())


def _kernel(name, storage=None):
    def reached(A):
        assert A.spmv_kernel() == name, (A.spmv_kernel(), name)
        if storage:
            assert A.get_storage() == storage, (A.get_storage(), storage)
    return reached


def _storage(storage):
    def reached(A):
        assert A.get_storage() == storage, (A.get_storage(), storage)
    return reached


def _random_host(case):
    def host(oracle):
        r = rng()
        n = 1000 if case == "random" else 4099
        rp, col, val = _random_csr(n, 5000, 40 if case == "random" else 9, r)
        if case == "random-short":            # test_spmv_and_residual_bitwise's recipe: no row longer than 9
            lens = np.minimum(np.diff(rp), 9)
            rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            col = np.concatenate([np.sort(r.choice(5000, size=l, replace=False)) for l in lens]).astype(np.int32)
            val = r.standard_normal(rp[-1])
        else:
            assert np.diff(rp).max() == 3000  # the long row that forces the direct kernel
        return oracle.Mat.from_arrays(n, 5000, rp, col, val)
    return host


def _banded_host(offsets, n=1029, drop=0.3):
    """test_layout_and_rows_per_lane_variants_bitwise's matrices at n = 1029: two 1024-row blocks at four rows per
    lane, five at one, the last one ragged."""
    def host(oracle):
        rp, col, val = _banded(n, offsets, [-1.0, 4.0, 0.5], rng(), drop=drop)
        return oracle.Mat.from_arrays(n, n, rp, col, val)
    return host


def _ell(width):
    """k_spmv_ell at `width` codes per row: the longest row decides the width (dv_build)."""
    def reached(A):
        _kernel("k_spmv_ell", "dv")(A)
        longest = int(np.diff(A.get_csr()[0]).max())
        assert width // 2 < longest <= width or (width == 4 and longest <= 4), (longest, width)
    return reached


def _box_host(nx, ny, nz, lo=False, hi=False):
    return lambda oracle: oracle.poisson3d_rows(nx, ny, nz + lo + hi, int(lo), int(lo) + nz)


def _box_device(nx, ny, nz, lo=False, hi=False, matfree=False):
    def device(ctx, O):
        if matfree:
            return Mat.box_matfree(ctx, 3, nx, ny, nz, lo, hi)
        A = Mat.box_stencil_ext(ctx, 3, nx, ny, nz, lo, hi) if lo or hi else Mat.box_stencil(ctx, 3, nx, ny, nz)
        for got, want in zip(A.get_csr(), O.arrays()):
            assert np.array_equal(got, want)            # the oracle's operator is the device's
        return A
    return device


def _march(nx, ny, nz, chunk):
    def reached(A):
        _kernel("k_spmv_box_march", "dv")(A)
        assert ((nx * ny) % CHUNK == 0 and nx % 2 == 0 and nx <= 2048) == chunk   # march_chunk_ok: the tile taken
    return reached


def _box_route(nx, ny, nz, chunk, lo=False, hi=False):
    return Route(_box_host(nx, ny, nz, lo, hi), _box_device(nx, ny, nz, lo, hi), _march(nx, ny, nz, chunk),
                 box=(nx, ny, nz, nx * ny if lo else 0))


def _stencil_host(nx, ny, nz, unsym):
    def host(oracle):
        rp, col, val = heterogeneous_poisson3d(nx, ny, nz)
        if unsym:
            val = _unsymmetric(rp, col, val)
        return oracle.Mat.from_arrays(nx * ny * nz, nx * ny * nz, rp, col, val)
    return host


_RV_ENV = {"MSPLIT_RV_LAYOUT": "blocked", "MSPLIT_RV_SYM": "1", "MSPLIT_RV_SYM2": "1"}
_BANDED = [-40, -1, 0, 2, 33]
_W16 = [-900, -64, -9, -8, -3, -2, -1, 0, 1, 2, 3, 8, 64, 900]

ROUTES = {
    "csr-lds-dma": Route(_random_host("random-short"), _from_csr, _kernel("k_spmv_lds8", "csr")),
    "csr-direct": Route(_random_host("random"), _from_csr, _kernel("k_spmv_csr", "csr")),
    "empty": Route(lambda o: o.Mat.from_arrays(3, 7, np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0)),
                   _from_csr, _storage("csr")),          # its only possible defect: an unwritten y
    "dv-csr-order": Route(_banded_host(_BANDED), _from_csr, _kernel("k_spmv_dv", "dv"),
                          assembly=DV_NOELL),
    "ell-w4": Route(_banded_host([-7, 0, 1]), _from_csr, _ell(4)),
    # the `banded` recipe drops 30 % of its entries, so padding to 8 codes would add more than half of them and
    # dv_build keeps CSR-order codes; with 10 % dropped the same offsets take the 8-wide ELL layout
    "banded": Route(_banded_host(_BANDED), _from_csr, _kernel("k_spmv_dv", "dv")),
    "ell-w8": Route(_banded_host(_BANDED, drop=0.1), _from_csr, _ell(8)),
    # `w16` is dense enough for the ELL layout from about 3000 rows on (its +-900 entries are missing near the ends)
    "ell-w16": Route(_banded_host(_W16, n=3077), _from_csr, _ell(16)),
    "ell-box": Route(_box_host(37, 11, 9), _box_device(37, 11, 9), _ell(8), flags=MARCH_OFF, box=(37, 11, 9, 0)),
    "z-march-37x11x9": _box_route(37, 11, 9, False),
    "z-march-256x5x16": _box_route(256, 5, 16, False),
    "march-2d-100x37": Route(lambda o: o.poisson2d_rows(37, 100, 0, 3700),
                             lambda ctx, O: Mat.box_stencil(ctx, 2, 100, 37), _march(100, 37, 1, False),
                             box=(100, 1, 37, 0)),       # marched as an nx x 1 x ny box
    "chunk-march-64x64x3": _box_route(64, 64, 3, True),
    "chunk-march-2048x2x3": _box_route(2048, 2, 3, True),
    "halo-march-lo": _box_route(64, 64, 3, True, lo=True),
    "halo-march-hi": _box_route(64, 64, 3, True, hi=True),
    "halo-march-both": _box_route(64, 64, 3, True, lo=True, hi=True),
    "stencil-sym": Route(_stencil_host(64, 64, 2, False), _from_csr, _kernel("k_box_march_chunk_rv_sym", "stencil"),
                         box=(64, 64, 2, 0), env=_RV_ENV),
    "stencil-blocked-unsym": Route(_stencil_host(64, 64, 2, True), _from_csr,
                                   _kernel("k_box_march_chunk_rv", "stencil"), box=(64, 64, 2, 0), env=_RV_ENV),
    "matfree-7x5x4": Route(_box_host(7, 5, 4, True, True), _box_device(7, 5, 4, True, True, matfree=True),
                           _kernel("k_stencil_spmv", "none"), box=(7, 5, 4, 35)),
    "matfree-16x16x16": Route(_box_host(16, 16, 16, True, True), _box_device(16, 16, 16, True, True, matfree=True),
                              _kernel("k_stencil_spmv", "none"), box=(16, 16, 16, 256)),
}

_built = {}


def build_route(ctx, oracle, name, monkeypatch):
    """(route, A, O) of a named route, assembled once per session and never modified; the route's environment is
    set for the calling test."""
    route = ROUTES[name]
    for k, v in route.env.items():      # on every call: some of it is read per product, not at assembly
        monkeypatch.setenv(k, v)
    if name not in _built:
        O = route.host(oracle)
        with tuning(route.assembly):
            A = route.device(ctx, O)
        assert A.shape == O.shape
        _built[name] = (A, O)
    A, O = _built[name]
    with tuning(route.flags):
        route.reached(A)
    return route, A, O


def products_guarded(ctx, A, O, x, b, lead, flags=0, what=""):
    """MatMult and MatResidual on guarded operands: every row written, the oracle's bits, no guard touched, the
    inputs unchanged."""
    X, B = Guarded.input(ctx, x, lead), Guarded.input(ctx, b, lead)
    Y, R = Guarded.output(ctx, O.shape[0], lead), Guarded.output(ctx, O.shape[0], lead)
    with tuning(flags):
        A.mult(X.vec, Y.vec)
        A.residual(B.vec, X.vec, R.vec)
    Y.assert_written()
    R.assert_written()
    with np.errstate(all="ignore"):
        want_y, want_r = O.mult(x), O.residual(b, x)
    assert_same_bits(Y.get_array(), want_y, f"{what} MatMult (lead {lead})")
    assert_same_bits(R.get_array(), want_r, f"{what} MatResidual (lead {lead})")
    check_all(X, B, Y, R)
    assert_same_bits(X.get_array(), x, "x after the products")
    assert_same_bits(B.get_array(), b, "b after the products")
    return want_y, want_r


@pytest.mark.parametrize("route", list(ROUTES))
def test_matmult_and_residual_guarded(ctx, oracle, route, monkeypatch):
    rt, A, O = build_route(ctx, oracle, route, monkeypatch)
    r = rng()
    x, b = r.uniform(-1, 1, O.shape[1]), r.uniform(-1, 1, O.shape[0])
    for lead in LEADS:
        products_guarded(ctx, A, O, x, b, lead, rt.flags, route)


def rows_problem():
    """The row-compressed coupling matrix of test_residual_listed_equals_residual_where_r_holds_b at n = 5000 with
    70 listed rows: (n, m, rows, rowptr, col, val, b, h)."""
    r = rng()
    n, m = 5000, 300
    rows = np.sort(r.choice(n, 70, replace=False)).astype(np.int32)
    cnt = r.integers(1, 5, rows.size)
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    col = np.concatenate([np.sort(r.choice(m, c, replace=False)) for c in cnt]).astype(np.int32)
    val = r.uniform(-1, 1, col.size)
    return n, m, rows, rp, col, val, r.uniform(-1, 1, n), r.uniform(-1, 1, m)


def rows_oracle(oracle, n, m, rows, rp, col, val):
    """The same operator with every row spelled out (the unlisted ones empty)."""
    cnt = np.zeros(n, np.int64)
    cnt[rows] = np.diff(rp)
    return oracle.Mat.from_arrays(n, m, np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), col, val)


def rows_guarded(ctx, A, O, rows, b, h, lead):
    n = O.shape[0]
    B, H = Guarded.input(ctx, b, lead), Guarded.input(ctx, h, lead)
    Y, R = Guarded.output(ctx, n, lead), Guarded.output(ctx, n, lead)
    A.mult(H.vec, Y.vec)
    A.residual(B.vec, H.vec, R.vec)
    Y.assert_written()
    R.assert_written()
    with np.errstate(all="ignore"):
        want_y, want_r = O.mult(h), O.residual(b, h)
    assert_same_bits(Y.get_array(), want_y, "row-compressed MatMult")
    assert_same_bits(R.get_array(), want_r, "row-compressed MatResidual")
    L = Guarded.input(ctx, b, lead)                      # r already holds b: the unlisted rows keep their bits
    A.residual_listed(B.vec, H.vec, L.vec)
    assert_same_bits(L.get_array(), want_r, "residual_listed over b")
    U = Guarded.output(ctx, n, lead)                     # and they keep any other bits too
    A.residual_listed(B.vec, H.vec, U.vec)
    got = U.get_array()
    keep = np.ones(n, bool)
    keep[rows] = False
    assert_same_bits(got[rows], want_r[rows], "the listed rows")
    assert np.all(got[keep].view(np.uint64) == UNWRITTEN_BITS), "residual_listed wrote a row it does not list"
    check_all(B, H, Y, R, L, U)
    return want_y, want_r


def test_row_compressed_guarded(ctx, oracle):
    n, m, rows, rp, col, val, b, h = rows_problem()
    A = Mat.from_csr_rows(ctx, n, m, rows, rp, col, val)
    assert A.spmv_kernel() == "k_spmv_rows"
    O = rows_oracle(oracle, n, m, rows, rp, col, val)
    for lead in LEADS:
        rows_guarded(ctx, A, O, rows, b, h, lead)


# --------------------------------------------------------------------------------------------------------- GMRES
def _gmres_guarded(ctx, A, b, x0, optstr, lead):
    B, X = Guarded.input(ctx, b, lead), Guarded.input(ctx, x0, lead)
    ksp = KSP(ctx)
    ksp.set_operators(A)
    ksp.set_from_options(Options(optstr))
    ksp.solve(B.vec, X.vec)
    check_all(B, X)
    assert_same_bits(B.get_array(), b, "b after the solve")
    return X.get_array(), {"its": ksp.get_iteration_number(), "reason": ksp.get_converged_reason(),
                           "rnorm": ksp.get_residual_norm(), "hist": ksp.get_residual_history()}


def _same_solve(got, want, what):
    (xg, rg), (xw, rw) = got, want
    assert (rg["its"], rg["reason"]) == (rw["its"], rw["reason"]), what
    assert_same_bits(rg["hist"], rw["hist"], f"{what}: residual history")
    assert_same_bits(rg["rnorm"], rw["rnorm"], f"{what}: residual norm")
    assert_same_bits(xg, xw, f"{what}: x")


_SMALL = dict(restart=5, max_it=12, rtol=1e-30)


@pytest.mark.parametrize("case", ["box-wfree-march", "box-unmarched", "csr-spmv-mdot"])
def test_gmres_guarded(ctx, oracle, case):
    """KSPSolve with b and x guarded and a nonzero initial guess in x, against the oracle's DBR solve: the fused
    march step with the W-free MAXPY (planes of whole chunks), the unmarched fused kernels (k_box_spmv_mdot,
    k_box_maxpy) and the CSR step with the MatMult fused with the VecMDot (k_spmv_mdot)."""
    flags = 0
    if case == "csr-spmv-mdot":
        n = 5000
        rp, col, val = _dominant_csr(np.random.default_rng(2024), n, 8)
        O = oracle.Mat.from_arrays(n, n, rp, col, val)
        A = Mat.from_csr(ctx, n, n, rp, col, val)
        assert A.get_storage() == "csr"
        flags = GM_SPMV_MDOT
    else:
        nx, ny, nz = (64, 64, 3) if case == "box-wfree-march" else (37, 11, 9)
        O = oracle.poisson3d_rows(nx, ny, nz, 0, nz)
        A = Mat.box_stencil(ctx, 3, nx, ny, nz)
        n = O.shape[0]
        assert A.spmv_kernel() == "k_spmv_box_march"
        assert _wfree_lib().msk_box_wfree_fits(nx, nx * ny, n, 0) == 1
        assert ((nx * ny) % CHUNK == 0) == (case == "box-wfree-march")   # k_box_spmv_mdot_march or k_box_spmv_mdot
    r = rng()
    b, x0 = r.uniform(-1, 1, n), r.uniform(-1, 1, n)
    want = oracle.gmres(O, b, x0=x0, reduce_mode=oracle.REDUCE_DBR, guess_nonzero=1, **_SMALL)
    assert want[1]["its"] == _SMALL["max_it"]
    for lead in LEADS:
        ctx.set_timing(True)
        ctx.reset_kernel_stats()
        try:
            with tuning(flags):
                got = _gmres_guarded(ctx, A, b, x0, _opts_str(_SMALL, True), lead)
            fused = ctx.kernel_stats()["spmvdot"]["launches"]
        finally:
            ctx.set_timing(False)
        assert fused >= _SMALL["max_it"], f"{case}: the MatMult fused with the VecMDot ran {fused} times"
        _same_solve(got, want, f"{case} (lead {lead})")


F32_CASES = {
    "exact-chunk": ((16, 16, 16), dict(restart=5, max_it=12, rtol=1e-30)),       # n = 4096: one full chunk, no tail
    "chunks-and-tail": ((17, 16, 16), dict(restart=6, max_it=14, rtol=1e-30)),   # n = 4352
    "more-than-32-vectors": ((17, 16, 16), dict(restart=40, max_it=45, rtol=1e-30)),
}


@pytest.mark.parametrize("case", list(F32_CASES))
def test_gmres_f32_basis_guarded(ctx, oracle, case):
    """-msplit_basis_precision single (msplit_cgs_basis.hip) with b and x guarded, against the f32 twin: n an exact
    chunk multiple (the full-chunk path alone), a full chunk plus a tail, and more than 32 basis vectors over full
    chunks (MDot and BuildSoln in two groups)."""
    (nx, ny, nz), o = F32_CASES[case]
    O = oracle.poisson3d_rows(nx, ny, nz, 0, nz)
    A = Mat.box_stencil(ctx, 3, nx, ny, nz)
    n = O.shape[0]
    assert (n % CHUNK == 0) == (case == "exact-chunk") and n >= CHUNK
    r = rng()
    b, x0 = r.uniform(-1, 1, n), r.uniform(-1, 1, n)
    want = bt.gmres(O, b, x0=x0, rnd=bt.f32, guess_nonzero=1, **o)
    assert want[1]["its"] == o["max_it"]
    for lead in LEADS:
        got = _gmres_guarded(ctx, A, b, x0, _opts_str(o, True) + " -msplit_basis_precision single", lead)
        _same_solve(got, want, f"{case} (lead {lead})")


# --------------------------------------------------------------------------------------------------------- dense
def _box_of(n):
    return {3: (3, 1, 1), 4096: (16, 16, 16), 5000: (25, 20, 10), 8192: (64, 64, 2)}[n]


def _march_chunk_fits(nx, ny):
    """msk_march_chunk_fits: whether the chunk-tile march (and the column-by-column SpMM over it) takes the box."""
    import ctypes
    from medane_tchakorom_ufc_thesis_repository_amd import _lib
    f = _lib.load().msk_march_chunk_fits
    f.argtypes, f.restype = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int], ctypes.c_int
    return bool(f(nx, ny, 0))


@pytest.mark.parametrize("s", [1, 7, 20])
@pytest.mark.parametrize("n", [3, 4096, 5000])
def test_dense_guarded(ctx, oracle, n, s):
    """DenseMat.mult (with its row0 / n / yoff form), mult_transpose and gram over a block whose pad rows n .. lda
    are poisoned, on guarded vectors."""
    r = rng()
    S = np.asfortranarray(r.uniform(-1, 1, (n, s)))
    a, u = r.uniform(-1, 1, s), r.uniform(-1, 1, n)
    D = DenseMat.from_array(ctx, S)
    G = DenseGuard(ctx, D)
    G.poison()
    assert_same_bits(D.get_values(), S)
    for lead in LEADS:
        Av, U = Guarded.input(ctx, a, lead), Guarded.input(ctx, u, lead)
        # the whole block into a window of exactly n doubles: 16-byte aligned operands, so k_dense_gemv takes its
        # vector form -- grouped 16-byte column loads and stores over the full chunks (n = 4096: one full chunk;
        # 5000: one and a tail), at lead 514 on an output that is not 32-byte aligned
        Y = Guarded.output(ctx, n, lead)
        D.mult(Av.vec, Y.vec)
        Y.assert_written()
        assert_same_bits(Y.get_array(), oracle.dense_mult(S, a), "dense mult, whole block")
        Y.check()
        if n > 8:                                                       # an even row and an even offset: still pairs
            m = n - 4
            Y = Guarded.output(ctx, n + 2, lead)
            D.mult(Av.vec, Y.vec, row0=2, n=m, yoff=4)
            got = Y.get_array()
            assert np.all(np.delete(got, np.s_[4:4 + m]).view(np.uint64) == UNWRITTEN_BITS)
            assert_same_bits(got[4:4 + m], oracle.dense_mult(S[2:2 + m], a), "dense mult, even row0 and yoff")
            Y.check()
        # odd offsets (8-byte aligned only): the element-wise fallback
        Y = Guarded.output(ctx, n + 5, lead)
        D.mult(Av.vec, Y.vec, row0=0, n=n, yoff=5)                    # an odd offset into y
        got = Y.get_array()
        assert np.all(got[:5].view(np.uint64) == UNWRITTEN_BITS)
        assert_same_bits(got[5:], oracle.dense_mult(S, a), "dense mult")
        Y.check()
        if n > 4:                                                       # a row range from an odd row
            Y = Guarded.output(ctx, n, lead)
            D.mult(Av.vec, Y.vec, row0=1, n=n - 3, yoff=0)
            got = Y.get_array()
            assert np.all(got[n - 3:].view(np.uint64) == UNWRITTEN_BITS)
            assert_same_bits(got[:n - 3], oracle.dense_mult(S[1:n - 2], a), "dense mult of a row range")
            Y.check()
        T = Guarded.output(ctx, s, lead)
        D.mult_transpose(U.vec, T.vec)
        T.assert_written()
        assert_same_bits(T.get_array(), np.array([oracle.dot(S[:, j], u, oracle.REDUCE_DBR) for j in range(s)]),
                         "dense mult_transpose")
        Gm = DenseMat(ctx, s, s + 1)
        Gg = DenseGuard(ctx, Gm)
        Gg.poison(entries=True)
        D.gram(U.vec, Gm)
        Gg.assert_written()
        assert_same_bits(Gm.get_values(), oracle.dense_gram(S, u, oracle.REDUCE_DBR), "gram")
        check_all(Av, U, T, G, Gg)
    assert_same_bits(D.get_values(), S)


@pytest.mark.parametrize("precision", ["double", "single"])
@pytest.mark.parametrize("storage", ["dv", "csr"])
@pytest.mark.parametrize("s", [1, 7, 20])
@pytest.mark.parametrize("n", [3, 4096, 5000, 8192])
def test_mat_mult_dense_guarded(ctx, oracle, n, s, storage, precision):
    """R = A S over CSR and DV storage, S's and R's pad rows poisoned and R's entries unwritten beforehand; a
    "single" R has its float storage wrapped, so its pad rows are checked as well.  Over DV storage a double R
    takes the ELL SpMM (n = 3, 4096, 5000) or, where the planes hold whole chunks (64 x 64 x 2, n = 8192), the
    chunk-tile march column by column (mspi_mat_spmm_dv; a float R always takes the ELL SpMM)."""
    nx, ny, nz = _box_of(n)
    assert _march_chunk_fits(nx, ny) == (n == 8192)
    O = oracle.poisson3d_rows(nx, ny, nz, 0, nz)
    A = Mat.box_stencil(ctx, 3, nx, ny, nz)
    A.set_storage(storage)
    assert A.get_storage() == storage
    S = np.asfortranarray(rng().uniform(-1, 1, (n, s)))
    Sd = DenseMat.from_array(ctx, S)
    Rd = DenseMat(ctx, n, s, precision)
    Sg, Rg = DenseGuard(ctx, Sd), DenseGuard(ctx, Rd)
    Sg.poison()
    Rg.poison(entries=True)
    if storage == "dv" and precision == "double":   # the march's own conditions on the operands (mspi_mat_spmm_dv)
        assert Sd.device_ptr() % 16 == 0 and Rd.device_ptr() % 16 == 0 and Sd.lda % 2 == 0 and Rd.lda % 2 == 0
        assert (A.spmv_kernel() == "k_spmv_box_march") == (n != 3)    # 3 x 1 x 1 keeps the ELL kernel
    A.mat_mult_dense(Sd, Rd)
    Rg.assert_written()
    ref = np.stack([O.mult(np.ascontiguousarray(S[:, j])) for j in range(s)], axis=1)
    if precision == "single":
        ref = bt.f32(ref)
    assert_same_bits(Rd.get_values(), ref, "R = A S")
    check_all(Sg, Rg)
    assert_same_bits(Sd.get_values(), S)


def test_lsqr_guarded(ctx, oracle):
    """One LSQR solve (the first case of test_gpu_lsqr.py) with b and alpha guarded and R's pad rows poisoned."""
    case = dict(LSQR_CASES[0])
    (n,), s = case.pop("cuts"), case.pop("s")
    r = rng()
    R = r.uniform(-1, 1, (n, s)) @ np.diag(np.geomspace(1, 1e-3, s))
    b = r.uniform(-1, 1, n)
    xo, ro = oracle.lsqr([R], [b], reduce_mode=oracle.REDUCE_DBR, **case)
    assert ro["its"] > 1
    D = DenseMat.from_array(ctx, R)
    G = DenseGuard(ctx, D)
    assert D.lda > n
    G.poison()
    for lead in LEADS:
        l = LSQR(ctx)
        l._set(**case)
        l.set_operators([D])
        B, X = Guarded.input(ctx, b, lead), Guarded.output(ctx, s, lead)
        l.solve([B.vec], X.vec)
        X.assert_written()
        assert (l.get_iteration_number(), l.get_converged_reason()) == (ro["its"], ro["reason"])
        assert_same_bits(l.get_residual_norm(), ro["rnorm"], "LSQR residual norm")
        assert_same_bits(l.get_norms(), (ro["arnorm"], ro["anorm"]), "LSQR norms")
        assert_same_bits(l.get_residual_history(), ro["hist"], "LSQR history")
        assert_same_bits(X.get_array(), xo, "alpha")
        check_all(B, X, G)
        assert_same_bits(B.get_array(), b, "b after the solve")

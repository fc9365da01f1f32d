"""GPU parity of the hot-path kernels against the CPU oracle.

Integer/index work (assembly) and every per-element operation (SpMV rows,
MAXPY, BLAS-1) must be bit-exact against the oracle.  Reductions (VecDot,
VecNorm, VecMDot) must be bit-exact against the oracle's DBR order.
"""
import contextlib
import ctypes

import numpy as np
import pytest

from medane_tchakorom_ufc_thesis_repository_amd import _lib, utils
from medane_tchakorom_ufc_thesis_repository_amd.petsc import Mat, Vec

pytestmark = pytest.mark.gpu

SEED = 20251121

# msplit_kernels.h tuning flags (MSPLIT_TUNING / msk_set_tuning): every kernel variant a flag selects is
# held to the same bitwise bar as the default
SPMV_TEMPORAL, SPMV_STAGE1, VEC_TEMPORAL, MAXPY_TEMPORAL_ST = 2, 8, 16, 64
MAXPY_HALVES, MDOT_SINGLE, MAXPY_UNROLL1, MDOT_UNROLL2 = 256, 1024, 131072, 262144
ELL_TEMPORAL_Y = 1048576
SPMV_NTY, SPMV_REG_STAGE = 2097152, 4194304
ELL_XCD_ON, ELL_XCD_OFF = 67108864, 134217728


@contextlib.contextmanager
def tuning(flags):
    L = _lib.load()
    L.msk_set_tuning.argtypes = [ctypes.c_int]
    L.msk_set_tuning.restype = None
    L.msk_set_tuning(flags)
    try:
        yield
    finally:
        L.msk_set_tuning(0)


def rng():
    return np.random.default_rng(SEED)


@pytest.mark.parametrize("dim,nx,ny,nz", [(3, 7, 5, 3), (3, 16, 16, 16), (3, 1, 1, 9), (3, 33, 17, 5),
                                          (2, 13, 9, 1), (2, 256, 8, 1), (2, 1, 5, 1)])
def test_box_stencil_matches_host_assembly(ctx, oracle, dim, nx, ny, nz):
    A = Mat.box_stencil(ctx, dim, nx, ny, nz)
    rp, col, val = A.get_csr()
    if dim == 3:
        ho = oracle.poisson3d_rows(nx, ny, nz, 0, nz).arrays()
        hu = utils.poisson3DMatrix_rows(nx, ny, nz, 0, nz)
    else:
        # poisson2DMatrix numbering: ny mesh lines of nx columns
        ho = oracle.poisson2d_rows(ny, nx, 0, nx * ny).arrays()
        hu = utils.poisson2DMatrix_rows(ny, nx, 0, nx * ny)
    for a, b, c in zip((rp, col, val), ho, hu[:3]):
        assert np.array_equal(a, b)
        assert np.array_equal(a, c)


def _spmv_cases(o):
    yield "box3d", o.poisson3d_rows(37, 11, 9, 0, 9)
    yield "slab-coupled", o.poisson3d_rows(16, 16, 16, 4, 8)
    yield "2d", o.poisson2d_rows(64, 50, 0, 64 * 50)


def _random_csr(n, ncols, maxlen, r):
    lens = r.integers(0, maxlen + 1, size=n)
    lens[r.integers(0, n)] = min(ncols, 3000)   # one long row (forces the direct kernel)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort(r.choice(ncols, size=l, replace=False)) for l in lens]).astype(np.int32)
    val = r.standard_normal(rp[-1])
    return rp, col, val


@pytest.mark.parametrize("flags", [0, SPMV_TEMPORAL, SPMV_STAGE1, SPMV_STAGE1 | SPMV_TEMPORAL, ELL_TEMPORAL_Y,
                                   SPMV_NTY, SPMV_REG_STAGE, SPMV_REG_STAGE | SPMV_TEMPORAL, SPMV_REG_STAGE | SPMV_NTY,
                                   ELL_XCD_ON, ELL_XCD_ON | ELL_TEMPORAL_Y])
@pytest.mark.parametrize("storage", ["default", "csr"])
@pytest.mark.parametrize("case", ["box3d", "slab-coupled", "2d", "random", "random-short", "one-row", "empty"])
def test_spmv_and_residual_bitwise(ctx, oracle, case, storage, flags):
    """MatMult / MatResidual in both storages and every load/store policy (the scaled form: test_gpu_gmres)."""
    r = rng()
    if case in ("random", "random-short"):
        n = 1000 if case == "random" else 4099
        rp, col, val = _random_csr(n, 5000, 40 if case == "random" else 9, r)
        if case == "random-short":
            lens = np.diff(rp)
            lens[lens > 9] = 9
            rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            col = np.concatenate([np.sort(r.choice(5000, size=l, replace=False)) for l in lens]).astype(np.int32)
            val = r.standard_normal(rp[-1])
        O = oracle.Mat.from_arrays(n, 5000, rp, col, val)
    elif case == "one-row":
        rp, col, val = np.array([0, 3], np.int32), np.array([0, 2, 5], np.int32), np.array([1.5, -2.0, 3.25])
        O = oracle.Mat.from_arrays(1, 6, rp, col, val)
    elif case == "empty":
        rp, col, val = np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0)
        O = oracle.Mat.from_arrays(3, 7, rp, col, val)
    else:
        O = dict(_spmv_cases(oracle))[case]
        rp, col, val = O.arrays()
    nr, nc = O.shape
    A = Mat.from_csr(ctx, nr, nc, rp, col, val)
    if storage == "csr":
        A.set_storage("csr")
    x = r.uniform(-1, 1, nc)
    b = r.uniform(-1, 1, nr)
    xv, bv, yv = Vec.from_array(ctx, x), Vec.from_array(ctx, b), Vec(ctx, nr)
    with tuning(flags):
        A.mult(xv, yv)
        assert np.array_equal(yv.get_array(), O.mult(x))
        A.residual(bv, xv, yv)
        assert np.array_equal(yv.get_array(), O.residual(b, x))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 511, 4095, 4096, 4097, 8192 + 77, 300001])
def test_dot_norm_bitwise_dbr(ctx, oracle, n):
    r = rng()
    x, y = r.uniform(-1, 1, n), r.uniform(-1, 1, n)
    xv, yv = Vec.from_array(ctx, x), Vec.from_array(ctx, y)
    assert xv.dot(yv) == oracle.dot(x, y, oracle.REDUCE_DBR)
    assert xv.norm() == oracle.norm2(x, oracle.REDUCE_DBR)
    if n:
        assert abs(xv.dot(yv) - oracle.dot(x, y)) <= 1e-12 * np.sum(np.abs(x * y))


@pytest.mark.parametrize("flags", [0, MDOT_UNROLL2, MDOT_UNROLL2 | VEC_TEMPORAL, MDOT_SINGLE, VEC_TEMPORAL])
@pytest.mark.parametrize("nv", [1, 2, 3, 4, 5, 7, 16, 30, 32, 33, 45])
@pytest.mark.parametrize("n", [1, 4097, 70001])
def test_mdot_bitwise_dbr(ctx, oracle, nv, n, flags):
    r = rng()
    w = r.uniform(-1, 1, n)
    V = [r.uniform(-1, 1, n) for _ in range(nv)]
    wv = Vec.from_array(ctx, w)
    Vv = [Vec.from_array(ctx, v) for v in V]
    with tuning(flags):
        got = wv.mdot(Vv)
    assert np.array_equal(got, oracle.mdot(w, V, oracle.REDUCE_DBR))


@pytest.mark.parametrize("flags", [0, MAXPY_UNROLL1, MAXPY_HALVES, MAXPY_HALVES | MAXPY_UNROLL1, MAXPY_TEMPORAL_ST,
                                   VEC_TEMPORAL | MAXPY_TEMPORAL_ST, VEC_TEMPORAL | MAXPY_TEMPORAL_ST | MAXPY_UNROLL1])
@pytest.mark.parametrize("nv", [1, 2, 3, 4, 5, 6, 7, 8, 13, 30, 31, 32, 33, 37, 64, 65])
@pytest.mark.parametrize("n", [1, 7, 4096, 10001])
def test_maxpy_bitwise(ctx, oracle, nv, n, flags):
    r = rng()
    w = r.uniform(-1, 1, n)
    V = [r.uniform(-1, 1, n) for _ in range(nv)]
    a = r.standard_normal(nv)
    wv = Vec.from_array(ctx, w)
    with tuning(flags):
        wv.maxpy(a, [Vec.from_array(ctx, v) for v in V])
    assert np.array_equal(wv.get_array(), oracle.maxpy(w, a, V))


@pytest.mark.parametrize("flags", [MAXPY_HALVES | VEC_TEMPORAL, MDOT_SINGLE | MDOT_UNROLL2,
                                   SPMV_TEMPORAL | SPMV_NTY, SPMV_REG_STAGE | SPMV_STAGE1, ELL_XCD_ON | ELL_XCD_OFF])
def test_tuning_combination_without_kernel_fails_loudly(ctx, flags):
    """A tuning combination no kernel is instantiated for returns an error; it never runs another variant."""
    n, nv = 5000, 3
    wv = Vec.from_array(ctx, np.ones(n))
    V = [Vec.from_array(ctx, np.ones(n)) for _ in range(nv)]
    if flags & (SPMV_REG_STAGE | SPMV_NTY | SPMV_TEMPORAL | ELL_XCD_ON):
        A = Mat.box_stencil(ctx, 3, 8, 8, 8)
        A.set_storage("dv" if flags & ELL_XCD_ON else "csr")
        x, y = Vec.from_array(ctx, np.ones(512)), Vec(ctx, 512)
        with tuning(flags), pytest.raises(Exception):
            A.mult(x, y)
        return
    with tuning(flags), pytest.raises(Exception):
        if flags & MAXPY_HALVES:
            wv.maxpy(np.ones(nv), V)
        else:
            wv.mdot(V)


def test_blas1_bitwise(ctx):
    r = rng()
    n = 12345
    x, y, z = r.uniform(-1, 1, n), r.uniform(-1, 1, n), r.uniform(-1, 1, n)
    X, Y, Z = Vec.from_array(ctx, x), Vec.from_array(ctx, y), Vec.from_array(ctx, z)
    Y.axpy(0.37, X)
    y1 = y + 0.37 * x
    assert np.array_equal(Y.get_array(), y1)
    Y.aypx(-1.25, X)
    y2 = x + (-1.25) * y1
    assert np.array_equal(Y.get_array(), y2)
    Z.waxpy(-1.0, X, Y)
    assert np.array_equal(Z.get_array(), y2 - x)
    Z.waxpy(2.5, X, Y)
    assert np.array_equal(Z.get_array(), y2 + 2.5 * x)
    Z.scale(0.3)
    assert np.array_equal(Z.get_array(), (y2 + 2.5 * x) * 0.3)
    Z.set(-4.0)
    assert np.all(Z.get_array() == -4.0)
    X.copy(Z)
    assert np.array_equal(Z.get_array(), x)
    W = Vec(ctx, 10)
    X.copy_range_to(100, W, 3, 5)
    got = W.get_array()
    assert np.array_equal(got[3:8], x[100:105]) and np.all(got[:3] == 0) and np.all(got[8:] == 0)


def test_errors_are_loud(ctx):
    from medane_tchakorom_ufc_thesis_repository_amd import MsplitError
    A = Mat.box_stencil(ctx, 3, 4, 4, 4)
    with pytest.raises(MsplitError) as e:
        A.mult(Vec(ctx, 63), Vec(ctx, 64))
    assert e.value.code == 60
    with pytest.raises(MsplitError):
        Mat.from_csr(ctx, 2, 2, [0, 2, 3], [1, 0, 1], [1.0, 2.0, 3.0])   # unsorted row
    with pytest.raises(MsplitError):
        Mat.from_csr(ctx, 1, 2, [0, 1], [5], [1.0])                      # column out of range


def test_residual_listed_equals_residual_where_r_holds_b(ctx):
    """msp_mat_residual_listed (updateLocalRHS after the first update): on a row-compressed coupling matrix it
    rewrites only the listed rows, bit for bit msp_mat_residual's, and leaves every other row of r as it was --
    so with r = b there, the whole of r equals the full MatResidual."""
    from medane_tchakorom_ufc_thesis_repository_amd.petsc import Mat, Vec
    r_ = rng()
    n, m = 50000, 3000
    rows = np.sort(r_.choice(n, 700, replace=False)).astype(np.int32)
    cnt = r_.integers(1, 5, rows.size)
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    col = np.concatenate([np.sort(r_.choice(m, c, replace=False)) for c in cnt]).astype(np.int32)
    val = r_.uniform(-1, 1, col.size)
    A = Mat.from_csr_rows(ctx, n, m, rows, rp, col, val)
    b = r_.uniform(-1, 1, n)
    h = r_.uniform(-1, 1, m)
    bv, hv = Vec.from_array(ctx, b), Vec.from_array(ctx, h)
    full = Vec(ctx, n)
    A.residual(bv, hv, full)
    ref = full.get_array()
    listed = Vec.from_array(ctx, b)                  # r already holds b
    A.residual_listed(bv, hv, listed)
    assert np.array_equal(listed.get_array(), ref)
    junk = r_.uniform(5, 6, n)
    other = Vec.from_array(ctx, junk)                # other rows untouched
    A.residual_listed(bv, hv, other)
    got = other.get_array()
    keep = np.ones(n, bool)
    keep[rows] = False
    assert np.array_equal(got[rows], ref[rows]) and np.array_equal(got[keep], junk[keep])

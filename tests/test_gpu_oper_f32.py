"""Compressed-operator GMRES (-msplit_operator_precision single, MSP_OPER_F32) on the GPU.

The Arnoldi products read a packed copy of a CSR-storage operator whose values are floats (msplit_csr32.hip); every
row is summed in f64 in CSR order, so the product is the f64 MatMult on the matrix (double)(float)a bit for bit, and
the restart's residual reads the f64 values.

  * the launcher mspi_spmv_scaled_p32 one call at a time on guarded buffers (tests/guarded.py): the LDS kernel at
    every size where a path changes (one row, a partial block, exactly one block, one block and a row, two blocks and
    a row, seventeen blocks) and the direct kernel, against the oracle's product on the rounded values;
  * whole solves against the twin (tests/oper_twin.py handed to the existing twin solvers) bit for bit: three
    operators, the three basis precisions, Jacobi, two restarts, nonzero guesses, both rnorm0 rules;
  * the copy's life (built by the first solve, rebuilt for a stale version, per matrix), graph replay, the overflow
    error and the refusals.
"""
import ctypes as C
import os

import numpy as np
import pytest

import basis_b16
import basis_twin as bt
import oper_twin as ot
import pc_twin as pt
from guarded import Guarded, assert_same_bits, check_all
from medane_tchakorom_ufc_thesis_repository_amd import MsplitError, _lib
from medane_tchakorom_ufc_thesis_repository_amd.petsc import KSP, Mat, Options, Vec
from medane_tchakorom_ufc_thesis_repository_amd.utils import heterogeneous_poisson3d
from test_gpu_pc_jacobi import _random_csr, _variable_diagonal_csr

pytestmark = pytest.mark.gpu

ERR_SUP, ERR_ARG_OUTOFRANGE = 56, 63
SC = 0.7310585786300049          # the scale sc[it]: no power of two, so x * sc rounds
ROW_LENGTHS = (0, 1, 7, 8, 9, 16, 17, 40)


# ------------------------------------------------------------------------------------------------- the launcher
def _lib_bound():
    L = _lib.load()
    L.mspi_spmv_scaled_p32.argtypes = [C.c_void_p] * 5
    L.mspi_spmv_scaled_p32.restype = C.c_int
    return L


def _ragged(n, seed):
    """Seeded ragged rows with 0, 1, 7, 8, 9, 16, 17 and 40 entries (at most n), sorted distinct columns; row 0 is
    chosen so that the second row block begins at an odd entry offset.  Values: not float-exact, with -0.0 and 1e-40
    among them."""
    rng = np.random.default_rng(seed)
    lens = np.minimum(rng.choice(ROW_LENGTHS, n), n)
    if n > 256:
        lens[0] = 1 if int(lens[1:256].sum()) % 2 == 0 else 0
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens] + [np.zeros(0, np.int64)])
    val = rng.uniform(-2, 2, col.size)
    if val.size >= 8:
        val[rng.choice(val.size, val.size // 8, replace=False)] = -0.0
        val[rng.choice(val.size, val.size // 8, replace=False)] = 1e-40
    return rp, col.astype(np.int32), val


def _launch(ctx, oracle, rp, col, val, x, lead=514, stop=0):
    """One mspi_spmv_scaled_p32 call on guarded x and y; returns (y as read back, the oracle's product)."""
    n = len(rp) - 1
    A = Mat.from_csr(ctx, n, n, rp, col, val)
    A.set_storage("csr")
    xg, yg = Guarded.input(ctx, x, lead), Guarded.output(ctx, n, lead)
    sc = Vec.from_array(ctx, np.array([SC]))
    flag = Vec.from_array(ctx, np.array([stop, 0], np.int32).view(np.float64))
    before = yg.get_array().view(np.uint64).copy()
    rc = _lib_bound().mspi_spmv_scaled_p32(A.h, xg.vec.device_ptr(), sc.device_ptr(), yg.vec.device_ptr(),
                                           flag.device_ptr())
    assert rc == 0, _lib.load().msp_get_last_error().decode(errors="replace")
    ctx.synchronize()
    check_all(xg, yg)                                                 # nothing outside the windows was written
    assert np.array_equal(xg.get_array().view(np.uint64), np.asarray(x, np.float64).view(np.uint64))
    assert A.get_value_copy_bytes() == 8 * (col.size + 2)
    with np.errstate(all="ignore"):
        want = oracle.Mat.from_arrays(n, n, rp, col, ot.round_values(val)).mult(np.asarray(x, np.float64) * SC)
    return A, yg, before, want


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513, 4097])
def test_launcher_on_guarded_buffers(ctx, oracle, n):
    rp, col, val = _ragged(n, 100 + n)
    if n > 256:
        assert rp[256] % 2 == 1                                       # a row block that begins at an odd entry
    if n >= 255:
        assert set(np.diff(rp)) == set(ROW_LENGTHS) and not np.array_equal(ot.round_values(val), val)
    x = np.random.default_rng(n).uniform(-1, 1, n)
    A, yg, _, want = _launch(ctx, oracle, rp, col, val, x)
    assert A.spmv_kernel() == "k_spmv_lds8"                           # the staged shape: k_spmv_p32, not the direct one
    yg.assert_written()
    assert_same_bits(yg.get_array(), want, f"A~ (sc x), n = {n}")
    if n >= 255:                                                      # the f64 values give another product
        assert not np.array_equal(oracle.Mat.from_arrays(n, n, rp, col, val).mult(x * SC), want)


@pytest.mark.parametrize("n", [257, 4097])
def test_launcher_leaves_y_alone_when_stopped(ctx, oracle, n):
    rp, col, val = _ragged(n, 100 + n)
    x = np.random.default_rng(n).uniform(-1, 1, n)
    _, yg, before, _ = _launch(ctx, oracle, rp, col, val, x, stop=1)
    assert np.array_equal(yg.get_array().view(np.uint64), before)


def _direct_matrix():
    """n = 300, the first 256 rows with 17 entries each: 4352 entries in one row block, more than the LDS stage
    takes (4088), so the matrix's lds_cap is 0 and the direct kernel runs."""
    rng = np.random.default_rng(300)
    n = 300
    lens = np.concatenate([np.full(256, 17), rng.choice(ROW_LENGTHS, n - 256)])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens]).astype(np.int32)
    val = rng.uniform(-2, 2, col.size)
    val[::11], val[5::13] = -0.0, 1e-40
    return rp, col, val


def test_launcher_direct_kernel(ctx, oracle):
    rp, col, val = _direct_matrix()
    x = np.random.default_rng(3).uniform(-1, 1, 300)
    A, yg, _, want = _launch(ctx, oracle, rp, col, val, x)
    assert A.spmv_kernel() == "k_spmv_csr"                            # lds_cap 0
    yg.assert_written()
    assert_same_bits(yg.get_array(), want, "the direct kernel")
    _, yg, before, _ = _launch(ctx, oracle, rp, col, val, x, stop=1)
    assert np.array_equal(yg.get_array().view(np.uint64), before)


@pytest.mark.parametrize("kind", ["lds", "direct"])
def test_launcher_ieee_values_in_x(ctx, oracle, kind):
    rp, col, val = _direct_matrix() if kind == "direct" else _ragged(513, 613)
    n = len(rp) - 1
    x = np.random.default_rng(9).uniform(-1, 1, n)
    gathered = np.unique(col)
    assert gathered.size >= 5
    x[gathered[:5]] = [np.inf, -np.inf, np.nan, 5e-324, -0.0]
    _, yg, _, want = _launch(ctx, oracle, rp, col, val, x)
    assert np.isnan(want).any() and np.isfinite(want).any()
    yg.assert_written()
    assert_same_bits(yg.get_array(), want, f"IEEE values in x, {kind} kernel")


def test_launcher_nan_and_inf_values_pass_through(ctx, oracle):
    rp, col, val = _ragged(513, 613)
    val = val.copy()
    val[[0, 50, 900]] = [np.inf, np.nan, -np.inf]                      # neither an error nor counted as overflow
    assert ot.overflow_count(val) == 0
    x = np.random.default_rng(9).uniform(-1, 1, 513)
    _, yg, _, want = _launch(ctx, oracle, rp, col, val, x)
    assert np.isnan(want).any() and np.isinf(want).any()
    assert_same_bits(yg.get_array(), want, "NaN and inf among the values")


# ---------------------------------------------------------------------------------------------------- whole solves
def _opts_str(o, basis="double", pc="none", oper="single"):
    s = (f"-ksp_type gmres -pc_type {pc} -ksp_gmres_restart {o['restart']} -ksp_max_it {o['max_it']} "
         f"-ksp_rtol {o['rtol']} -msplit_basis_precision {basis} -msplit_operator_precision {oper}")
    if o.get("uirnorm"):
        s += " -ksp_converged_use_initial_residual_norm"
    if o.get("guess_nonzero"):
        s += " -ksp_initial_guess_nonzero"
    return s


def _result(ksp, xv):
    return xv.get_array(), {"its": ksp.get_iteration_number(), "reason": ksp.get_converged_reason(),
                            "rnorm": ksp.get_residual_norm(), "hist": ksp.get_residual_history().copy()}


def _gpu(ctx, A, b, x0, optstr):
    ksp = KSP(ctx)
    ksp.set_operators(A)
    ksp.set_from_options(Options(optstr))
    bv = Vec.from_array(ctx, b)
    xv = Vec.from_array(ctx, x0) if x0 is not None else Vec(ctx, A.shape[0])
    ksp.solve(bv, xv)
    return _result(ksp, xv)


def _same(got, want):
    (xg, rg), (xw, rw) = got, want
    assert (rg["its"], rg["reason"]) == (rw["its"], rw["reason"])
    assert rg["rnorm"] == rw["rnorm"] or (np.isnan(rg["rnorm"]) and np.isnan(rw["rnorm"]))
    assert np.array_equal(rg["hist"], rw["hist"], equal_nan=True)
    assert np.array_equal(xg, xw, equal_nan=True)


_cache = {}


def _problem(name):
    """(rowptr, col, val, RoundedOperator, b) of a named operator, built once and shared (never modified)."""
    if name not in _cache:
        if name == "random_csr":
            rp, col, val = _random_csr(np.random.default_rng(2024), 5000, 8)
        elif name == "variable_diagonal":
            rp, col, val = _variable_diagonal_csr()
        else:
            rp, col, val = heterogeneous_poisson3d(17, 16, 16)
        n = len(rp) - 1
        assert not np.array_equal(ot.round_values(val), val)
        _cache[name] = (rp, col, val, ot.RoundedOperator(n, rp, col, val),
                        np.random.default_rng(5).uniform(-1, 1, n))
    return _cache[name]


def _device_matrix(ctx, name):
    rp, col, val, Op, _ = _problem(name)
    A = Mat.from_csr(ctx, Op.shape[0], Op.shape[0], rp, col, val)
    A.set_storage("csr")
    assert A.get_storage() == "csr"
    return A


_twins = {}


def _twin(name, basis, pc, o, x0=None):
    key = (name, basis, pc, tuple(sorted(o.items())), x0 is not None)
    if key not in _twins:
        rp, col, val, Op, b = _problem(name)
        if pc == "jacobi":
            _twins[key] = pt.gmres(Op, b, pt.jacobi_dinv(rp, col, val), x0=x0, **o)
        elif basis == "block16":
            _twins[key] = basis_b16.gmres(Op, b, x0=x0, **o)
        else:
            _twins[key] = bt.gmres(Op, b, x0=x0, rnd=bt.f32 if basis == "single" else bt.identity, **o)
    return _twins[key]


def _x0(n):
    return np.random.default_rng(7).uniform(-1, 1, n)


RESTARTS = {5: dict(restart=5, max_it=17, rtol=1e-30), 30: dict(restart=30, max_it=65, rtol=1e-30)}
MODES = [("double", "none"), ("single", "none"), ("block16", "none"), ("double", "jacobi")]


@pytest.mark.parametrize("restart", list(RESTARTS))
@pytest.mark.parametrize("basis,pc", MODES)
@pytest.mark.parametrize("name", ["random_csr", "variable_diagonal", "box-17x16x16"])
def test_solves_bitwise_vs_twin(ctx, name, basis, pc, restart):
    o = RESTARTS[restart]
    _, _, _, Op, b = _problem(name)
    want = _twin(name, basis, pc, o)
    assert want[1]["its"] > o["restart"]                              # more than one cycle: a restart's f64 residual
    _same(_gpu(ctx, _device_matrix(ctx, name), b, None, _opts_str(o, basis, pc)), want)


@pytest.mark.parametrize("uirnorm", [0, 1])
@pytest.mark.parametrize("basis,pc", MODES)
def test_nonzero_guess_bitwise_vs_twin(ctx, basis, pc, uirnorm):
    o = dict(restart=5, max_it=12, rtol=1e-9, guess_nonzero=1, uirnorm=uirnorm)
    _, _, _, Op, b = _problem("variable_diagonal")
    x0 = _x0(Op.shape[0])
    want = _twin("variable_diagonal", basis, pc, o, x0)
    assert want[1]["its"] > 5
    _same(_gpu(ctx, _device_matrix(ctx, "variable_diagonal"), b, x0, _opts_str(o, basis, pc)), want)


def test_float_exact_operator_is_the_default_solve_and_the_oracle(ctx, oracle):
    O = oracle.poisson3d_rows(17, 16, 16, 0, 16)
    n = O.shape[0]
    rp, col, val = O.arrays()
    b = O.mult(np.ones(n))
    o = dict(restart=30, max_it=300, rtol=1e-6)
    A = Mat.from_csr(ctx, n, n, rp, col, val)
    A.set_storage("csr")
    xo, ro = oracle.gmres(O, b, reduce_mode=oracle.REDUCE_DBR, **o)
    assert ro["its"] > 30
    _same(_gpu(ctx, A, b, None, _opts_str(o, oper="single")), (xo, ro))
    _same(_gpu(ctx, A, b, None, _opts_str(o, oper="double")), (xo, ro))


def test_single_is_not_the_double_solve(ctx, oracle):
    rp, col, val, Op, b = _problem("variable_diagonal")
    o = RESTARTS[30]
    A = _device_matrix(ctx, "variable_diagonal")
    xs, rs = _gpu(ctx, A, b, None, _opts_str(o, oper="single"))
    xd, rd = _gpu(ctx, A, b, None, _opts_str(o, oper="double"))
    xo, ro = oracle.gmres(Op.A, b, reduce_mode=oracle.REDUCE_DBR, **o)
    assert np.array_equal(xd, xo) and np.array_equal(rd["hist"], ro["hist"])     # double is still the oracle's
    assert rs["hist"][0] == rd["hist"][0] and rs["hist"][1] != rd["hist"][1]
    assert not np.array_equal(xs, xd)


def test_graph_replay_equals_eager(ctx):
    _, _, _, Op, b = _problem("variable_diagonal")
    o = RESTARTS[5]
    want = _twin("variable_diagonal", "double", "none", o)
    out = {}
    for graphs in (False, True):
        os.environ["MSPLIT_GRAPHS"] = "1" if graphs else "0"
        try:
            A = _device_matrix(ctx, "variable_diagonal")
            ksp = KSP(ctx)
            ksp.set_operators(A)
            ksp.set_from_options(Options(_opts_str(o)))
            bv, xv = Vec.from_array(ctx, b), Vec(ctx, Op.shape[0])
            out[graphs] = []
            for _ in range(2):                                        # the second solve replays what the first captured
                ksp.solve(bv, xv)
                out[graphs].append(_result(ksp, xv))
        finally:
            os.environ.pop("MSPLIT_GRAPHS", None)
    for got in out[False] + out[True]:
        _same(got, want)


def test_copy_is_built_rebuilt_and_per_matrix(ctx):
    rp, col, val, Op, b = _problem("variable_diagonal")
    n, o = Op.shape[0], RESTARTS[5]
    A = _device_matrix(ctx, "variable_diagonal")
    ksp = KSP(ctx)
    ksp.set_operators(A)
    ksp.set_from_options(Options(_opts_str(o, oper="double")))
    assert ksp.get_operator_precision() == "double"
    bv, xv = Vec.from_array(ctx, b), Vec(ctx, n)
    ksp.solve(bv, xv)
    double = _result(ksp, xv)
    assert A.get_value_copy_bytes() == 0                              # a double solve builds nothing
    want = _twin("variable_diagonal", "double", "none", o)
    ksp.set_operator_precision("single")
    assert ksp.get_operator_precision() == "single"
    ksp.solve(bv, xv)
    _same(_result(ksp, xv), want)
    assert A.get_value_copy_bytes() == 8 * (col.size + 2)
    ksp.set_operator_precision("double")                              # and back: the captured cycles were dropped
    ksp.solve(bv, xv)
    _same(_result(ksp, xv), double)
    A.set_storage("csr")                                              # a new version: the copy is stale, rebuilt
    ksp.set_operator_precision("single")
    ksp.solve(bv, xv)
    _same(_result(ksp, xv), want)
    # a new operator on the same KSP: its own copy, and the solve is that operator's
    rp2, col2, val2, Op2, b2 = _problem("random_csr")
    A2 = _device_matrix(ctx, "random_csr")
    assert A2.get_value_copy_bytes() == 0
    ksp.set_operators(A2)
    bv2 = Vec.from_array(ctx, b2)
    ksp.solve(bv2, xv)
    _same(_result(ksp, xv), _twin("random_csr", "double", "none", o))
    assert A2.get_value_copy_bytes() == 8 * (col2.size + 2)


def test_value_beyond_float_range(ctx, oracle):
    rp, col, val, Op, b = _problem("variable_diagonal")
    n, o = Op.shape[0], RESTARTS[5]
    big = val.copy()
    big[[3, 1000]] = [1e39, -1e39]
    assert ot.overflow_count(big) == 2
    A = Mat.from_csr(ctx, n, n, rp, col, big)
    A.set_storage("csr")
    with pytest.raises(MsplitError) as e:
        _gpu(ctx, A, b, None, _opts_str(o))
    assert e.value.code == ERR_ARG_OUTOFRANGE and "2 finite values" in str(e.value)
    assert A.get_value_copy_bytes() == 0
    # the matrix stays usable in double: bitwise the default solve (no option at all)
    base = f"-ksp_type gmres -pc_type none -ksp_gmres_restart {o['restart']} -ksp_max_it {o['max_it']} -ksp_rtol 1e-30"
    _same(_gpu(ctx, A, b, None, _opts_str(o, oper="double")), _gpu(ctx, A, b, None, base))


# ------------------------------------------------------------------------------------------------------- refusals
def _refused(ctx, A, word):
    n = A.shape[0]
    ones, b = Vec(ctx, n), Vec(ctx, n)
    ones.set(1.0)
    A.mult(ones, b)
    ksp = KSP(ctx)
    ksp.set_operators(A)
    ksp.set_from_options(Options("-ksp_max_it 5 -msplit_operator_precision single"))
    with pytest.raises(MsplitError) as e:
        ksp.solve(b, Vec(ctx, n))
    assert e.value.code == ERR_SUP and word in str(e.value) and "MSP_STORAGE_CSR" in str(e.value)
    ksp.set_operator_precision("double")                              # the KSP and the matrix stay usable
    ksp.solve(b, Vec(ctx, n))


def test_storages_whose_products_do_not_read_the_csr_are_refused(ctx):
    A = Mat.box_stencil(ctx, 3, 8, 8, 8)
    A.set_storage("dv")
    _refused(ctx, A, "MSP_STORAGE_DV")
    rp, col, val = heterogeneous_poisson3d(64, 64, 2)
    S = Mat.from_csr(ctx, len(rp) - 1, len(rp) - 1, rp, col, val)
    S.set_storage("stencil")
    _refused(ctx, S, "MSP_STORAGE_STENCIL")
    _refused(ctx, Mat.box_matfree(ctx, 3, 8, 8, 8), "matrix-free")


def test_seq_reduction_is_refused(ctx):
    _, _, _, Op, b = _problem("variable_diagonal")
    A = _device_matrix(ctx, "variable_diagonal")
    ctx.set_reduction("seq")
    try:
        with pytest.raises(MsplitError) as e:
            _gpu(ctx, A, b, None, _opts_str(RESTARTS[5]))
        assert e.value.code == ERR_SUP and "MSP_REDUCE_SEQ" in str(e.value)
    finally:
        ctx.set_reduction("dbr")


def test_bad_words_are_out_of_range(ctx):
    ksp = KSP(ctx)
    with pytest.raises(MsplitError) as e:
        ksp.set_from_options(Options("-msplit_operator_precision half"))
    assert e.value.code == ERR_ARG_OUTOFRANGE
    with pytest.raises(MsplitError) as e:
        ksp.set_operator_precision("float")
    assert e.value.code == ERR_ARG_OUTOFRANGE
    assert _lib.load().msp_ksp_set_operator_precision(ksp.h, 2) == ERR_ARG_OUTOFRANGE
    assert ksp.get_operator_precision() == "double"

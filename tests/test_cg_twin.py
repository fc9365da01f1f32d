"""The numpy twin of KSPCG (tests/cg_twin.py) against what it must be without a GPU: a dense solve, the identity
preconditioner, and every branch of the solver contract on hand-made systems.  The device solver is then held to
the twin bit for bit (tests/test_gpu_cg.py)."""
import numpy as np
import pytest

import cg_twin as ct


def _diag(oracle, d):
    n = len(d)
    return oracle.Mat.from_arrays(n, n, np.arange(n + 1), np.arange(n), np.asarray(d, float))


@pytest.fixture(scope="module")
def poisson(oracle):
    A = oracle.poisson3d_rows(6, 5, 4, 0, 4)
    b = np.random.default_rng(11).uniform(-1, 1, A.shape[0])
    return A, b


def test_norm2_is_the_square_root_of_the_dot(oracle):
    """With PCNONE one reduction serves beta and dp: the oracle's DBR norm2 is bitwise sqrt of its DBR dot."""
    for n in (1, 7, 4095, 4097, 10000):
        v = np.random.default_rng(n).uniform(-1, 1, n)
        assert oracle.norm2(v, oracle.REDUCE_DBR) == np.sqrt(ct.dot(v, v))


def test_against_dense_solve(oracle, poisson):
    A, b = poisson
    rtol = 1e-10
    x, res = ct.cg(A, b, rtol=rtol)
    assert res["reason"] == ct.CONVERGED_RTOL and 0 < res["its"] <= A.shape[0]
    assert len(res["hist"]) == res["its"] + 1 and res["rnorm"] == res["hist"][-1]
    # the recurrence residual drifts from the true one by O(eps cond): far below 10 rtol ||b||
    true = np.linalg.norm(b - A.dense() @ x)
    print("true residual", true, "recurrence", res["rnorm"], "bound", 10 * rtol * np.linalg.norm(b))
    assert true <= 10 * rtol * np.linalg.norm(b)
    xd = np.linalg.solve(A.dense(), b)
    assert np.linalg.norm(x - xd) <= 1e-8 * np.linalg.norm(xd)


@pytest.mark.parametrize("norm", ["preconditioned", "unpreconditioned"])
def test_identity_preconditioner_is_pcnone(oracle, poisson, norm):
    A, b = poisson
    x0, r0 = ct.cg(A, b, rtol=1e-12)
    x1, r1 = ct.cg(A, b, dinv=np.ones(len(b)), norm=norm, rtol=1e-12)
    assert (r0["its"], r0["reason"]) == (r1["its"], r1["reason"])
    assert np.array_equal(r0["hist"], r1["hist"]) and np.array_equal(x0, x1)


def test_jacobi_norms(oracle):
    """The two norm types run the same recurrence and report ||dinv .* r|| resp. ||r||."""
    d = np.array([1.0, 4.0, 9.0, 16.0])
    A = _diag(oracle, d)
    b = np.ones(4)
    dinv = 1.0 / d
    xp, rp = ct.cg(A, b, dinv=dinv, rtol=1e-30, max_it=1)
    xu, ru = ct.cg(A, b, dinv=dinv, norm="unpreconditioned", rtol=1e-30, max_it=1)
    assert np.array_equal(xp, xu)
    assert rp["hist"][0] == oracle.norm2(dinv * b, oracle.REDUCE_DBR) and ru["hist"][0] == 2.0
    # Jacobi on a diagonal matrix is exact after one step
    assert np.allclose(xp, 1.0 / d, rtol=1e-15)


def test_zero_rhs(oracle, poisson):
    A, _ = poisson
    x, res = ct.cg(A, np.zeros(A.shape[0]))
    assert (res["its"], res["reason"]) == (0, ct.CONVERGED_ATOL) and not x.any() and list(res["hist"]) == [0.0]


def test_beta_zero(oracle):
    """z . r == 0 with ||z|| != 0: the loop's first test ends the solve."""
    A = _diag(oracle, [1.0, 1.0])
    x, res = ct.cg(A, np.array([1.0, 1.0]), dinv=np.array([1.0, -1.0]))
    assert (res["its"], res["reason"]) == (1, ct.CONVERGED_ATOL) and not x.any()
    assert list(res["hist"]) == [np.sqrt(2.0)]


def test_indefinite_matrix(oracle):
    """diag(2, -1): p . A p is 1 at i = 0 and negative at i = 1."""
    A = _diag(oracle, [2.0, -1.0])
    x, res = ct.cg(A, np.array([1.0, 1.0]))
    assert (res["its"], res["reason"]) == (2, ct.DIVERGED_INDEFINITE_MAT)
    assert np.array_equal(x, [2.0, 2.0]) and len(res["hist"]) == 2
    # and p . A p == 0 at i = 0
    x, res = ct.cg(_diag(oracle, [1.0, -1.0]), np.array([1.0, 1.0]))
    assert (res["its"], res["reason"]) == (1, ct.DIVERGED_INDEFINITE_MAT) and not x.any()


def test_indefinite_preconditioner(oracle):
    """One negative entry of dinv: beta = z . r is positive at the start and negative after one step."""
    A = _diag(oracle, [1.0, 2.0, 4.0])
    dinv = np.array([1.0, 0.5, -0.125])
    x, res = ct.cg(A, np.array([1.0, 1.0, 2.0]), dinv=dinv, divtol=1e30)
    print(res)
    assert (res["its"], res["reason"]) == (2, ct.DIVERGED_INDEFINITE_PC) and len(res["hist"]) == 2


def test_nan_and_inf(oracle, poisson):
    A, b = poisson
    bn = b.copy()
    bn[3] = np.nan
    x, res = ct.cg(A, bn)
    assert (res["its"], res["reason"]) == (0, ct.DIVERGED_NANORINF) and np.isnan(res["hist"][0])
    x, res = ct.cg(_diag(oracle, [1.0, np.inf]), np.array([1.0, 1.0]))
    assert (res["its"], res["reason"]) == (1, ct.DIVERGED_NANORINF) and len(res["hist"]) == 1


def test_dtol(oracle):
    A = _diag(oracle, [2.0, -1.0])  # ||r|| grows from sqrt(2) to sqrt(18) in the first step
    x, res = ct.cg(A, np.array([1.0, 1.0]), divtol=2.0)
    assert (res["its"], res["reason"]) == (1, ct.DIVERGED_DTOL) and res["rnorm"] == np.sqrt(18.0)
    # at the start: a guess whose residual is 1e4 ||b|| away
    x, res = ct.cg(_diag(oracle, [1.0, 1.0]), np.array([1.0, 1.0]), x0=np.array([3e4, 0.0]))
    assert (res["its"], res["reason"]) == (0, ct.DIVERGED_DTOL)


def test_atol_and_rtol(oracle, poisson):
    A, b = poisson
    x, res = ct.cg(A, b, rtol=1e-30, abstol=1e-3)
    assert res["reason"] == ct.CONVERGED_ATOL and res["rnorm"] < 1e-3 <= res["hist"][-2]
    x, res = ct.cg(A, b, rtol=1e-4)
    assert res["reason"] == ct.CONVERGED_RTOL and res["rnorm"] <= 1e-4 * res["hist"][0] < res["hist"][-2]


def test_max_it(oracle, poisson):
    A, b = poisson
    x, res = ct.cg(A, b, max_it=0)
    assert (res["its"], res["reason"]) == (0, ct.DIVERGED_ITS) and not x.any() and len(res["hist"]) == 1
    x, res = ct.cg(A, b, max_it=1)
    assert (res["its"], res["reason"]) == (1, ct.DIVERGED_ITS) and len(res["hist"]) == 2
    xf, free = ct.cg(A, b, rtol=1e-6)
    N = free["its"]
    assert N > 3 and free["reason"] == ct.CONVERGED_RTOL
    x, res = ct.cg(A, b, rtol=1e-6, max_it=N)  # the exact hit: converged, not DIVERGED_ITS
    assert (res["its"], res["reason"]) == (N, ct.CONVERGED_RTOL) and np.array_equal(x, xf)
    x, res = ct.cg(A, b, rtol=1e-6, max_it=N - 1)
    assert (res["its"], res["reason"]) == (N - 1, ct.DIVERGED_ITS)
    assert np.array_equal(res["hist"], free["hist"][:N])


def test_nonzero_guess(oracle, poisson):
    A, b = poisson
    x0 = np.random.default_rng(12).uniform(-1, 1, len(b)) * 1e-3 + np.linalg.solve(A.dense(), b)
    r0 = oracle.norm2(A.residual(b, x0), oracle.REDUCE_DBR)
    bn = oracle.norm2(b, oracle.REDUCE_DBR)
    x, res = ct.cg(A, b, x0=x0, rtol=1e-4)                     # relative to ||b||
    xu, resu = ct.cg(A, b, x0=x0, rtol=1e-4, uirnorm=True)     # relative to the initial residual
    assert res["hist"][0] == r0 == resu["hist"][0]
    assert res["reason"] == resu["reason"] == ct.CONVERGED_RTOL
    assert res["rnorm"] <= 1e-4 * bn and resu["rnorm"] <= 1e-4 * r0
    assert res["its"] < resu["its"]                            # r0 is far below ||b||
    # under Jacobi the reference norm is ||dinv .* b||
    dinv = np.full(len(b), 0.25)
    x, res = ct.cg(A, b, x0=x0, dinv=dinv, rtol=1e-4)
    assert res["rnorm"] <= 1e-4 * oracle.norm2(dinv * b, oracle.REDUCE_DBR) < res["hist"][-2]

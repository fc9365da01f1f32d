"""The KSPLSQR step on the GPU, one launcher at a time, against its CPU twin -- bit for bit, on guarded buffers.

Whole solves (tests/test_gpu_lsqr.py) see x and the history.  They do not see U, U1, the partials, the gathered
block sums, V, V1, W or the state, they reach 3 of the 8 template sizes of k_lsqr_onepass, and they never meet a
NaN.  Here every launcher of msp_lsqr_solve runs alone on the buffers of tests/lsqr_step.py and is compared with
tests/lsqr_twin.py (pinned to the C oracle on the CPU by tests/test_lsqr_twin.py): what it may write equals the
twin, everything else is unchanged word for word, every guard word is intact.
"""
import numpy as np
import pytest

import lsqr_step as ls
import lsqr_twin as lt
from guarded import UNWRITTEN_BITS, assert_same_bits, same_bits
from test_gpu_kernels import tuning

pytestmark = pytest.mark.gpu

DENSE_G1, DENSE_G2, DENSE_TEMPORAL_ST, VEC_TEMPORAL = 8388608, 16777216, 33554432, 16   # msplit_kernels.h
PRECS = ("double", "single")
DBL_MAX, DENORM = np.finfo(np.float64).max, 5e-324
FLT_MAX, FLT_DENORM = float(np.finfo(np.float32).max), float(np.float32(1e-45))


def _problem(rows, s, seed=1):
    rng = np.random.default_rng(seed)
    n = sum(rows)
    R = rng.standard_normal((n, s)) @ np.diag(np.geomspace(1, 1e-2, s))
    b = rng.standard_normal(n)
    e = np.cumsum([0] + list(rows))
    return [R[a:c] for a, c in zip(e[:-1], e[1:])], [b[a:c] for a, c in zip(e[:-1], e[1:])]


def _partial_written(call, n, nc):
    """How many leading words of partial a launcher may use (its stage-1 partials)."""
    nch = ls.nchunks(n)
    if call == "onepass":
        return nch * (nc + 1) if nc <= 32 else nch * 32      # s > 32: the gemv's nch, then 32 per dot launch
    return nch * min(nc, 32) if call in ("dots", "dots0") else nch


class Walker:
    """The callback of lt.solve: after every twin call, the same call on the device and the comparison."""

    def __init__(self, W, exact, check=True):
        self.W, self.exact, self.check = W, exact, check
        self.snap = W.snapshot()
        self.calls = []

    def __call__(self, call, k, st, writes, i):
        W, s = self.W, self.W.s
        a, a1 = (i or 0) & 1, 1 - ((i or 0) & 1)
        usc = bool(i)
        rc = {"norm2sq": lambda: W.norm2sq(k), "start": W.ls_start, "colsumsq": lambda: W.colsumsq(k),
              "dots0": lambda: W.scaled_dots(k, f"b{k}", f"U0_{k}", True, k * s),
              "first": lambda: W.ls_first(frob=bool(self.exact)),
              "onepass": lambda: W.onepass(k, f"U{a}_{k}", usc, f"U{a1}_{k}", k * (s + 1)),
              "onepass_step": W.ls_onepass_step,
              "gemv": lambda: W.gemv(k, f"U{a}_{k}", usc, f"U{a1}_{k}", k), "beta": W.ls_beta,
              "dots": lambda: W.scaled_dots(k, f"U{a1}_{k}", None, True, k * s), "step": W.ls_step}[call]()
        assert rc == 0, f"{call}: {ls.last_error()}"
        self.calls.append(call)
        if not self.check:
            return
        what = f"{call}, block {k}, step {i}"
        after = W.snapshot()
        free = []
        for name, val in writes.items():
            if name in ("g", "frob"):
                off, val = val
                assert_same_bits(W.get(name, after)[off:off + len(val)], val, f"{what}: {name}[{off}:]")
                free.append((name, off, off + len(val)))
            else:
                assert_same_bits(W.get(name, after), val, f"{what}: {name}")
                free.append(name)
        if k is None:
            W.assert_state(st, after, what)
            free += ["state"] + list(ls.VECTORS)
        elif writes and call != "norm2sq":
            free.append(("partial", 0, _partial_written(call, W.rows[k], s)))
        W.assert_unchanged(self.snap, after, free, what)
        W.check_guards(after)
        self.snap = after


def _walk(ctx, rows, s, precisions, onepass, exact, max_it=7, max_steps=8, check=True, seed=1):
    Rs, bs = _problem(rows, s, seed)
    W = ls.LsqrWork(ctx, Rs, bs, precisions, max_it=max_it)
    opts = dict(max_it=max_it, rtol=1e-15, abstol=1e-100, exact_norm=exact, conv_test=0)
    W.push_state(lt.new_state(s, len(rows), **opts))                    # as msp_lsqr_solve pushes it
    walker = Walker(W, exact, check)
    x, r = lt.solve(Rs, bs, precisions=precisions, onepass_step=onepass, on=walker, max_steps=max_steps, **opts)
    return W, walker, r


LAYOUTS = [([4097], ("double",)), ([4097], ("single",)), ([4096, 5000], ("double", "double")),
           ([4096, 5000], ("single", "double")), ([3000, 1, 4095], ("single", "single", "single")),
           ([3000, 1, 4095], ("double", "single", "double"))]


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("onepass", [1, 0])
@pytest.mark.parametrize("s", [5, 33])
@pytest.mark.parametrize("rows,precisions", LAYOUTS, ids=lambda v: "-".join(map(str, v)))
def test_solve_launcher_by_launcher(ctx, oracle, rows, precisions, s, onepass, exact):
    """A whole solve of 7 steps in ksp_lsqr.c's order: after each call every region it may write equals the twin,
    everything else is unchanged and the guards hold.  s = 33 takes the two-launch form of the one-pass step."""
    W, walker, r = _walk(ctx, rows, s, precisions, onepass, exact)
    assert (r["its"], r["reason"]) == (7, -3)
    assert walker.calls.count("onepass_step" if onepass else "step") == 7
    assert walker.calls.count("beta") == (0 if onepass else 7)


NCS = (1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32, 33, 64, 65)


@pytest.fixture(scope="module")
def wide():
    """n = 4097 (a full chunk and a one-row tail) x 65 columns, V, U and the scalars of one crafted step."""
    rng = np.random.default_rng(7)
    R = rng.standard_normal((4097, 65)) @ np.diag(np.geomspace(1, 1e-2, 65))
    return dict(R=R, V=rng.standard_normal(65), U=rng.standard_normal(4097), usc=1 / 3, nal=-1.7)


def _wide_work(ctx, wide, prec, R=None):
    W = ls.LsqrWork(ctx, [wide["R"] if R is None else R], None, (prec,))
    st = lt.new_state(W.s, 1, max_it=8, uscale=wide["usc"], nalpha=wide["nal"], V=wide["V"][:W.s])
    W.push_state(st)
    W.put("U0_0", wide["U"][:W.rows[0]])
    return W


def _reset(W):
    for r in ("U1_0", "partial", "g"):
        W.put_bits(r)
    return W.snapshot()


def _check_dense(W, before, call, n, nc, y, out, what):
    """After one dense launcher over n rows and nc columns: y (None: nothing stored) in U1_0[:n], out in g[:len],
    partial untouched past the stage-1 partials, everything else untouched, guards intact."""
    after = W.snapshot()
    free = [("g", 0, len(out))]
    assert_same_bits(W.get("g", after)[:len(out)], out, f"{what}: sums")
    if y is not None:
        assert_same_bits(W.get("U1_0", after)[:n], y, f"{what}: the stored vector")
        free.append(("U1_0", 0, n))
    if n > 0:
        free.append(("partial", 0, _partial_written(call, n, nc)))
    W.assert_unchanged(before, after, free, what)
    W.check_guards(after)


def _three_launchers(W, wide, Rp, n, nc, what, flags=0, with_u=True):
    """onepass, gemv and the two forms of scaled_dots over rows [0, n) and columns [0, nc) of block 0."""
    V, U, usc, nal = wide["V"][:nc], wide["U"][:n], wide["usc"], wide["nal"]
    A = Rp[:n, :nc]
    Un, un = ("U0_0", U) if with_u else (None, None)
    with tuning(flags):
        before = _reset(W)
        assert W.onepass(0, Un, with_u, "U1_0", 0, nc=nc, n=n) == 0, ls.last_error()
        y, out = lt.onepass(A, V, nal, un, usc if with_u else None)
        _check_dense(W, before, "onepass", n, nc, y, out, f"{what}: onepass")
        before = _reset(W)
        assert W.gemv(0, Un, with_u, "U1_0", 0, nc=nc, n=n) == 0, ls.last_error()
        y, sq = lt.gemv(A, V, nal, un, usc if with_u else None)
        _check_dense(W, before, "gemv", n, nc, y if n else None, [sq], f"{what}: gemv")
        for write_back in (True, False):
            before = _reset(W)
            assert W.scaled_dots(0, "U0_0", "U1_0" if write_back else None, True, 0, nc=nc, n=n) == 0
            w, out = lt.scaled_dots(U, usc, A, write_back)
            _check_dense(W, before, "dots", n, nc, w if n else None, out, f"{what}: scaled_dots({write_back})")
        before = _reset(W)                                             # no scale at all: the dots of U as stored
        assert W.scaled_dots(0, "U0_0", None, False, 0, nc=nc, n=n) == 0
        _check_dense(W, before, "dots", n, nc, None, lt.scaled_dots(U, None, A, False)[1], f"{what}: dots")


@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("prec", PRECS)
def test_onepass_every_column_count(ctx, oracle, wide, prec, nc):
    """One call per launcher at every column count around the template sizes NCT = 4 .. 32 of k_lsqr_onepass
    (nc == NCT, NCT + 1), at 1, and across the 32 | 33 switch to the two-launch form and k_scaled_dot's column
    groups (33, 64, 65): U1, the nc + 1 sums, partial untouched past nchunks * (nc + 1), g past nc + 1."""
    Rp = lt.promote(wide["R"], prec)
    W = _wide_work(ctx, wide, prec)
    _three_launchers(W, wide, Rp, 4097, nc, f"nc {nc}")
    if nc in (4, 16, 32):
        _three_launchers(W, wide, Rp, 4097, nc, f"nc {nc}, temporal stores", DENSE_TEMPORAL_ST)
    if nc == 12:
        _three_launchers(W, wide, Rp, 4097, nc, f"nc {nc}, U = NULL", with_u=False)
    if nc in (1, 5, 33, 65):
        for flags in (DENSE_G1, DENSE_G2):
            _three_launchers(W, wide, Rp, 4097, nc, f"nc {nc}, grouping {flags}", flags)


@pytest.mark.parametrize("n", [0, 1, 2, 4095, 4096, 4097, 8193])
@pytest.mark.parametrize("prec", PRECS)
def test_row_counts(ctx, oracle, prec, n):
    """nc = 5 and 33 over the first n rows of an 8193-row block: no store past n, and at n = 0 only the sums
    are written, as +0.0."""
    rng = np.random.default_rng(8)
    big = dict(R=rng.standard_normal((8193, 33)), V=rng.standard_normal(33), U=rng.standard_normal(8193),
               usc=0.7, nal=-0.9)
    W = _wide_work(ctx, big, prec)
    Rp = lt.promote(big["R"], prec)
    for nc in (5, 33):
        _three_launchers(W, big, Rp, n, nc, f"n {n}, nc {nc}")
    if n == 0:
        before = _reset(W)
        assert W.onepass(0, "U0_0", True, "U1_0", 0, nc=5, n=0) == 0
        after = W.assert_unchanged(before, None, [("g", 0, 6)], "n 0: only the six sums")
        got = W.get("g", after)
        assert not got[:6].view(np.uint64).any() and (got[6:].view(np.uint64) == UNWRITTEN_BITS).all()
        W.check_guards(after)


@pytest.mark.parametrize("how", ["y_odd", "U_odd", "vec_temporal"])
@pytest.mark.parametrize("prec", PRECS)
def test_unaligned_operands_take_the_two_launch_form(ctx, oracle, prec, how):
    """y or U at an odd double offset (8-byte aligned only), or MSK_TUNE_VEC_TEMPORAL: dense_lsqr_onepass_t then
    runs the gemv and the unscaled dots instead of k_lsqr_onepass (element-wise loads when unaligned).  The two
    forms give the same bits by design, so which one ran cannot be seen from here; what the test holds is that
    operands only the fallback accepts give the bits of the aligned call and of the twin, store nothing outside
    [0, n) and leave every guard intact.  gemv and scaled_dots get the same operands directly (VEC = 0 with U
    and usc, SCALE = false)."""
    rng = np.random.default_rng(9)
    d = dict(R=rng.standard_normal((8193, 5)), V=rng.standard_normal(5), U=rng.standard_normal(8193), usc=0.3,
             nal=-1.1)
    Rp = lt.promote(d["R"], prec)
    ref = _wide_work(ctx, d, prec)
    _reset(ref)
    assert ref.onepass(0, "U0_0", True, "U1_0", 0) == 0
    shift = {"y_odd": {"U1_0": 1}, "U_odd": {"U0_0": 1}, "vec_temporal": {}}[how]
    W = ls.LsqrWork(ctx, [d["R"]], None, (prec,), shift=shift)
    W.push_state(lt.new_state(5, 1, max_it=8, uscale=d["usc"], nalpha=d["nal"], V=d["V"]))
    W.put("U0_0", d["U"])
    assert (W.ptr("U1_0") % 16 == 8) == (how == "y_odd") and (W.ptr("U0_0") % 16 == 8) == (how == "U_odd")
    _three_launchers(W, d, Rp, 8193, 5, how, VEC_TEMPORAL if how == "vec_temporal" else 0)
    with tuning(VEC_TEMPORAL if how == "vec_temporal" else 0):
        _reset(W)
        assert W.onepass(0, "U0_0", True, "U1_0", 0) == 0
    assert np.array_equal(W.get("U1_0").view(np.uint64), ref.get("U1_0").view(np.uint64))
    assert np.array_equal(W.get("g")[:6].view(np.uint64), ref.get("g")[:6].view(np.uint64))


@pytest.mark.parametrize("onepass", [1, 0])
def test_stop_flag_makes_every_launcher_a_no_op(ctx, oracle, onepass):
    """msp_lsqr_solve enqueues steps in chunks of 8, so up to 7 steps run after the device has set stop.  From
    the state after 3 real steps with stop = 1, each of the 8 launchers that take the flag -- the one-pass
    product, the gemv, the scaled dots (write-back and deferred), mspi_ls_start / first / beta / step /
    onepass_step -- changes nothing anywhere: not U, V, W, g, the partials, the history or the state.
    mspi_dense_colsumsq_p and mspi_norm2sq take no flag (they run before the first test) and are excluded."""
    W, walker, _ = _walk(ctx, [3000, 1, 4095], 5, ("double", "single", "double"), onepass, 1, max_it=20,
                         max_steps=3, check=False)
    assert W.state().its == 3 and W.state().stop == 0
    W.set_stop(1)
    before = W.snapshot()
    s = W.s
    for k in range(3):
        for name, call in (("onepass", lambda: W.onepass(k, f"U0_{k}", True, f"U1_{k}", k * (s + 1))),
                           ("gemv", lambda: W.gemv(k, f"U0_{k}", True, f"U1_{k}", k)),
                           ("scaled_dots, write-back", lambda: W.scaled_dots(k, f"b{k}", f"U0_{k}", True, k * s)),
                           ("scaled_dots, deferred", lambda: W.scaled_dots(k, f"U1_{k}", None, True, k * s))):
            assert call() == 0, ls.last_error()
            W.assert_unchanged(before, None, (), f"{name} of block {k} after stop")
    for name, call in (("ls_start", W.ls_start), ("ls_first", W.ls_first), ("ls_beta", W.ls_beta),
                       ("ls_step", W.ls_step), ("ls_onepass_step", W.ls_onepass_step)):
        assert call() == 0, ls.last_error()
        W.assert_unchanged(before, None, (), f"{name} after stop")
    W.check_guards()


# ------------------------------------------------------------------------------- the one-lane recurrence kernels
def _crafted(s, nblk, **over):
    """A state as after mspi_ls_first and one step: i = its = 1, two history entries, unit V, W, an x with a -0.0."""
    rng = np.random.default_rng(100 * s + nblk)
    V = rng.standard_normal(s)
    V /= np.linalg.norm(V)
    X = rng.standard_normal(s)
    X[-1] = -0.0
    hist = np.full(8, lt.UNSET)
    hist[:2] = [1.0, 0.8]
    base = dict(max_it=6, hist_cap=8, conv_test=0, exact_norm=0, rtol=1e-5, abstol=1e-50, divtol=1e4, i=1, its=1,
                nhist=2, rnorm=0.8, rnorm0=1.0, ttol=1e-5, arnorm=0.3, anorm=2.0, alpha=0.7, beta=0.9, phibar=0.8,
                rhobar=2.0, uscale=1 / 0.9, nalpha=-0.7, V=V, V1=rng.standard_normal(s), W=rng.standard_normal(s),
                X=X, hist=hist)
    base.update(over)
    return lt.new_state(s, nblk, **base)


def _parts(total, nblk):
    """nblk block partials adding up (in block order, roughly) to total: uneven, so the order matters."""
    w = np.array([0.5, 0.25, 0.25]) if nblk == 3 else np.ones(1)
    return np.outer(w, np.atleast_1d(total))


def _case(name, s, nblk):
    """(kernel, state, g (two-pass form), frob, check): check(before, after) asserts the twin reached the branch."""
    rng = np.random.default_rng(len(name) + 10 * s + nblk)
    q = _parts(rng.standard_normal(s), nblk)                            # R_k^T U1_k
    bsq = _parts(0.25, nblk)                                            # ||U1_k||^2: beta = 0.5
    fresh = dict(i=0, its=0, nhist=0, rnorm=0.0, rnorm0=0.0, ttol=0.0, arnorm=0.0, anorm=0.0, alpha=0.0, beta=0.0,
                 phibar=0.0, rhobar=0.0, uscale=0.0, nalpha=0.0, hist=np.full(8, lt.UNSET))
    kernel, frob, st, g = name.split("_")[0], None, _crafted(s, nblk), None
    if kernel == "start":
        st = _crafted(s, nblk, **fresh)
        g = _parts(4.0, nblk)
        if name == "start_nan":
            g[-1, 0] = np.nan
            chk = lambda b, a: a["reason"] == -9 and a["nhist"] == 0 and a["stop"] == 1 and np.isnan(a["rnorm"])
        elif name == "start_inf":
            g[:] = DBL_MAX if nblk > 1 else np.inf                      # three finite partials whose sum overflows
            chk = lambda b, a: a["reason"] == -9 and a["nhist"] == 0 and np.isinf(a["rnorm"])
        elif name == "start_zero":
            g[:] = 0.0
            chk = lambda b, a: a["reason"] == 3 and a["nhist"] == 1 and a["rnorm"] == 0 and a["stop"] == 1
        elif name == "start_dtol":
            st["divtol"] = lt.F(0.5)
            chk = lambda b, a: a["reason"] == -4 and a["stop"] == 1
        elif name == "start_atol":
            st["abstol"] = lt.F(1e3)
            chk = lambda b, a: a["reason"] == 3 and a["rnorm"] > 0 and a["ttol"] == 1e3
        else:
            assert name == "start_iterating"
            chk = lambda b, a: (a["reason"] == 0 and a["stop"] == 0 and
                                a["uscale"] == 1 / a["rnorm"] and not a["X"].any())
    elif kernel == "first":
        st = _crafted(s, nblk, **dict(fresh, beta=2.0, uscale=0.5, nhist=1, rnorm=2.0, rnorm0=2.0, ttol=2e-5))
        g, frob = q, _parts(np.geomspace(1e16, 1.0, s), nblk)
        if name == "first_alpha_zero":
            g = np.zeros((nblk, s))
            chk = lambda b, a: (np.isnan(a["V"]).all() and np.isnan(a["W"]).all() and
                                a["reason"] == 0 and a["alpha"] == 0)
        elif name == "first_frobenius":
            st["exact_norm"] = 1
            blockwise = np.sqrt(sum([sum(row.tolist(), 0.0) for row in frob], 0.0))
            chk = lambda b, a: a["anorm"] == blockwise and a["anorm"] > 0
        elif name == "first_vscale_one":                                # alpha == 1: VecScale(V, 1) leaves V alone
            g = _parts(np.eye(s)[0], nblk)
            chk = lambda b, a: a["alpha"] == 1 and np.array_equal(a["V"], np.eye(s)[0]) and a["reason"] == 0
        elif name == "first_vscale_zero":                               # alpha = inf is not looked at: VecScale(V, 0)
            g = _parts(1e200 * np.eye(s)[0], nblk)
            chk = lambda b, a: np.isinf(a["alpha"]) and not a["V"].view(np.uint64).any() and a["reason"] == 0
        else:
            assert name == "first_no_exact_norm"
            chk = lambda b, a: a["anorm"] == 0 and a["alpha"] > 0 and a["nalpha"] == -a["alpha"]
    elif kernel == "beta":
        g = bsq
        if name == "beta_nan":
            g[0, 0] = np.nan
            chk = lambda b, a: a["reason"] == -9 and a["stop"] == 1 and same_bits(a["beta"], b["beta"])
        elif name == "beta_zero":
            g[:] = 0.0
            chk = lambda b, a: a["beta"] == 0 and a["uscale"] == 1 and a["anorm"] == b["anorm"]
        else:
            assert name == "beta_anorm_update"
            chk = lambda b, a: a["beta"] == 0.5 and a["uscale"] == 2 and a["anorm"] > b["anorm"]
    else:
        assert kernel == "step"
        g = q
        small = dict(V=np.zeros(s))                                     # V1 = q * uscale: alpha as small as q
        if name == "step_alpha_nan":
            g[-1, 0] = np.nan
            chk = lambda b, a: (a["reason"] == -9 and a["beta"] == 0.5 and
                                a["its"] == b["its"] and a["nhist"] == b["nhist"])
        elif name == "step_alpha_zero":
            st, g = _crafted(s, nblk, conv_test=2, **small), np.zeros((nblk, s))
            chk = lambda b, a: (np.isnan(a["V1"]).all() and np.isnan(a["W"]).all() and
                                a["reason"] == 0 and a["alpha"] == 0)
        elif name == "step_beta_zero":
            bsq[:] = 0.0
            chk = lambda b, a: a["beta"] == 0 and a["uscale"] == 1 and a["anorm"] == b["anorm"] and a["reason"] == 3
        elif name == "step_rtol":
            st = _crafted(s, nblk, rtol=0.9, ttol=0.9)
            chk = lambda b, a: a["reason"] == 2 and a["stop"] == 1 and a["its"] == 2
        elif name == "step_atol":
            st = _crafted(s, nblk, abstol=10.0, ttol=10.0)
            chk = lambda b, a: a["reason"] == 3 and a["rnorm"] > 0
        elif name == "step_atol_normal":
            st, g = _crafted(s, nblk, conv_test=1, abstol=1e-3, ttol=1e-3, **small), q * 1e-8
            chk = lambda b, a: a["reason"] == 9 and a["rnorm"] > a["ttol"]
        elif name == "step_rtol_normal":
            st, g = _crafted(s, nblk, conv_test=1, exact_norm=1, anorm=1e3, **small), q * 1e-8
            chk = lambda b, a: a["reason"] == 1 and a["arnorm"] >= a["abstol"]
        elif name == "step_dtol":
            st = _crafted(s, nblk, divtol=0.1)
            chk = lambda b, a: a["reason"] == -4
        elif name == "step_skip_its":
            st = _crafted(s, nblk, conv_test=2, max_it=2)
            chk = lambda b, a: a["reason"] == 4 and a["i"] == 1
        elif name == "step_max_it":
            st = _crafted(s, nblk, max_it=2)
            chk = lambda b, a: a["reason"] == -3 and a["i"] == 2 and a["stop"] == 1
        elif name == "step_hist_full":
            st = _crafted(s, nblk, nhist=8)
            chk = lambda b, a: a["nhist"] == 9 and same_bits(a["hist"], b["hist"]) and a["reason"] == 0
        elif name == "step_phi_zero":
            st = _crafted(s, nblk, phibar=0.0, conv_test=2)
            chk = lambda b, a: np.array_equal(a["X"].view(np.uint64), b["X"].view(np.uint64)) and np.signbit(a["X"][-1])
        elif name == "step_theta_zero":
            st = _crafted(s, nblk, conv_test=2)
            bsq[:] = 0.0
            chk = lambda b, a: np.array_equal(a["W"].view(np.uint64), a["V1"].view(np.uint64)) and a["reason"] == 0
        elif name == "step_vaypx_one":
            # -theta / rho == 1 needs theta < 0: no solve gets there (beta = sqrt(..) >= 0), and neither does
            # mspi_ls_onepass_step, which takes beta from g; mspi_ls_step reads st->beta, so a hand-written
            # beta = -2 with rhobar = 0, V = 0 and g summing to 2 e_0 gives alpha = rho = 2, sn = -1, theta = -2
            st = _crafted(s, nblk, conv_test=2, beta=-2.0, rhobar=0.0, V=np.zeros(s))
            g, bsq = _parts(2 * np.eye(s)[0], nblk), None

            def chk(b, a):
                rho = np.sqrt(b["rhobar"] * b["rhobar"] + b["beta"] * b["beta"])
                theta = (b["beta"] / rho) * a["alpha"]
                return (-theta / rho == 1 and a["alpha"] == 2 and a["reason"] == 0
                        and np.array_equal(a["W"].view(np.uint64), (b["W"] + a["V1"]).view(np.uint64)))
        else:
            assert name == "step_iterating"
            chk = lambda b, a: (a["reason"] == 0 and a["i"] == 2 and
                                same_bits(a["V"], a["V1"]) and a["nalpha"] == -a["alpha"])
        g = (bsq, g)
    return kernel, st, g, frob, chk


CASES = ("start_nan", "start_inf", "start_zero", "start_dtol", "start_atol", "start_iterating", "first_alpha_zero",
         "first_frobenius", "first_no_exact_norm", "first_vscale_one", "first_vscale_zero", "beta_nan", "beta_zero",
         "beta_anorm_update", "step_alpha_nan", "step_alpha_zero", "step_beta_zero", "step_rtol", "step_atol",
         "step_atol_normal", "step_rtol_normal", "step_dtol", "step_skip_its", "step_max_it", "step_hist_full",
         "step_phi_zero", "step_theta_zero", "step_vaypx_one", "step_iterating")


def _run_kernel(W, st0, steps, chk, what):
    """steps: [(g, twin kernel, device launcher)].  From st0 on both sides; after each launch the device holds
    the twin's state and vectors, nothing else changed; chk on the twin's final state."""
    W.put_bits("g")
    W.push_state(st0)
    st = lt.copy_state(st0)
    for g, twin_kernel, launch in steps:
        W.put("g", np.asarray(g, np.float64).ravel())
        before = W.snapshot()
        twin_kernel(st, g)
        assert launch() == 0, ls.last_error()
        after = W.snapshot()
        W.assert_state(st, after, what)
        W.assert_unchanged(before, after, ["state"] + list(ls.VECTORS), what)
        W.check_guards(after)
    assert chk(st0, st), f"{what}: the twin does not reach the branch this case is named for"


@pytest.mark.parametrize("nblk", [1, 3])
@pytest.mark.parametrize("s", [1, 5])
@pytest.mark.parametrize("name", CASES)
def test_recurrence_kernels_on_crafted_state(ctx, oracle, name, s, nblk):
    """One one-lane kernel on a hand-written state, g, V, W, X: every field and vector equals the twin, nothing
    else changes, and the twin's result shows the branch the case is named for.  A step case runs twice from the
    same input: mspi_ls_beta + mspi_ls_step, and mspi_ls_onepass_step on [||U1||^2 | R^T U1] -- the two
    hand-written copies of the recurrence, each against the one twin.  step_vaypx_one (-theta / rho == 1,
    VecAYPX's y + x form) runs mspi_ls_step alone: it needs a negative beta, which no solve produces and which
    mspi_ls_onepass_step, taking beta = sqrt(..) from g, cannot be handed."""
    W = ls.LsqrWork(ctx, [np.ones((2, s))] * nblk, None, None, max_it=6)
    kernel, st0, g, frob, chk = _case(name, s, nblk)
    if kernel == "start":
        _run_kernel(W, st0, [(g, lt.ls_start, W.ls_start)], chk, name)
    elif kernel == "first":
        W.put("frob", frob.ravel())
        for use in (True, False):                                       # gfrob = NULL: no exact norm either
            c = chk if use or name != "first_frobenius" else (lambda b, a: a["anorm"] == 0)
            _run_kernel(W, st0, [(g, lambda st, gg, use=use: lt.ls_first(st, gg, frob if use else None),
                                  lambda use=use: W.ls_first(frob=use))], c, f"{name}, gfrob {use}")
    elif kernel == "beta":
        _run_kernel(W, st0, [(g, lt.ls_beta, W.ls_beta)], chk, name)
    else:
        bsq, q = g
        if bsq is None:
            return _run_kernel(W, st0, [(q, lt.ls_step, W.ls_step)], chk, f"{name}, mspi_ls_step alone")
        _run_kernel(W, st0, [(bsq, lt.ls_beta, W.ls_beta), (q, lt.ls_step, W.ls_step)], chk, f"{name}, two-pass")
        _run_kernel(W, st0, [(np.hstack([bsq, q]), lt.ls_onepass_step, W.ls_onepass_step)], chk, f"{name}, one-pass")


# ------------------------------------------------------------------------------------------ IEEE edge values
KINDS = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "+0": 0.0, "-0": -0.0, "denorm": DENORM, "+max": DBL_MAX,
         "-max": -DBL_MAX}
PLACES = ("full_row", "tail_row", "coef", "U", "usc", "nal")


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("prec", PRECS)
def test_dense_launchers_edge_values(ctx, oracle, prec, kind, place):
    """n = 4097, nc = 5: one special value at a time in a row of the full chunk, in the tail row (whose chunk is
    padded with 0.0 and guarded by e < n), in coef, U, usc and nal, through the three launchers.  A float block
    takes the float's own largest and smallest values."""
    rng = np.random.default_rng(11)
    d = dict(R=rng.standard_normal((4097, 5)), V=rng.standard_normal(5), U=rng.standard_normal(4097), usc=0.3,
             nal=-1.1)
    v = KINDS[kind]
    if place in ("full_row", "tail_row"):
        if prec == "single":
            v = {"denorm": FLT_DENORM, "+max": FLT_MAX, "-max": -FLT_MAX}.get(kind, v)
        d["R"][777 if place == "full_row" else 4096, 2] = v
    elif place == "coef":
        d["V"][3] = v
    elif place == "U":
        d["U"][4096] = v
        d["U"][5] = v
    else:
        d[place] = v
    W = _wide_work(ctx, d, prec)
    Rp = lt.promote(d["R"], prec)
    if place in ("full_row", "tail_row"):
        assert same_bits(Rp[777 if place == "full_row" else 4096, 2], v), "the float block holds the value itself"
    _three_launchers(W, d, Rp, 4097, 5, f"{kind} in {place}")


@pytest.mark.parametrize("nal", [0.0, -0.0])
@pytest.mark.parametrize("prec", PRECS)
def test_dense_launchers_skip_the_axpy_for_a_zero_nal(ctx, oracle, prec, nal):
    """nal == 0 (either sign): VecAXPY does nothing, so a NaN in U and an inf in usc stay out of U1."""
    rng = np.random.default_rng(12)
    d = dict(R=rng.standard_normal((4097, 5)), V=rng.standard_normal(5), U=rng.standard_normal(4097), usc=np.inf,
             nal=nal)
    d["U"][[3, 4096]] = np.nan
    W = _wide_work(ctx, d, prec)
    Rp = lt.promote(d["R"], prec)
    assert not np.isnan(lt.onepass(Rp, d["V"], nal, d["U"], d["usc"])[0]).any()
    _three_launchers(W, d, Rp, 4097, 5, f"nal {nal!r}")

"""GMRES with CGS iterative refinement (msp_ksp_set_cgs_refinement: refine_ifneeded / refine_always) on the GPU.

  * the fused launcher mspi_maxpy_norm_mdot_basis (k_maxpy_mdot: the first pass and the second pass' VecMDot in one
    sweep) on guarded, 16-byte-but-not-32-byte aligned operands, against the two launchers it restates
    (mspi_maxpy_norm_basis then mspi_mdot_basis) and against pyoracle's primitives, bit for bit, at every vector
    count where the 4-grouping or the load schedule changes and every size where a chunk path changes;
  * the decide and update kernels on hand-written blocks, one case per branch; the update against k_norm_update on
    the column it must build;
  * pass 2's MAXPY under the skip word;
  * whole solves against the twin (tests/refine_twin.py) bit for bit, refine counts included;
  * refusals, bad words, switching the type on one KSP.
"""
import ctypes as C
import os

import numpy as np
import pytest

import dbr_fold as df
import oper_twin as ot
import refine_twin as rt
from gmres_step import GmresDev, StepWork, bind, last_error
from guarded import GUARD_BITS, SLACK, UNWRITTEN_BITS, Guarded, assert_same_bits, same_bits
from medane_tchakorom_ufc_thesis_repository_amd import MsplitError, _lib
from medane_tchakorom_ufc_thesis_repository_amd.petsc import KSP, Mat, Options, Vec
from medane_tchakorom_ufc_thesis_repository_amd.utils import heterogeneous_poisson3d
from test_refine_twin import rhs, zero_diagonal_laplacian

pytestmark = pytest.mark.gpu

ERR_SUP, ERR_ARG_OUTOFRANGE = 56, 63
NEVER, IFNEEDED, ALWAYS = 0, 1, 2
DIVERGED_NANORINF = -9
CHUNK = 4096
MAX_GROUP = 32

_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64


class Refine(C.Structure):
    """mspi_gmres_refine (msplit_internal.h); c(0..m+1) follows it."""
    _fields_ = [("mode", C.c_int32), ("refine", C.c_int32), ("skip", C.c_int32), ("count", C.c_int32),
                ("ss1", C.c_double), ("ss2", C.c_double)]


RF_WORDS = C.sizeof(Refine) // 8


def _L():
    L = bind()
    for name, args in {
        "mspi_maxpy_norm_mdot_basis": [_vp, _vp, _vp, _i, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp],
        "mspi_gm_refine_decide": [_vp, GmresDev, _vp, _vp, _i64],
        "mspi_gm_refine_maxpy2": [_vp, _vp, _i, _vp, _i64, _vp, _i64, _vp],
        "mspi_gm_refine_update": [_vp, GmresDev, _vp, _vp, _i64, _i],
        "mspi_gm_refine_fused": [_i],
    }.items():
        f = getattr(L, name)
        f.argtypes, f.restype = args, C.c_int
    L.mspi_ctx_partial.argtypes, L.mspi_ctx_partial.restype = [_vp], _vp
    return L


def _ok(rc):
    assert rc == 0, last_error()


# ---------------------------------------------------------------------------------------------- the fused launcher
class Operands:
    """W, the output vector and nv basis vectors, every one a window at an address that is 16-byte but not 32-byte
    aligned, NaN guard words between and around them; sc, h, the outputs and the stop flag in a small vector."""
    LEAD = 514

    def __init__(self, ctx, n, nv, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.n, self.nv = ctx, n, nv
        self.stride = n + (n & 1) + 6                       # even: every vector 16-byte aligned; + 6: the pads
        if (self.stride // 2) % 2 == 1:
            self.stride += 2                                 # a multiple of 4: every vector at 16 mod 32 like the first
        self.W = rng.uniform(-1, 1, n)
        self.V = rng.uniform(-1, 1, (nv, n))
        self.sc = rng.uniform(0.5, 1.5, nv)
        self.h = rng.uniform(-1, 1, nv)
        tot = self.LEAD + nv * self.stride + SLACK
        img = np.full(tot, GUARD_BITS, np.uint64)
        for j in range(nv):
            lo = self.LEAD + j * self.stride
            img[lo:lo + n] = self.V[j].view(np.uint64)
        self.basis = Vec(ctx, tot)
        self.basis.set_values(img.view(np.float64))
        self.bimg = img
        self.base = self.basis.device_ptr() + 8 * self.LEAD
        assert self.base % 32 == 16 and (self.stride * 8) % 32 == 0
        self.vec = {}
        for name, fill in (("w", self.W.view(np.uint64)), ("out", np.full(n, UNWRITTEN_BITS, np.uint64)),
                           ("ref", np.full(n, UNWRITTEN_BITS, np.uint64))):
            im = np.full(self.LEAD + n + (n & 1) + SLACK, GUARD_BITS, np.uint64)
            im[self.LEAD:self.LEAD + n] = fill
            v = Vec(ctx, im.size)
            v.set_values(im.view(np.float64))
            self.vec[name] = (v, im)
        # scalars: sc[32] h[32] c_fused[32] ss_fused[1] c_ref[32] ss_ref[1] flag[1]
        s = np.full(32 * 4 + 3 + 8, GUARD_BITS, np.uint64).view(np.float64)
        s[0:nv], s[32:32 + nv] = self.sc, self.h
        s[64:64 + 33] = np.full(33, UNWRITTEN_BITS, np.uint64).view(np.float64)
        s[97:97 + 33] = np.full(33, UNWRITTEN_BITS, np.uint64).view(np.float64)
        s[130] = 0.0
        self.sv = Vec.from_array(ctx, s)
        self.simg = s.view(np.uint64).copy()

    def p(self, name):
        return self.vec[name][0].device_ptr() + 8 * self.LEAD

    def s(self, off):
        return self.sv.device_ptr() + 8 * off

    def set_stop(self, v):
        self.sv.set_values(np.array([v, 0], np.int32).view(np.float64), 130)
        self.simg[130] = np.array([v, 0], np.int32).view(np.uint64)[0]

    def window(self, name):
        return self.vec[name][0].get_array()[self.LEAD:self.LEAD + self.n]

    def scalars(self):
        return self.sv.get_array()

    def check_guards(self):
        self.ctx.synchronize()
        assert np.array_equal(self.basis.get_array().view(np.uint64), self.bimg), "the basis was written"
        for name, (v, im) in self.vec.items():
            u = v.get_array().view(np.uint64)
            keep = np.ones(u.size, bool)
            if name != "w":
                keep[self.LEAD:self.LEAD + self.n] = False
            bad = np.flatnonzero(keep & (u != im))
            assert bad.size == 0, f"{bad.size} words around {name} changed, first at window offset {bad[0] - self.LEAD}"

    def fused(self, L, fold=True):
        return L.mspi_maxpy_norm_mdot_basis(self.ctx.h, self.p("w"), self.p("out"), self.nv, self.base, self.stride,
                                            self.s(0), self.n, self.s(32), self.s(64) if fold else None,
                                            self.s(96) if fold else None, self.s(130))

    def two_kernels(self, L):
        rc = L.mspi_maxpy_norm_basis(self.ctx.h, self.p("w"), self.p("ref"), self.nv, self.base, self.stride,
                                     self.s(0), self.n, self.s(32), self.s(129), self.s(130))
        return rc or L.mspi_mdot_basis(self.ctx.h, self.p("ref"), self.nv, self.base, self.stride, self.s(0), self.n,
                                       self.s(97), self.s(130))


NVS = [1, 2, 3, 4, 5, 7, 8, 29, 30, 31]
NS = [1, 511, 4095, 4096, 4097, 8193, 3 * 4096 + 17]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("nv", NVS)
def test_fused_launcher_equals_the_two_kernels_and_the_oracle(ctx, oracle, nv, n):
    L = _L()
    op = Operands(ctx, n, nv, 1000 * nv + n)
    _ok(L.mspi_reserve_partial(ctx.h, n))
    _ok(op.fused(L))
    _ok(op.two_kernels(L))
    op.check_guards()
    u, uref, s = op.window("out"), op.window("ref"), op.scalars()
    assert not (u.view(np.uint64) == UNWRITTEN_BITS).any()
    D = oracle.REDUCE_DBR
    Vs = [op.V[j] * op.sc[j] for j in range(nv)]
    want_u = oracle.maxpy(op.W, -op.h, Vs)
    assert_same_bits(uref, want_u, "the two kernels' u against the oracle")
    assert_same_bits(u, uref, f"u, nv = {nv}, n = {n}")
    assert_same_bits(s[96], s[129], "ss1 against the two kernels")
    assert_same_bits(s[96], oracle.dot(want_u, want_u, D), "ss1 against the oracle")
    assert_same_bits(s[64:64 + nv], s[97:97 + nv], "c against the two kernels")
    assert_same_bits(s[64:64 + nv], oracle.mdot(want_u, Vs, D), "c against the oracle")
    # rows beyond nv, and everything else in the scalar vector, untouched
    after = s.view(np.uint64)
    keep = np.ones(after.size, bool)
    keep[64:64 + nv] = keep[96] = keep[97:97 + nv] = keep[129] = False
    assert np.array_equal(after[keep], op.simg[keep])


@pytest.mark.parametrize("n", [4095, 3 * 4096 + 17])
@pytest.mark.parametrize("nv", [3, 31])
def test_fused_launcher_writes_nothing_when_stopped(ctx, nv, n):
    L = _L()
    op = Operands(ctx, n, nv, 7)
    op.set_stop(1)
    _ok(L.mspi_reserve_partial(ctx.h, n))
    pv = Vec(ctx, (n + CHUNK - 1) // CHUNK * MAX_GROUP, device_ptr=L.mspi_ctx_partial(ctx.h))
    before = pv.get_array().view(np.uint64).copy()
    _ok(op.fused(L))
    op.check_guards()
    assert (op.window("out").view(np.uint64) == UNWRITTEN_BITS).all()
    assert np.array_equal(op.scalars().view(np.uint64), op.simg)
    assert np.array_equal(pv.get_array().view(np.uint64), before)


def test_fused_launcher_limits(ctx):
    L = _L()
    op = Operands(ctx, 100, 31, 3)
    op.nv = 32                                                        # 33 rows: more than the partial buffer holds
    assert op.fused(L) == ERR_SUP
    assert L.mspi_gm_refine_fused(31) == 1 and L.mspi_gm_refine_fused(32) == 0


# ------------------------------------------------------------------------------------ the decide and update kernels
M, IT = 5, 2


class Block:
    """A StepWork recurrence block at step it = 2 of GMRES(5) (earlier rotations the identity, so the column the
    update builds is read off directly) and a refinement block behind guard words."""

    def __init__(self, ctx, mode, h, c, ss1, stop=0):
        self.ctx, self.L = ctx, _L()
        self.w = StepWork(ctx, 64, M)
        self.w.init_state(it=IT, its=IT, res=0.5, rnorm=0.5, rnorm0=1.0, ttol=1e-30, gm_rnorm0=1.0, stop=stop)
        self.w.put("cc", np.ones(IT))
        self.w.put("grs", np.array([0.0, 0.0, 0.5]))
        self.w.put("sc", np.ones(IT + 1))
        self.w.put("h", np.asarray(h, np.float64))
        self.w.put("hist", np.array([1.0, 0.75, 0.5]))
        st = self.w.state()
        st.nhist = 3
        self.w.push_state(st)
        img = np.full(RF_WORDS + M + 2 + 8, GUARD_BITS, np.uint64).view(np.float64)
        hdr = Refine(mode, 0, 1, 4, ss1, -7.0)
        img[:RF_WORDS] = np.frombuffer(bytes(hdr), np.float64)
        img[RF_WORDS:RF_WORDS + M + 2] = 0.0
        img[RF_WORDS:RF_WORDS + len(c)] = c
        self.rf = Vec.from_array(ctx, img)

    def block(self):
        a = self.rf.get_array()
        return Refine.from_buffer_copy(a[:RF_WORDS].tobytes()), a[RF_WORDS:RF_WORDS + M + 2], a[RF_WORDS + M + 2:]

    def decide(self, partial=None, nchunks=0):
        _ok(self.L.mspi_gm_refine_decide(self.ctx.h, self.w.g, self.rf.device_ptr(), partial, nchunks))
        self.ctx.synchronize()

    def update(self, ss2=None, partial=None, nchunks=1):
        """ss2 handed over as one partial, or partial: a device array of nchunks partials of it."""
        if partial is None:
            pv = Vec.from_array(self.ctx, np.array([ss2 if ss2 is not None else np.nan, np.nan]))
            partial = pv.device_ptr()
        _ok(self.L.mspi_gm_refine_update(self.ctx.h, self.w.g, self.rf.device_ptr(), partial, nchunks, M))
        self.ctx.synchronize()


def _reference_update(ctx, h_col, sumsq):
    """k_norm_update on the column h_col with ||w||^2 = sumsq: what the refined update must leave in the recurrence."""
    b = Block(ctx, NEVER, h_col, [], 0.0)
    pv = Vec.from_array(ctx, np.array([sumsq, np.nan]))
    _ok(b.w.gm_norm_update(pv.device_ptr(), 1))
    return b.w


def _same_recurrence(got: StepWork, want: StepWork, what):
    sg, sw = got.snapshot(), want.snapshot()
    for r in ("state", "hh", "cc", "ss", "grs", "sc", "hist"):
        assert same_bits(got.words(r, sg).view(np.float64), want.words(r, sw).view(np.float64)), f"{what}: {r} differs"
    assert same_bits(got.get("h", sg)[IT + 1], want.get("h", sw)[IT + 1]), f"{what}: h(it+1) differs"
    got.check_guards(sg)


H = np.array([0.3, -0.4, 1.2])                 # ||h||^2 = 0.09 + 0.16 + 1.44, summed in j order
CC = np.array([1e-3, -2e-3, 5e-4])
HSQ = (np.float64(0.0) + H[0] * H[0] + H[1] * H[1]) + H[2] * H[2]
HNRM = np.sqrt(HSQ)
SS_EQ = float(HSQ)                             # sqrt(ss1) == hnrm exactly: not "<"
SS_LT = float(np.nextafter(HNRM, 0.0) ** 2 * (1 - 1e-15))
SS_GT = float(np.nextafter(HNRM, 4.0) ** 2 * (1 + 1e-15))


@pytest.mark.parametrize("name,mode,ss1,refine", [
    ("always", ALWAYS, 9.0, 1), ("ifneeded <", IFNEEDED, SS_LT, 1), ("ifneeded =", IFNEEDED, SS_EQ, 0),
    ("ifneeded >", IFNEEDED, SS_GT, 0), ("never", NEVER, 0.01, 0)])
def test_decide_and_update_branches(ctx, name, mode, ss1, refine):
    assert np.sqrt(SS_LT) < HNRM and np.sqrt(SS_EQ) == HNRM and np.sqrt(SS_GT) > HNRM
    b = Block(ctx, mode, H, CC, ss1)
    b.decide()
    hdr, c, guard = b.block()
    assert (hdr.mode, hdr.refine, hdr.skip, hdr.count) == (mode, refine, 1 - refine, 4 + refine)
    assert hdr.ss1 == ss1 and hdr.ss2 == -7.0 and np.array_equal(c[:3], CC)
    assert (guard.view(np.uint64) == GUARD_BITS).all()
    ss2 = 0.0625
    b.update(ss2)
    hdr, c, guard = b.block()
    assert hdr.skip == 1 and hdr.refine == refine and hdr.count == 4 + refine
    assert hdr.ss2 == (ss2 if refine else -7.0)
    assert (guard.view(np.uint64) == GUARD_BITS).all()
    col = (np.float64(0.0) - (-H)) - (-CC) if refine else H           # hh_j = 0.0; hh_j -= -h_j; hh_j -= -c_j
    _same_recurrence(b.w, _reference_update(ctx, col, ss2 if refine else ss1), name)
    st = b.w.state()
    assert (st.it, st.its, st.reason) == (IT + 1, IT + 1, 0)
    assert b.w.get("hh")[IT * (M + 2) + IT + 1] == np.sqrt(ss2 if refine else ss1)


def test_decide_folds_the_fused_pass_partials(ctx, oracle):
    """rows 0..it of the partial buffer are c, row it + 1 is ss1: the fold of the fused launcher's stage 2."""
    L = _L()
    n, nv = 3 * 4096 + 17, IT + 1
    op = Operands(ctx, n, nv, 11)
    _ok(L.mspi_reserve_partial(ctx.h, n))
    _ok(op.fused(L, fold=True))
    s = op.scalars().copy()
    b = Block(ctx, IFNEEDED, op.h, [], -1.0)
    _ok(op.fused(L, fold=False))
    b.decide(L.mspi_ctx_partial(ctx.h), (n + CHUNK - 1) // CHUNK)
    hdr, c, _ = b.block()
    assert_same_bits(c[:nv], s[64:64 + nv], "c folded by the decide kernel")
    assert_same_bits(hdr.ss1, s[96], "ss1 folded by the decide kernel")
    hsq = np.float64(0.0)
    for v in op.h:
        hsq = hsq + v * v
    assert hdr.refine == int(np.sqrt(s[96]) < np.sqrt(hsq))


@pytest.mark.parametrize("mode", [ALWAYS, IFNEEDED], ids=["always", "ifneeded"])
@pytest.mark.parametrize("nch", df.NCH_THIN)
def test_decide_and_update_fold_many_chunks(ctx, nch, mode):
    """fold_partials beyond one trip per lane (tests/dbr_fold.py: the second trip, the 8-deep and the 16-deep loop,
    one after the other), on synthetic partials in guarded windows: the decide kernel's c_j and ss1 and the update
    kernel's ss2 are fold() of their rows bit for bit, the decision is the one those sums give, and the recurrence
    is k_norm_update's on the column and the sum they give."""
    for name in df.NAMES:
        seed = 31 * nch + 7 * mode
        rows = [df.data_sets(nch, seed + r)["mixed" if r != 1 else name] for r in range(IT + 1)]      # c_0 .. c_it
        rows.append(df.data_sets(nch, seed + 5, signed=False)[name])                                   # ||u||^2
        ss2row = df.data_sets(nch, seed + 6, signed=False)[name]
        cw = np.array([df.fold(r) for r in rows[:IT + 1]])
        ss1, ss2 = df.fold(rows[IT + 1]), df.fold(ss2row)
        p1 = Guarded.input(ctx, np.concatenate(rows), Operands.LEAD)
        p2 = Guarded.input(ctx, ss2row, Operands.LEAD)
        b = Block(ctx, mode, H, [], -1.0)
        b.decide(p1.vec.device_ptr(), nch)
        hdr, c, guard = b.block()
        what = f"{name}, {nch} chunks"
        assert_same_bits(c[:IT + 1], cw, f"c folded by the decide kernel, {what}")
        assert_same_bits(hdr.ss1, ss1, f"ss1 folded by the decide kernel, {what}")
        with np.errstate(invalid="ignore"):
            wnrm = np.sqrt(ss1)
        refine = 1 if mode == ALWAYS else int(bool(np.isfinite(wnrm) and wnrm < HNRM))
        assert (hdr.refine, hdr.skip, hdr.count) == (refine, 1 - refine, 4 + refine), what
        assert (guard.view(np.uint64) == GUARD_BITS).all() and not c[IT + 1:].any()
        if not refine and not np.isfinite(wnrm):
            continue                                   # KSPCheckNorm's branch folds nothing (test_nan_ss1_...)
        b.update(partial=p2.vec.device_ptr(), nchunks=nch)
        hdr, _, guard = b.block()
        assert hdr.skip == 1 and (guard.view(np.uint64) == GUARD_BITS).all()
        assert_same_bits(hdr.ss2, ss2 if refine else -7.0, f"ss2 folded by the update kernel, {what}")
        col = (np.float64(0.0) - (-H)) - (-cw) if refine else H
        _same_recurrence(b.w, _reference_update(ctx, col, ss2 if refine else ss1), what)
        p1.check()
        p2.check()


def test_nan_ss1_ends_the_cycle_like_a_nan_dot(ctx):
    b = Block(ctx, IFNEEDED, H, CC, float("nan"))
    b.decide()
    hdr, _, _ = b.block()
    assert (hdr.refine, hdr.skip, hdr.count) == (0, 1, 4)
    b.update()
    st = b.w.state()
    assert (st.reason, st.stop, st.skip_build, st.it, st.its) == (DIVERGED_NANORINF, 1, 0, IT, IT)
    assert not b.w.get("hh")[IT * (M + 2):IT * (M + 2) + IT + 1].any()   # the column zeroed
    _same_recurrence(b.w, _reference_update(ctx, [np.nan, 0.0, 0.0], np.nan), "NaN ss1")


def test_inf_c_ends_the_cycle_like_a_nan_dot(ctx):
    b = Block(ctx, ALWAYS, H, [1e-3, np.inf, 0.0], 9.0)
    b.decide()
    assert b.block()[0].refine == 1
    b.update(0.0625)
    st = b.w.state()
    assert (st.reason, st.stop, st.skip_build, st.it) == (DIVERGED_NANORINF, 1, 0, IT)
    _same_recurrence(b.w, _reference_update(ctx, [0.3, np.inf, 1.2], 0.0625), "inf c")


def test_inf_h_does_not_refine(ctx):
    b = Block(ctx, ALWAYS, [0.3, np.inf, 1.2], CC, 9.0)
    b.decide()
    hdr, _, _ = b.block()
    assert (hdr.refine, hdr.skip, hdr.count) == (0, 1, 4)
    b.update()
    assert b.w.state().reason == DIVERGED_NANORINF


def test_decide_and_update_are_no_ops_when_stopped(ctx):
    b = Block(ctx, ALWAYS, H, CC, 9.0, stop=1)
    rf0, snap = b.rf.get_array().view(np.uint64).copy(), b.w.snapshot()
    b.decide()
    b.update(0.0625)
    assert np.array_equal(b.rf.get_array().view(np.uint64), rf0)
    b.w.assert_unchanged(snap, what="decide + update under stop")


@pytest.mark.parametrize("skip", [1, 0])
def test_second_maxpy_follows_the_skip_word(ctx, oracle, skip):
    L = _L()
    n, nv = 4097, 5
    op = Operands(ctx, n, nv, 21)
    _ok(L.mspi_reserve_partial(ctx.h, n))
    _ok(op.fused(L))
    u = op.window("out").copy()
    cvals = op.scalars()[64:64 + nv].copy()
    img = np.zeros(RF_WORDS + nv + 1)
    img[:RF_WORDS] = np.frombuffer(bytes(Refine(ALWAYS, 1 - skip, skip, 0, 0.0, 0.0)), np.float64)
    img[RF_WORDS:RF_WORDS + nv] = cvals
    rf = Vec.from_array(ctx, img)
    nch = (n + CHUNK - 1) // CHUNK
    pv = Vec(ctx, nch * MAX_GROUP, device_ptr=L.mspi_ctx_partial(ctx.h))
    before = pv.get_array().view(np.uint64).copy()
    _ok(L.mspi_gm_refine_maxpy2(ctx.h, op.p("out"), nv, op.base, op.stride, op.s(0), n, rf.device_ptr()))
    op.check_guards()
    if skip:
        assert_same_bits(op.window("out"), u, "VV(it+1) under skip")
        assert np.array_equal(pv.get_array().view(np.uint64), before)
    else:
        Vs = [op.V[j] * op.sc[j] for j in range(nv)]
        assert_same_bits(op.window("out"), oracle.maxpy(u, -cvals, Vs), "u' = u - sum c_j v_j")
        assert not np.array_equal(pv.get_array().view(np.uint64)[:nch], before[:nch])


# ---------------------------------------------------------------------------------------------------- whole solves
_cache = {}


def _problem(oracle, name):
    """(rowptr, col, val, twin operator, b), built once and shared."""
    if name not in _cache:
        if name.startswith("box"):
            g = tuple(int(v) for v in name[4:].split("x"))
            rp, col, val = oracle.poisson3d_rows(*g, 0, g[2]).arrays()
        elif name == "aij":
            rp, col, val = heterogeneous_poisson3d(17, 16, 16)
        elif name == "mixed":
            rp, col, val = zero_diagonal_laplacian(oracle, 12, 10, 8)
        elif name == "inf":
            rp, col, val = heterogeneous_poisson3d(12, 10, 8)
            val = val.copy()
            val[len(val) // 2] = np.inf
        n = len(rp) - 1
        _cache[name] = (rp, col, np.asarray(val, np.float64), oracle.Mat.from_arrays(n, n, rp, col, val), rhs(n))
    return _cache[name]


def _device_matrix(ctx, oracle, name):
    rp, col, val, O, _ = _problem(oracle, name)
    n = O.shape[0]
    if name.startswith("box"):
        g = tuple(int(v) for v in name[4:].split("x"))
        return Mat.box_stencil(ctx, 3, *g)
    A = Mat.from_csr(ctx, n, n, rp, col, val)
    if name in ("aij", "inf"):
        A.set_storage("csr")
    return A


_twins = {}


def _twin(oracle, name, mode, o, x0=None, single=False):
    key = (name, mode, tuple(sorted(o.items())), x0 is not None, single)
    if key not in _twins:
        rp, col, val, O, b = _problem(oracle, name)
        Op = ot.RoundedOperator(O.shape[0], rp, col, val) if single else O
        _twins[key] = rt.gmres(Op, b, x0=x0, cgs=mode, **o)
    return _twins[key]


def _opts_str(o, oper="double"):
    s = (f"-ksp_type gmres -pc_type none -ksp_gmres_restart {o['restart']} -ksp_max_it {o['max_it']} "
         f"-ksp_rtol {o['rtol']} -msplit_operator_precision {oper}")
    if o.get("guess_nonzero"):
        s += " -ksp_initial_guess_nonzero"
    return s


def _result(ksp, xv):
    return xv.get_array(), {"its": ksp.get_iteration_number(), "reason": ksp.get_converged_reason(),
                            "rnorm": ksp.get_residual_norm(), "hist": ksp.get_residual_history().copy(),
                            "count": ksp.get_cgs_refinement_count()}


def _gpu(ctx, A, b, x0, o, mode, oper="double"):
    ksp = KSP(ctx)
    ksp.set_operators(A)
    ksp.set_from_options(Options(_opts_str(o, oper)))
    if mode is not None:
        ksp.set_cgs_refinement(mode)
        assert ksp.get_cgs_refinement() == mode
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
    if "refined" in rw:
        assert rg["count"] == sum(rw["refined"])
    else:
        assert rg["count"] == rw["count"]


RESTARTS = {5: dict(restart=5, max_it=17, rtol=1e-30), 30: dict(restart=30, max_it=65, rtol=1e-30)}


@pytest.mark.parametrize("restart", list(RESTARTS))
@pytest.mark.parametrize("mode", rt.MODES)
@pytest.mark.parametrize("name", ["box-12x10x8", "box-24x24x16", "aij", "mixed"])
def test_solves_bitwise_vs_twin(ctx, oracle, name, mode, restart):
    o = RESTARTS[restart]                                             # max_it ends mid-cycle: 3 x 5 + 2, 2 x 30 + 5
    _, _, _, _, b = _problem(oracle, name)
    want = _twin(oracle, name, mode, o)
    A = _device_matrix(ctx, oracle, name)
    got = _gpu(ctx, A, b, None, o, mode)
    _same(got, want)
    assert want[1]["its"] == o["max_it"]
    if mode == "always":
        assert got[1]["count"] == got[1]["its"]                        # every Arnoldi step run
    if mode == "never":
        assert got[1]["count"] == 0
        _same(got, _gpu(ctx, A, b, None, o, None))                     # the present default path
    if mode == "ifneeded" and name == "mixed":
        dec = want[1]["refined"]
        assert any(dec) and not all(dec) and 0 < got[1]["count"] < got[1]["its"]


@pytest.mark.parametrize("mode", ["ifneeded", "always"])
def test_nonzero_guess_over_three_restarts(ctx, oracle, mode):
    o = dict(restart=5, max_it=12, rtol=1e-30, guess_nonzero=1)
    _, _, _, O, b = _problem(oracle, "aij")
    x0 = np.random.default_rng(7).uniform(-1, 1, O.shape[0])
    want = _twin(oracle, "aij", mode, o, x0)
    assert want[1]["its"] == 12
    _same(_gpu(ctx, _device_matrix(ctx, oracle, "aij"), b, x0, o, mode), want)


@pytest.mark.parametrize("mode", ["ifneeded", "always"])
def test_restart_33_takes_the_two_kernel_sequence_from_32_vectors(ctx, oracle, mode):
    o = dict(restart=33, max_it=40, rtol=1e-30)
    _, _, _, _, b = _problem(oracle, "mixed")
    want = _twin(oracle, "mixed", mode, o)
    assert want[1]["its"] == 40
    _same(_gpu(ctx, _device_matrix(ctx, oracle, "mixed"), b, None, o, mode), want)


@pytest.mark.parametrize("mode", ["ifneeded", "always"])
def test_graph_replay_equals_eager(ctx, oracle, mode):
    o = RESTARTS[5]
    _, _, _, O, b = _problem(oracle, "mixed")
    want = _twin(oracle, "mixed", mode, o)
    out = []
    for graphs in ("0", "1"):
        os.environ["MSPLIT_GRAPHS"] = graphs
        try:
            ksp = KSP(ctx)
            ksp.set_operators(_device_matrix(ctx, oracle, "mixed"))
            ksp.set_from_options(Options(_opts_str(o)))
            ksp.set_cgs_refinement(mode)
            bv, xv = Vec.from_array(ctx, b), Vec(ctx, O.shape[0])
            for _ in range(2):                                        # the second solve replays what the first captured
                ksp.solve(bv, xv)
                out.append(_result(ksp, xv))
        finally:
            os.environ.pop("MSPLIT_GRAPHS", None)
    for got in out:
        _same(got, want)


@pytest.mark.parametrize("mode", ["ifneeded", "always"])
def test_single_precision_operator_composes(ctx, oracle, mode):
    o = RESTARTS[5]
    rp, col, val, _, b = _problem(oracle, "aij")
    assert not np.array_equal(ot.round_values(val), val)
    want = _twin(oracle, "aij", mode, o, single=True)
    assert not np.array_equal(want[0], _twin(oracle, "aij", mode, o)[0])
    _same(_gpu(ctx, _device_matrix(ctx, oracle, "aij"), b, None, o, mode, oper="single"), want)


@pytest.mark.parametrize("mode", ["ifneeded", "always"])
def test_inf_entry_diverges_like_the_twin(ctx, oracle, mode):
    o = RESTARTS[5]
    _, _, _, _, b = _problem(oracle, "inf")
    want = _twin(oracle, "inf", mode, o)
    assert want[1]["reason"] == DIVERGED_NANORINF
    _same(_gpu(ctx, _device_matrix(ctx, oracle, "inf"), b, None, o, mode), want)


def test_switching_the_type_on_one_ksp(ctx, oracle):
    o = RESTARTS[5]
    _, _, _, O, b = _problem(oracle, "mixed")
    ksp = KSP(ctx)
    ksp.set_operators(_device_matrix(ctx, oracle, "mixed"))
    ksp.set_from_options(Options(_opts_str(o)))
    assert ksp.get_cgs_refinement() == "never"
    bv, xv = Vec.from_array(ctx, b), Vec(ctx, O.shape[0])
    bytes_seen = set()
    for mode in ("ifneeded", "never", "always", "ifneeded", "never"):
        ksp.set_cgs_refinement(mode)
        ksp.solve(bv, xv)
        _same(_result(ksp, xv), _twin(oracle, "mixed", mode, o))
        bytes_seen.add(ksp.get_work_bytes())
    assert len(bytes_seen) == 1                                       # the work stays; only captured cycles go
    assert not np.array_equal(_twin(oracle, "mixed", "never", o)[1]["hist"],
                              _twin(oracle, "mixed", "always", o)[1]["hist"])


# -------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("mode", ["ifneeded", "always"])
@pytest.mark.parametrize("what,word", [("single", "MSP_BASIS_F32"), ("block16", "MSP_BASIS_B16"),
                                       ("jacobi", "MSP_PC_JACOBI"), ("seq", "MSP_REDUCE_SEQ")])
def test_refusals_name_their_cause(ctx, oracle, what, word, mode):
    _, _, _, O, b = _problem(oracle, "aij")
    A = _device_matrix(ctx, oracle, "aij")
    ksp = KSP(ctx)
    ksp.set_operators(A)
    ksp.set_from_options(Options("-ksp_max_it 5"))
    ksp.set_cgs_refinement(mode)
    if what in ("single", "block16"):
        ksp.set_basis_precision(what)
    elif what == "jacobi":
        ksp.set_pc_type("jacobi")
    else:
        ctx.set_reduction("seq")
    bv, xv = Vec.from_array(ctx, b), Vec(ctx, O.shape[0])
    try:
        with pytest.raises(MsplitError) as e:
            ksp.solve(bv, xv)
        assert e.value.code == ERR_SUP and word in str(e.value)
        assert ("MSP_CGS_REFINE_ALWAYS" if mode == "always" else "MSP_CGS_REFINE_IFNEEDED") in str(e.value)
    finally:
        if what == "seq":
            ctx.set_reduction("dbr")
    ksp.set_cgs_refinement("never")                                   # the KSP stays usable
    if what != "seq":
        ksp.solve(bv, xv)


def test_words_and_options(ctx):
    ksp = KSP(ctx)
    with pytest.raises(MsplitError) as e:
        ksp.set_cgs_refinement("sometimes")
    assert e.value.code == ERR_ARG_OUTOFRANGE
    assert _lib.load().msp_ksp_set_cgs_refinement(ksp.h, 3) == ERR_ARG_OUTOFRANGE
    assert _lib.load().msp_ksp_set_cgs_refinement(ksp.h, -1) == ERR_ARG_OUTOFRANGE
    assert ksp.get_cgs_refinement() == "never" and ksp.get_cgs_refinement_count() == 0
    ksp.set_from_options(Options("-ksp_gmres_cgs_refinement_type refine_ifneeded"))
    assert ksp.get_cgs_refinement() == "ifneeded"
    ksp.set_from_options(Options("-ksp_max_it 7"))                    # an absent option leaves the type alone
    assert ksp.get_cgs_refinement() == "ifneeded"
    ksp.set_from_options(Options("-ksp_gmres_cgs_refinement_type refine_never"))
    assert ksp.get_cgs_refinement() == "never"
    with pytest.raises(MsplitError) as e:
        ksp.set_from_options(Options("-ksp_gmres_cgs_refinement_type refine_always"))
    assert e.value.code == ERR_SUP and 'set_cgs_refinement("always")' in str(e.value)
    with pytest.raises(MsplitError):
        ksp.set_from_options(Options("-ksp_gmres_cgs_refinement_type refine_twice"))
    pk = KSP(ctx)
    pk.set_options_prefix("inner1_")
    pk.set_from_options(Options("-inner1_ksp_gmres_cgs_refinement_type refine_ifneeded"))
    assert pk.get_cgs_refinement() == "ifneeded"
    ksp.set_cgs_refinement("always")
    assert ksp.get_cgs_refinement() == "always"

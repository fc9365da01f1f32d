"""The KSPLSQR step one launcher at a time, on guarded work buffers (helper, not a test).

TEST INFRASTRUCTURE ONLY.  msp_lsqr_solve (ksp_lsqr.c) drives a solve through the internal launchers of
msplit_internal.h; the suite reaches them only through whole solves, where U, U1, the partials, the gathered block
sums and the state block are internal allocations nobody looks at.  This module binds the launchers with ctypes
and gives them buffers laid out as lsqr_setup lays them out, but inside owned backing Vecs whose every non-operand
word holds a NaN of a known bit pattern (tests/guarded.py), so that a test can run one call, read everything back
and say which words changed.  The twin of tests/gmres_step.py.

  LsqrState, LsqrDev   ctypes mirrors of mspi_lsqr_state / mspi_lsqr_dev (checked against the C header by
                       tests/test_lsqr_step_layout.py, on the CPU, before any pointer reaches the device)
  bind()               the library with the launchers' signatures set
  LsqrWork             the buffers, the named regions inside them, snapshots, and one method per launcher

A launcher's return code is returned, never raised.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from lsqr_names import DEV_FIELDS, STATE_DOUBLES, STATE_INTS, VECTORS   # noqa: F401  (re-exported)
from guarded import GUARD_BITS, SLACK, UNWRITTEN_BITS, DenseGuard, assert_same_bits
from medane_tchakorom_ufc_thesis_repository_amd import _lib
from medane_tchakorom_ufc_thesis_repository_amd.petsc import DenseMat, Vec

CHUNK = 4096                     # MSK_DBR_CHUNK: rows per DBR partial


class LsqrState(C.Structure):
    _fields_ = [(f, C.c_int32) for f in STATE_INTS] + [(f, C.c_double) for f in STATE_DOUBLES]


class LsqrDev(C.Structure):
    """Passed BY VALUE to the mspi_ls_* launchers."""
    _fields_ = [(f, C.c_void_p) for f in DEV_FIELDS]


def layout(struct) -> dict:
    """{"sizeof": n, field: offset, ...} of a ctypes mirror (tests/test_lsqr_step_layout.py)."""
    out = {"sizeof": C.sizeof(struct)}
    out.update({name: getattr(struct, name).offset for name, _ in struct._fields_})
    return out


_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
_SIGS = {
    "mspi_norm2sq": [_vp, _vp, _i64, _vp],
    "mspi_dense_colsumsq_p": [_vp, _vp, _i, _i64, _i, _i64, _vp, _vp],
    # ctx, A, prec, lda, nc, n, coef, nal, U, usc, y, partial, out, stop
    "mspi_dense_gemv_p": [_vp, _vp, _i, _i64, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "mspi_dense_lsqr_onepass_p": [_vp, _vp, _i, _i64, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    # ctx, win, wout, sc, A, prec, lda, nc, n, partial, out, stop
    "mspi_dense_scaled_dots_p": [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _i64, _vp, _vp, _vp],
    "mspi_ls_start": [_vp, LsqrDev],
    "mspi_ls_first": [_vp, LsqrDev, _vp],
    "mspi_ls_beta": [_vp, LsqrDev],
    "mspi_ls_step": [_vp, LsqrDev],
    "mspi_ls_onepass_step": [_vp, LsqrDev],
}


def bind() -> C.CDLL:
    """The loaded library with the launchers' argument types set (all return int)."""
    L = _lib.load()
    for name, args in _SIGS.items():
        f = getattr(L, name)
        f.argtypes, f.restype = args, C.c_int
    return L


def last_error() -> str:
    return _lib.load().msp_get_last_error().decode(errors="replace")


def round_up(n: int, k: int) -> int:
    return (n + k - 1) // k * k


def nchunks(n: int) -> int:
    return (n + CHUNK - 1) // CHUNK


class LsqrWork:
    """The work buffers of one msp_lsqr over the row blocks Rs (one array per block, s columns each), as lsqr_setup
    lays them out:

      R<k>      a DenseMat of precisions[k] ("double" / "single"), its pad rows n .. lda poisoned (DenseGuard)
      b<k>      the block's right-hand side, n doubles
      U0_<k>, U1_<k>   the two N-vectors of a block: n doubles, the rest of the allocation (n rounded up to 512,
                plus 512) is guard
      partial   exactly nchunks(max n) * max(s + 1, 32) doubles
      g, frob   nblk * (s + 1) and nblk * s doubles
      state, V, V1, W, hist   one block: the state rounded up to 256 bytes, three s-vectors, max_it + 2 doubles
      X         s doubles

    Each buffer is a window at 512 doubles (4 KiB) into an owned backing Vec -- shift moves named windows by a few
    doubles, for the unaligned forms -- with SLACK guard doubles behind it.  Words outside every region hold
    GUARD_BITS for good (check_guards); U, partial, g, frob, V, V1, W, X and hist start as UNWRITTEN_BITS, the
    state as zeros.  snapshot() reads everything back; assert_unchanged() compares two snapshots word for word
    outside the listed exceptions."""

    LEAD = 512

    def __init__(self, ctx, Rs, bs=None, precisions=None, max_it=8, shift=None):
        self.ctx, self.L = ctx, bind()
        self.nblk = len(Rs)
        self.rows = [int(R.shape[0]) for R in Rs]
        self.s = int(Rs[0].shape[1])
        self.prec = list(precisions or ["double"] * self.nblk)
        self.max_it, self.hist_cap = int(max_it), int(max_it) + 2
        self.st_words = round_up(C.sizeof(LsqrState), 256) // 8
        self.back, self.regions, self._operand = {}, {}, {}
        shift = shift or {}
        s, lead = self.s, self.LEAD

        self.R, self.Rguard = [], []
        for R, p in zip(Rs, self.prec):
            D = DenseMat.from_array(ctx, R, precision=p)
            gd = DenseGuard(ctx, D)
            gd.poison()
            self.R.append(D)
            self.Rguard.append(gd)
        for k, n in enumerate(self.rows):
            self._alloc(f"b{k}", n, {f"b{k}": n}, shift.get(f"b{k}", 0))
            for a in (0, 1):
                name = f"U{a}_{k}"
                self._alloc(name, round_up(n, 512) + 512, {name: n}, shift.get(name, 0), slack=0)
        pw = max(s + 1, 32)
        self.npartial = max(nchunks(max(self.rows)), 1) * pw
        self._alloc("partial", self.npartial, {"partial": self.npartial})
        self._alloc("g", self.nblk * (s + 1), {"g": self.nblk * (s + 1)})
        self._alloc("frob", self.nblk * s, {"frob": self.nblk * s})
        self._alloc("rec", self.st_words + 3 * s + self.hist_cap,
                    {"state": self.st_words, "V": s, "V1": s, "W": s, "hist": self.hist_cap})
        self._alloc("X", s, {"X": s})

        for b, vec in self.back.items():
            img = np.full(vec.n, GUARD_BITS, np.uint64)
            for r, (rb, lo, cnt) in self.regions.items():
                if rb == b:
                    img[lo:lo + cnt] = 0 if r == "state" else UNWRITTEN_BITS
            vec.set_values(img.view(np.float64))
        for k in range(self.nblk):
            self.put(f"b{k}", np.zeros(self.rows[k]) if bs is None else bs[k])
        self.dev = LsqrDev(*[self.ptr(f if f != "st" else "state") for f in DEV_FIELDS])
        self.p_stop = self.ptr("state") + LsqrState.stop.offset
        self.p_uscale = self.ptr("state") + LsqrState.uscale.offset
        self.p_nalpha = self.ptr("state") + LsqrState.nalpha.offset

    # ------------------------------------------------------------------------------------------------ layout
    def _alloc(self, name, ndoubles, regions, shift=0, slack=SLACK):
        """A backing of LEAD + shift + ndoubles + slack doubles; regions {name: count} in order from LEAD + shift."""
        total = self.LEAD + shift + ndoubles + slack
        self.back[name] = Vec(self.ctx, total)
        assert self.back[name].device_ptr() % 4096 == 0
        self._operand[name] = np.zeros(total, bool)
        off = self.LEAD + shift
        for r, cnt in regions.items():
            self.regions[r] = (name, off, cnt)
            self._operand[name][off:off + cnt] = True
            off += cnt

    def ptr(self, region: str, index: int = 0) -> int:
        b, lo, _ = self.regions[region]
        return self.back[b].device_ptr() + 8 * (lo + index)

    def Rptr(self, k: int) -> int:
        return self.R[k].device_ptr_f32() if self.prec[k] == "single" else self.R[k].device_ptr()

    # -------------------------------------------------------------------------------------------- host <-> device
    def put(self, region: str, values, index: int = 0):
        b, lo, cnt = self.regions[region]
        a = np.ascontiguousarray(np.atleast_1d(values), np.float64)
        assert index + a.size <= cnt
        if a.size:
            self.back[b].set_values(a, lo + index)

    def put_bits(self, region: str, bits=UNWRITTEN_BITS):
        self.put(region, np.full(self.regions[region][2], bits, np.uint64).view(np.float64))

    def snapshot(self) -> dict:
        """Every backing as uint64 words, after a synchronise."""
        self.ctx.synchronize()
        return {b: v.get_array().view(np.uint64).copy() for b, v in self.back.items()}

    def get(self, region: str, snap: dict | None = None) -> np.ndarray:
        b, lo, cnt = self.regions[region]
        snap = self.snapshot() if snap is None else snap
        return snap[b][lo:lo + cnt].view(np.float64).copy()

    def _where(self, b, i) -> str:
        for r, (rb, lo, cnt) in self.regions.items():
            if rb == b and lo <= i < lo + cnt:
                return f"{r}[{i - lo}]"
        return f"guard word {i - self.LEAD} (from the first window's start) of the {b} buffer"

    def check_guards(self, snap: dict | None = None):
        """Every word outside the regions still holds its guard bits; so do the pad rows of every R block."""
        snap = self.snapshot() if snap is None else snap
        for b, words in snap.items():
            bad = np.flatnonzero(~self._operand[b] & (words != GUARD_BITS))
            assert bad.size == 0, (f"{bad.size} guard words of the {b} buffer were overwritten, first: "
                                   f"{self._where(b, int(bad[0]))} = {int(words[bad[0]]):#x}")
        for gd in self.Rguard:
            gd.check()

    def assert_unchanged(self, before: dict, after: dict | None = None, except_=(), what=""):
        """after (default: now) equals before word for word, outside except_: region names, or (region, lo, hi)."""
        after = self.snapshot() if after is None else after
        for b in before:
            free = np.zeros(before[b].size, bool)
            for e in except_:
                r, lo, hi = (e, 0, None) if isinstance(e, str) else e
                rb, rlo, cnt = self.regions[r]
                if rb == b:
                    free[rlo + lo:rlo + (cnt if hi is None else hi)] = True
            bad = np.flatnonzero(~free & (before[b] != after[b]))
            assert bad.size == 0, (f"{what}: {bad.size} words of the {b} buffer changed, first: "
                                   f"{self._where(b, int(bad[0]))}: {int(before[b][bad[0]]):#x} -> "
                                   f"{int(after[b][bad[0]]):#x}")
        return after

    # ------------------------------------------------------------------------------------------------- state
    def push_state(self, st: dict):
        """A twin state (tests/lsqr_twin.py): the scalar fields into the state block, the vectors into theirs."""
        c = LsqrState()
        for f in STATE_INTS:
            setattr(c, f, int(st[f]))
        for f in STATE_DOUBLES:
            setattr(c, f, float(st[f]))
        raw = np.zeros(self.st_words)
        raw.view(np.uint8)[:C.sizeof(c)] = np.frombuffer(bytes(c), np.uint8)
        self.put("state", raw)
        for v in VECTORS:
            a = np.asarray(st[v], np.float64)
            assert a.size == self.regions[v][2], v
            self.put(v, a)

    def state(self, snap: dict | None = None) -> LsqrState:
        return LsqrState.from_buffer_copy(self.get("state", snap).tobytes()[:C.sizeof(LsqrState)])

    def assert_state(self, st: dict, snap: dict | None = None, what=""):
        """The device's state block and s-vectors hold the twin's, bit for bit (NaN against NaN)."""
        snap = self.snapshot() if snap is None else snap
        got = self.state(snap)
        for f in STATE_INTS:
            assert getattr(got, f) == int(st[f]), f"{what}: state.{f} = {getattr(got, f)}, the twin has {int(st[f])}"
        for f in STATE_DOUBLES:
            assert_same_bits(getattr(got, f), float(st[f]), f"{what}: state.{f}")
        for v in VECTORS:
            assert_same_bits(self.get(v, snap), st[v], f"{what}: {v}")
        tail = self.get("state", snap)[C.sizeof(LsqrState) // 8:]
        assert not tail.view(np.uint64).any(), f"{what}: the state block's padding was written"

    def set_stop(self, stop: int = 1):
        raw = self.get("state")
        raw.view(np.int32)[LsqrState.stop.offset // 4] = stop
        self.put("state", raw)

    # -------------------------------------------------------------------------------- the launchers, as ksp_lsqr.c
    def _dense(self, k, nc, n):
        D = self.R[k]
        return self.Rptr(k), DenseMat.PRECISIONS[self.prec[k]], int(D.lda), self.s if nc is None else nc, \
            self.rows[k] if n is None else n

    def norm2sq(self, k, gi=None):
        return self.L.mspi_norm2sq(self.ctx.h, self.ptr(f"b{k}"), self.rows[k], self.ptr("g", k if gi is None else gi))

    def colsumsq(self, k, nc=None, n=None):
        A, prec, lda, nc, n = self._dense(k, nc, n)
        return self.L.mspi_dense_colsumsq_p(self.ctx.h, A, prec, lda, nc, n, self.ptr("partial"),
                                            self.ptr("frob", k * self.s))

    def scaled_dots(self, k, win, wout, sc, gi, nc=None, n=None, stop=True):
        """win, wout: region names (wout None: no write-back); sc: True = &st->uscale; out = g + gi."""
        A, prec, lda, nc, n = self._dense(k, nc, n)
        return self.L.mspi_dense_scaled_dots_p(self.ctx.h, self.ptr(win), self.ptr(wout) if wout else None,
                                               self.p_uscale if sc else None, A, prec, lda, nc, n,
                                               self.ptr("partial"), self.ptr("g", gi), self.p_stop if stop else None)

    def _step_args(self, k, U, usc, y, gi, nc, n):
        A, prec, lda, nc, n = self._dense(k, nc, n)
        return (self.ctx.h, A, prec, lda, nc, n, self.ptr("V"), self.p_nalpha, self.ptr(U) if U else None,
                self.p_uscale if usc else None, self.ptr(y), self.ptr("partial"), self.ptr("g", gi), self.p_stop)

    def gemv(self, k, U, usc, y, gi, nc=None, n=None):
        """y = R_k V + nalpha (U uscale), g[gi] = ||y||^2."""
        return self.L.mspi_dense_gemv_p(*self._step_args(k, U, usc, y, gi, nc, n))

    def onepass(self, k, U, usc, y, gi, nc=None, n=None):
        """y as gemv, g[gi ..] = [||y||^2 | R_k^T y]."""
        return self.L.mspi_dense_lsqr_onepass_p(*self._step_args(k, U, usc, y, gi, nc, n))

    def ls_start(self):
        return self.L.mspi_ls_start(self.ctx.h, self.dev)

    def ls_first(self, frob=True):
        return self.L.mspi_ls_first(self.ctx.h, self.dev, self.ptr("frob") if frob else None)

    def ls_beta(self):
        return self.L.mspi_ls_beta(self.ctx.h, self.dev)

    def ls_step(self):
        return self.L.mspi_ls_step(self.ctx.h, self.dev)

    def ls_onepass_step(self):
        return self.L.mspi_ls_onepass_step(self.ctx.h, self.dev)

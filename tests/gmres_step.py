"""The GMRES Arnoldi step one entry point at a time, on guarded work buffers (helper, not a test).

TEST INFRASTRUCTURE ONLY.  ksp_gmres.c:enqueue_cycle drives a restart cycle through the internal launchers of
msplit_internal.h (mspi_spmv_mdot, mspi_maxpy_norm_update, ...).  The suite reaches them only through whole solves,
where the basis, W, the f32 current vector and the recurrence block are zero-filled internal allocations nobody
looks at.  This module binds those launchers with ctypes and gives them buffers laid out exactly as msp_ksp_set_up
lays them out, but inside owned backing Vecs whose every non-operand word holds a NaN of a known bit pattern
(tests/guarded.py), so that a test can run one call, read everything back and say which words changed.

  GmresState, GmresDev   ctypes mirrors of mspi_gmres_state / mspi_gmres_dev (checked against the C header by
                         tests/test_gmres_step_layout.py, on the CPU, before any pointer reaches the device)
  bind()                 the library with the step entry points' signatures set
  StepWork               the buffers, the named regions inside them, snapshots, and one method per entry point

A launcher's return code is returned, never raised: refusals are part of what the tests check.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from guarded import GUARD_BITS, GUARD_BITS_F32, SLACK, UNWRITTEN_BITS, UNWRITTEN_BITS_F32
from medane_tchakorom_ufc_thesis_repository_amd import _lib
from medane_tchakorom_ufc_thesis_repository_amd.petsc import Vec

ERR_SUP = 56                     # include/msplit.h: MSP_ERR_SUP (PETSc's number)
DIVERGED_ITS, DIVERGED_BREAKDOWN = -3, -5

# mspi_gmres_state, field for field (msplit_internal.h)
STATE_INTS = ("stop", "skip_build", "it", "its", "reason", "nhist", "nbuild", "guess_zero", "m", "max_it", "uirnorm",
              "hist_cap")
STATE_DOUBLES = ("res", "rnorm", "rnorm0", "ttol", "gm_rnorm0", "scale", "bnorm", "rtol", "abstol", "divtol",
                 "haptol", "breakdowntol")
DEV_FIELDS = ("st", "hh", "cc", "ss", "grs", "h", "sc", "hist")


class GmresState(C.Structure):
    _fields_ = [(f, C.c_int32) for f in STATE_INTS] + [(f, C.c_double) for f in STATE_DOUBLES]


class GmresDev(C.Structure):
    """Passed BY VALUE to the launchers that take an mspi_gmres_dev."""
    _fields_ = [(f, C.c_void_p) for f in DEV_FIELDS]


def layout(struct) -> dict:
    """{"sizeof": n, field: offset, ...} of a ctypes mirror, in the form tests/test_gmres_step_layout.py compares
    with what the C compiler says."""
    out = {"sizeof": C.sizeof(struct)}
    out.update({name: getattr(struct, name).offset for name, _ in struct._fields_})
    return out


_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
_BASIS = [_i, _vp, _i64, _vp]           # nv, base, stride, scale
_SIGS = {
    "mspi_reserve_partial": [_vp, _i64],
    "mspi_norm2sq": [_vp, _vp, _i64, _vp],
    "mspi_gm_cycle_start": [_vp, GmresDev, _vp],
    "mspi_spmv_scaled": [_vp, _vp, _vp, _vp, _vp, _vp],
    "mspi_spmv_mdot": [_vp, _vp, _vp, _vp] + _BASIS + [_vp, _vp],
    "mspi_mdot_basis": [_vp, _vp] + _BASIS + [_i64, _vp, _vp],
    "mspi_maxpy_norm_update": [_vp, _vp, _vp] + _BASIS + [_i64, GmresDev, _i, _i, _vp],
    "mspi_maxpy_norm_update_march": [_vp, _vp, _vp, _vp] + _BASIS + [GmresDev, _i, _vp],
    "mspi_mdot_op": [_vp, _vp, _vp] + _BASIS + [_vp, _vp],
    "mspi_maxpy_norm_update_op": [_vp, _vp, _vp, _vp] + _BASIS + [GmresDev, _i, _vp],
    "mspi_maxpy_norm_basis": [_vp, _vp, _vp] + _BASIS + [_i64, _vp, _vp, _vp],
    "mspi_gm_iter_update": [_vp, GmresDev],
    "mspi_gm_norm_update": [_vp, GmresDev, _vp, _i64, _i],
    "mspi_gm_build": [_vp, GmresDev, _i],
    "mspi_maxpy_accum_basis": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i],
    "mspi_cb_round_store": [_vp, _vp, _vp, _vp, _i64, _vp, _vp],
    "mspi_cb_mdot": [_vp, _vp] + _BASIS + [_i64, _vp, _vp],
    "mspi_cb_maxpy_norm_update": [_vp, _vp, _vp, _vp] + _BASIS + [_i64, GmresDev, _i, _vp],
    "mspi_cb_accum": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i],
    "mspi_gm_wfree": [_vp],
    "mspi_op_fusable": [_vp],
}


def bind() -> C.CDLL:
    """The loaded library with the step entry points' argument types set (all return int)."""
    L = _lib.load()
    for name, args in _SIGS.items():
        f = getattr(L, name)
        f.argtypes, f.restype = args, C.c_int
    return L


def last_error() -> str:
    return _lib.load().msp_get_last_error().decode(errors="replace")


def round_up(n: int, k: int) -> int:
    return (n + k - 1) // k * k


class StepWork:
    """The work buffers of one KSP with restart m on n rows, as msp_ksp_set_up lays them out:

      basis   m + 2 vectors VV(j) = base + j * stride, base 4 KiB aligned, stride = n rounded up to 512 doubles
              (f32: 1024 floats); the pad [n, stride) behind each vector is guard
      w, cur  W and (f32) the current vector: n doubles, then guard up to n rounded to 512 and 512 more
      x       a separate n-vector: the solution BuildSoln accumulates into, or an operand outside the basis
      rec     the recurrence block in msp_ksp_set_up's order -- state (rounded up to 64 bytes), hh (m+2)(m+1), cc,
              ss, grs, h, sc (m + 2 each), hist (max_it + 2) -- zero-filled as that allocation is, followed by a
              spare guarded array

    Each buffer is a window at 512 doubles (4 KiB) into an owned backing Vec and has SLACK guard doubles behind it.
    A region is a named range of one backing: "vv3", "w", "cur", "x", "state", "hh", "cc", "ss", "grs", "h", "sc",
    "hist".  Words outside every region hold GUARD_BITS for good (check_guards); the basis vectors, W and cur start
    as UNWRITTEN_BITS.  snapshot() reads everything back; assert_unchanged() compares two snapshots word for word
    outside the listed exceptions.  Every read-back synchronises the context first."""

    LEAD = 512

    def __init__(self, ctx, n: int, m: int, f32: bool = False, max_it: int | None = None):
        self.ctx, self.n, self.m, self.f32 = ctx, int(n), int(m), bool(f32)
        self.L = bind()
        self.nvec = m + 2
        self.stride = round_up(n, 1024 if f32 else 512)               # in basis elements
        self.max_it = m if max_it is None else int(max_it)
        self.hist_cap = self.max_it + 2
        self.st_words = round_up(C.sizeof(GmresState), 64) // 8
        self.back, self.dtype, self.regions, self._operand = {}, {}, {}, {}
        lead = self.LEAD
        npad = round_up(n, 512)

        sd = self.stride // 2 if f32 else self.stride                   # the stride in doubles
        self._alloc("basis", lead + self.nvec * sd + SLACK, np.float32 if f32 else np.float64)
        k = 2 if f32 else 1
        for j in range(self.nvec):
            self._region(f"vv{j}", "basis", k * lead + j * self.stride, n)
        for name in ("w", "cur", "x"):
            self._alloc(name, lead + npad + SLACK, np.float64)
            self._region(name, name, lead, n)
        nd = (m + 2) * (m + 1) + 5 * (m + 2) + self.hist_cap
        self._alloc("rec", lead + self.st_words + nd + SLACK, np.float64)
        off = lead
        for name, cnt in (("state", self.st_words), ("hh", (m + 2) * (m + 1)), ("cc", m + 2), ("ss", m + 2),
                          ("grs", m + 2), ("h", m + 2), ("sc", m + 2), ("hist", self.hist_cap)):
            self._region(name, "rec", off, cnt)
            off += cnt

        # fill: guards everywhere, then the operands
        for b, vec in self.back.items():
            img = np.full(vec.n, GUARD_BITS, np.uint64).view(self._word(b))
            if self.dtype[b] == np.float32:
                img[:] = GUARD_BITS_F32
            for r, (rb, lo, cnt) in self.regions.items():
                if rb != b:
                    continue
                if b == "rec" or r == "x":
                    img[lo:lo + cnt] = 0
                else:
                    img[lo:lo + cnt] = UNWRITTEN_BITS_F32 if self.dtype[b] == np.float32 else UNWRITTEN_BITS
            vec.set_values(img.view(np.float64))
        base = self.back["basis"].device_ptr() + 8 * lead
        assert base % 4096 == 0, "the basis must start 4 KiB aligned, as the KSP's does"
        self.base = base
        self.g = GmresDev(*[self.ptr(f if f != "st" else "state") for f in DEV_FIELDS])
        self.p_stop = self.ptr("state") + GmresState.stop.offset
        self.p_nbuild = self.ptr("state") + GmresState.nbuild.offset
        rc = self.L.mspi_reserve_partial(ctx.h, self.n)   # as run_cycle does: mspi_maxpy_norm_update does not
        assert rc == 0, last_error()

    # ------------------------------------------------------------------------------------------------ layout
    def _word(self, b):
        return np.uint32 if self.dtype[b] == np.float32 else np.uint64

    def _alloc(self, name, ndoubles, dtype):
        self.back[name] = Vec(self.ctx, ndoubles)
        self.dtype[name] = dtype
        assert self.back[name].device_ptr() % 4096 == 0
        self._operand[name] = np.zeros(ndoubles * (2 if dtype == np.float32 else 1), bool)

    def _region(self, name, backing, lo, cnt):
        """[lo, lo + cnt) of a backing, in elements of its type."""
        self.regions[name] = (backing, lo, cnt)
        self._operand[backing][lo:lo + cnt] = True

    def ptr(self, region: str, index: int = 0) -> int:
        b, lo, _ = self.regions[region]
        return self.back[b].device_ptr() + (lo + index) * np.dtype(self.dtype[b]).itemsize

    def vv(self, j: int) -> int:
        return self.ptr(f"vv{j}")

    # -------------------------------------------------------------------------------------------- host <-> device
    def put(self, region: str, values, index: int = 0):
        """values -> region[index:], element type of the region's backing (f32: an even index and count)."""
        b, lo, cnt = self.regions[region]
        a = np.ascontiguousarray(values, self.dtype[b])
        assert index + a.size <= cnt
        if self.dtype[b] == np.float32:
            assert (lo + index) % 2 == 0 and a.size % 2 == 0
            self.back[b].set_values(a.view(np.float64), (lo + index) // 2)
        else:
            self.back[b].set_values(a, lo + index)

    def put_bits(self, region: str, bits, lo: int = 0, hi: int | None = None):
        """The same bit pattern into region[lo:hi] (f64 regions)."""
        hi = self.regions[region][2] if hi is None else hi
        self.put(region, np.full(hi - lo, bits, np.uint64).view(np.float64), lo)

    def put_vv(self, j: int, values):
        """A basis vector; its pad keeps the guard."""
        v = np.ascontiguousarray(values, self.dtype["basis"])
        if self.f32:
            full = np.full(self.stride, GUARD_BITS_F32, np.uint32).view(np.float32)
            full[:self.n] = v
            b, lo, _ = self.regions[f"vv{j}"]
            self.back[b].set_values(full.view(np.float64), lo // 2)
        else:
            self.put(f"vv{j}", v)

    def snapshot(self) -> dict:
        """Every backing as unsigned words (uint64; the f32 basis as uint32), after a synchronise."""
        self.ctx.synchronize()
        return {b: v.get_array().view(self._word(b)).copy() for b, v in self.back.items()}

    def get(self, region: str, snap: dict | None = None) -> np.ndarray:
        """A region's values (from a snapshot, or read back now)."""
        b, lo, cnt = self.regions[region]
        if snap is None:
            self.ctx.synchronize()
            words = self.back[b].get_array().view(self._word(b))
        else:
            words = snap[b]
        return words[lo:lo + cnt].view(self.dtype[b]).copy()

    def words(self, region: str, snap: dict) -> np.ndarray:
        b, lo, cnt = self.regions[region]
        return snap[b][lo:lo + cnt]

    def _where(self, b, i) -> str:
        for r, (rb, lo, cnt) in self.regions.items():
            if rb == b and lo <= i < lo + cnt:
                return f"{r}[{i - lo}]"
        if b == "basis":
            k = 2 if self.f32 else 1
            j, e = divmod(i - k * self.LEAD, self.stride)
            if 0 <= j < self.nvec:
                return f"the pad of vv{j}, element {e} (n = {self.n})"
        return f"guard word {i} of the {b} buffer"

    def check_guards(self, snap: dict | None = None):
        """Every word outside the regions still holds its guard bits."""
        snap = self.snapshot() if snap is None else snap
        for b, words in snap.items():
            guard = GUARD_BITS_F32 if self.dtype[b] == np.float32 else GUARD_BITS
            bad = np.flatnonzero(~self._operand[b] & (words != guard))
            assert bad.size == 0, (f"{bad.size} guard words of the {b} buffer were overwritten, first: "
                                   f"{self._where(b, int(bad[0]))} = {int(words[bad[0]]):#x}")

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
    def init_state(self, **over):
        """The state msp_ksp_solve pushes before the first cycle: zeroed, rnorm = -1, m, max_it, the default
        tolerances (msp_ksp_get_default_opts) with rtol = 1e-30, scale = 1; over: fields set otherwise."""
        st = GmresState()
        st.rnorm, st.guess_zero, st.m, st.max_it, st.hist_cap = -1.0, 1, self.m, self.max_it, self.hist_cap
        st.rtol, st.abstol, st.divtol, st.haptol, st.breakdowntol, st.scale = 1e-30, 1e-50, 1e4, 1e-30, 0.1, 1.0
        for k, v in over.items():
            setattr(st, k, v)
        self.push_state(st)
        return st

    def push_state(self, st: GmresState):
        raw = np.zeros(self.st_words)
        raw.view(np.uint8)[:C.sizeof(st)] = np.frombuffer(bytes(st), np.uint8)
        self.put("state", raw)

    def state(self, snap: dict | None = None) -> GmresState:
        return GmresState.from_buffer_copy(self.get("state", snap).tobytes()[:C.sizeof(GmresState)])

    def set_stop(self, stop: int = 1):
        st = self.state()
        st.stop = stop
        self.push_state(st)

    # ------------------------------------------------------------------------ the entry points, as enqueue_cycle
    def _basis(self, nv):
        return nv, self.base, self.stride, self.ptr("sc")

    def norm2sq(self):
        return self.L.mspi_norm2sq(self.ctx.h, self.vv(0), self.n, self.ptr("h"))

    def cb_round_store(self, stop: bool = False):
        """cur = rnd(cur), VV(0) the same as float, h[0] its norm; the KSP passes no stop flag (stop=True: st->stop)."""
        return self.L.mspi_cb_round_store(self.ctx.h, self.ptr("cur"), self.ptr("cur"), self.vv(0), self.n,
                                          self.ptr("h"), self.p_stop if stop else None)

    def gm_norm_update(self, partial: int, nchunks: int):
        """The fold + recurrence launch on its own: partial is a device array of nchunks ||w||^2 partials."""
        return self.L.mspi_gm_norm_update(self.ctx.h, self.g, partial, nchunks, self.m)

    def cycle_start(self):
        return self.L.mspi_gm_cycle_start(self.ctx.h, self.g, self.ptr("h"))

    def spmv_scaled(self, A, it, x=None, vout=None):
        """W = A (sc[it] x), x = VV(it) (f32: the current vector) unless given."""
        x = x if x is not None else (self.ptr("cur") if self.f32 else self.vv(it))
        return self.L.mspi_spmv_scaled(A.h, x, self.ptr("sc", it), vout, self.ptr("w"), self.p_stop)

    def spmv_mdot(self, A, it, y: bool, x=None, nv=None):
        """The fused MatMult + MDot over VV(0..nv), nv = it + 1 by default; y: W stored; x = VV(it) unless given."""
        return self.L.mspi_spmv_mdot(A.h, self.vv(it) if x is None else x, self.ptr("sc", it),
                                     self.ptr("w") if y else None, *self._basis(it + 1 if nv is None else nv),
                                     self.ptr("h"), self.p_stop)

    def mdot_basis(self, it):
        return self.L.mspi_mdot_basis(self.ctx.h, self.ptr("w"), *self._basis(it + 1), self.n, self.ptr("h"),
                                      self.p_stop)

    def maxpy_norm_update(self, it):
        return self.L.mspi_maxpy_norm_update(self.ctx.h, self.ptr("w"), self.vv(it + 1), *self._basis(it + 1), self.n,
                                             self.g, it, self.m, self.p_stop)

    def maxpy_norm_update_march(self, A, it, x=None):
        return self.L.mspi_maxpy_norm_update_march(A.h, self.vv(it) if x is None else x, self.ptr("sc", it),
                                                   self.vv(it + 1), *self._basis(it + 1), self.g, self.m, self.p_stop)

    def mdot_op(self, A, it):
        return self.L.mspi_mdot_op(A.h, self.vv(it), self.ptr("sc", it), *self._basis(it + 1), self.ptr("h"),
                                   self.p_stop)

    def maxpy_norm_update_op(self, A, it):
        return self.L.mspi_maxpy_norm_update_op(A.h, self.vv(it), self.ptr("sc", it), self.vv(it + 1),
                                                *self._basis(it + 1), self.g, self.m, self.p_stop)

    def maxpy_norm_basis(self, it):
        """The MSK_TUNE_GM_UNFUSED (128) form of mspi_maxpy_norm_update, first half; then gm_iter_update."""
        return self.L.mspi_maxpy_norm_basis(self.ctx.h, self.ptr("w"), self.vv(it + 1), *self._basis(it + 1), self.n,
                                            self.ptr("h"), self.ptr("h", it + 1), self.p_stop)

    def gm_iter_update(self):
        return self.L.mspi_gm_iter_update(self.ctx.h, self.g)

    def cb_mdot(self, it):
        return self.L.mspi_cb_mdot(self.ctx.h, self.ptr("w"), *self._basis(it + 1), self.n, self.ptr("h"),
                                   self.p_stop)

    def cb_maxpy_norm_update(self, it):
        return self.L.mspi_cb_maxpy_norm_update(self.ctx.h, self.ptr("w"), self.ptr("cur"), self.vv(it + 1),
                                                *self._basis(it + 1), self.n, self.g, self.m, self.p_stop)

    def gm_build(self, m=None):
        return self.L.mspi_gm_build(self.ctx.h, self.g, self.m if m is None else m)

    def accum(self, K):
        """x += sum nrs_j sc[j] VV(j) over the st->nbuild vectors (mspi_maxpy_accum_basis / mspi_cb_accum)."""
        f = self.L.mspi_cb_accum if self.f32 else self.L.mspi_maxpy_accum_basis
        return f(self.ctx.h, self.ptr("x"), self.p_nbuild, self.base, self.stride, self.ptr("sc"), self.n,
                 self.ptr("grs"), K)

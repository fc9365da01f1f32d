"""Guard bands around device vectors and dense storage, and a bit-level comparison (helper, not a test).

TEST INFRASTRUCTURE ONLY.  A freshly created Vec is zero-filled, 4 KiB aligned and followed by at least 512 zero
doubles, so a store past n, a read past n that leaks into a result, or an output row that was never written all
go unnoticed when every operand is such a vector.  The classes here present the library with what
msp_vec_create_with_array documents instead (include/msplit.h): a window of n doubles that is 16-byte aligned,
has 512 readable doubles behind it, and is surrounded by NaNs of a known bit pattern.

  same_bits / assert_same_bits   equality of the uint64 views, NaN against NaN whatever the payload
  Guarded                        a window inside one owned backing Vec, guards before and after it
  DenseGuard                     the pad rows n .. lda of every column of a DenseMat (f64 or f32 storage)
"""
from __future__ import annotations

import numpy as np

from medane_tchakorom_ufc_thesis_repository_amd.petsc import DenseMat, Vec

# quiet NaNs (exponent all ones, top mantissa bit set) with a payload no arithmetic produces
GUARD_BITS = np.uint64(0x7FF8_5EED_0BAD_C0DE)      # around a window, and in the pad word of an odd n
UNWRITTEN_BITS = np.uint64(0x7FF8_F111_0DD0_F111)  # inside an output window before the kernel runs
GUARD_BITS_F32 = np.uint32(0x7FC5_EED1)            # pad rows of a float dense block
UNWRITTEN_BITS_F32 = np.uint32(0x7FCF_111D)

LEADS = (512, 514)   # doubles before the window: 4 KiB aligned, and 16-byte but not 32-byte aligned
SLACK = 512          # readable doubles behind an owned vector's n (msp_vec_create), kept behind a window too


def _bits(a):
    a = np.ascontiguousarray(np.atleast_1d(np.asarray(a, np.float64)))
    return a, a.view(np.uint64)


def same_bits(a, b) -> bool:
    """Equal shapes; where neither side is NaN the uint64 views are equal (so -0.0 is not 0.0 and a subnormal is
    not its neighbour); both sides are NaN at the same places.  NaN sign and payload are not compared: x86 and
    gfx950 propagate them differently."""
    a, ua = _bits(a)
    b, ub = _bits(b)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(ua[~na], ub[~nb]))


def assert_same_bits(got, want, what="result"):
    g, ug = _bits(got)
    w, uw = _bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape}, expected {w.shape}"
    if same_bits(g, w):
        return
    ng, nw = np.isnan(g), np.isnan(w)
    bad = np.flatnonzero((ng != nw) | (~ng & ~nw & (ug != uw)))
    i = np.unravel_index(bad[0], g.shape)
    raise AssertionError(f"{what}: {bad.size} of {g.size} entries differ in their bits, first at {tuple(map(int, i))}: "
                         f"got {g[i]!r} ({int(ug[i]):#018x}), expected {w[i]!r} ({int(uw[i]):#018x})")


class Guarded:
    """A window of n doubles at [lead, lead + n) of one owned backing Vec of lead + n_padded + trail doubles
    (n_padded = n rounded up to even, trail = 512), exposed as .vec = Vec(ctx, n, device_ptr=backing + 8 * lead).
    Everything outside the window -- the lead, the pad word of an odd n, the trail -- holds GUARD_BITS; a kernel
    entitled to read the slack behind an owned vector stays inside the backing allocation, and check() finds any
    word it wrote there."""

    def __init__(self, ctx, n: int, lead: int, window: np.ndarray):
        assert lead in LEADS and n >= 1 and window.shape == (n,)
        self.n, self.lead = int(n), int(lead)
        self.total = lead + n + (n & 1) + SLACK
        self.backing = Vec(ctx, self.total)
        host = np.full(self.total, GUARD_BITS, np.uint64)
        host[lead:lead + n] = np.ascontiguousarray(window, np.float64).view(np.uint64)
        self.backing.set_values(host.view(np.float64))
        self.vec = Vec(ctx, n, device_ptr=self.backing.device_ptr() + 8 * lead)
        assert self.vec.device_ptr() % 16 == 0 and (lead != 514 or self.vec.device_ptr() % 32 == 16)

    @classmethod
    def input(cls, ctx, array, lead: int) -> "Guarded":
        """A window holding array, NaN guards around it."""
        a = np.ascontiguousarray(array, np.float64)
        return cls(ctx, a.size, lead, a)

    @classmethod
    def output(cls, ctx, n: int, lead: int) -> "Guarded":
        """A window holding UNWRITTEN_BITS in every word: after a kernel that writes all of [0, n) none is left
        (assert_written), which a zero-filled vector cannot show for a row whose result is 0.0."""
        return cls(ctx, n, lead, np.full(n, UNWRITTEN_BITS, np.uint64).view(np.float64))

    def get_array(self) -> np.ndarray:
        return self.vec.get_array()

    def check(self):
        """Every guard word still holds its bits."""
        u = self.backing.get_array().view(np.uint64)
        keep = np.ones(self.total, bool)
        keep[self.lead:self.lead + self.n] = False
        bad = np.flatnonzero(keep & (u != GUARD_BITS))
        assert bad.size == 0, (f"{bad.size} guard words around a window of {self.n} doubles (lead {self.lead}) were "
                               f"overwritten, at window offsets {(bad[:8] - self.lead).tolist()}")

    def assert_written(self, rows=None):
        """No word of the window (or of rows) still holds UNWRITTEN_BITS."""
        u = self.get_array().view(np.uint64)
        if rows is not None:
            u = u[rows]
        left = np.flatnonzero(u == UNWRITTEN_BITS)
        assert left.size == 0, f"{left.size} of {u.size} output words were never written, first at {int(left[0])}"


def check_all(*guards):
    for g in guards:
        g.check()


class DenseGuard:
    """The pad rows n .. lda of every column of a DenseMat.  The whole storage is wrapped as one Vec -- lda * ncols
    doubles at device_ptr(), or, for a "single" block, its lda * ncols floats at device_ptr_f32() as
    lda * ncols / 2 doubles (lda is a multiple of 1024 floats there, so the lengths always work out) -- and
    poison() fills the pad rows with GUARD_BITS (GUARD_BITS_F32); check() asserts they still hold them.  Call
    poison() after the entries are set and never zero_entries() after it (that clears the pad rows too)."""

    def __init__(self, ctx, D: DenseMat):
        self.D = D
        self.n, self.s = D.shape
        self.lda = int(D.lda)
        self.f32 = D.get_precision() == "single"
        if self.f32:
            assert (self.lda * self.s) % 2 == 0
            self.vec = Vec(ctx, self.lda * self.s // 2, device_ptr=D.device_ptr_f32())
            self.guard, self.unwritten, self.word = GUARD_BITS_F32, UNWRITTEN_BITS_F32, np.uint32
        else:
            self.vec = Vec(ctx, self.lda * self.s, device_ptr=D.device_ptr())
            self.guard, self.unwritten, self.word = GUARD_BITS, UNWRITTEN_BITS, np.uint64

    def _words(self) -> np.ndarray:
        return self.vec.get_array().view(self.word).reshape(self.s, self.lda)   # [column, row]

    def poison(self, entries: bool = False):
        """Pad rows <- guard bits; entries=True also fills rows [0, n) with the unwritten pattern (an output)."""
        w = self._words().copy()
        w[:, self.n:] = self.guard
        if entries:
            w[:, :self.n] = self.unwritten
        self.vec.set_values(w.reshape(-1).view(np.float64))

    def check(self):
        pad = self._words()[:, self.n:]
        bad = np.argwhere(pad != self.guard)
        assert bad.size == 0, (f"{len(bad)} pad words of a {self.n} x {self.s} dense block (lda {self.lda}) were "
                               f"overwritten, first in column {int(bad[0][0])} row {self.n + int(bad[0][1])}")

    def assert_written(self):
        left = np.argwhere(self._words()[:, :self.n] == self.unwritten)
        assert left.size == 0, f"{len(left)} entries of the dense block were never written"

"""The four block16 launchers (mspi_cb16_*, msplit_cgs_basis.hip) one call at a time, on guarded buffers.

The f64 operands -- W, the current vector, x, the recurrence block -- are a tests/gmres_step.py StepWork; the block16
basis is a buffer of this module laid out as msp_ksp_set_up lays it out: 33 vectors of stride = n rounded up to 2048
int16 from a 4 KiB aligned base, the int32 exponent table [vector][chunk] behind the last one, and a known 16-bit
pattern in every word before the first call.  Each call is followed by a read-back of everything: the outputs are
held to tests/basis_b16.py and pyoracle's DBR primitives bit for bit, every other word -- the pads [n, stride), the
int16 words and exponent slots of the other vectors, the guards -- is unchanged, and under a set stop flag nothing
is stored at all.

The stored words are compared too.  The layout inside a full chunk is two lane-contiguous halves (the element at DBR
position lane t, slice j, half k of chunk c is int16 4096c + 2048 (j / 4) + 8t + 2 (j % 4) + k); a partial last chunk
is in natural order.
"""
import ctypes as C

import numpy as np
import pytest

import basis_b16 as b16
import gmres_step as gs
from guarded import SLACK, UNWRITTEN_BITS, assert_same_bits

pytestmark = pytest.mark.gpu

CHUNK = 4096
M = 31                       # restart: vectors 0..31 are read, vector 32 is the MAXPY's output slot
NVEC = M + 2
NVS = (1, 2, 3, 4, 5, 31)
GUARD16 = np.uint16(0x5EED)
NONFINITE = -2 ** 31         # the exponent slot of a chunk that held a NaN or an inf

_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
_SIGS = {
    "mspi_cb16_round_store": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp],
    "mspi_cb16_mdot": [_vp, _vp, _i, _vp, _i64, _vp, _vp, _i64, _vp, _vp],
    "mspi_cb16_maxpy_norm_update": [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i64, _vp, _vp, _i64, gs.GmresDev, _i, _vp],
    "mspi_cb16_accum": [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i],
}


def stored_index(n):
    """int16 index of element e of a vector of n entries."""
    e = np.arange(n)
    c, l = e // CHUNK, e % CHUNK
    j, t, k = l // 512, (l % 512) // 2, l % 2
    return np.where((c + 1) * CHUNK <= n, c * CHUNK + 2048 * (j // 4) + 8 * t + 2 * (j % 4) + k, e)


class Work:
    def __init__(self, ctx, n):
        from medane_tchakorom_ufc_thesis_repository_amd.petsc import Vec
        self.ctx, self.n = ctx, n
        self.wk = wk = gs.StepWork(ctx, n, M, f32=True)
        self.L = wk.L
        for name, args in _SIGS.items():
            f = getattr(self.L, name)
            f.argtypes, f.restype = args, C.c_int
        self.stride = gs.round_up(n, 2048)
        self.nch = (n + CHUNK - 1) // CHUNK
        self.vv_words = NVEC * self.stride                       # int16
        nbytes = 2 * self.vv_words + 4 * NVEC * self.nch
        self.lead = 512
        self.total = self.lead + (nbytes + 7) // 8 + SLACK       # doubles
        self.back = Vec(ctx, self.total)
        self.back.set_values(np.full(4 * self.total, GUARD16, np.uint16).view(np.float64))
        self.base = self.back.device_ptr() + 8 * self.lead
        assert self.base % 4096 == 0
        self.ebase = self.base + 2 * self.vv_words
        self.idx = stored_index(n)
        self.D = None

    # layout
    def vv(self, j):
        return self.base + 2 * j * self.stride

    def ex(self, j):
        return self.ebase + 4 * j * self.nch

    def snapshot(self):
        """(the StepWork's snapshot, the basis buffer as uint16)."""
        s = self.wk.snapshot()
        return s, self.back.get_array().view(np.uint16).copy()

    def q_of(self, j, words):
        lo = 4 * self.lead + j * self.stride
        return words[lo:lo + self.stride].view(np.int16)

    def e_of(self, j, words):
        lo = 4 * self.lead + self.vv_words + 2 * j * self.nch
        return words[lo:lo + 2 * self.nch].view(np.int32)

    def assert_basis_unchanged(self, before, after, except_vec=None, what=""):
        """Word for word, outside the int16 entries [0, n) and the exponent slots of one vector."""
        free = np.zeros(before.size, bool)
        if except_vec is not None:
            lo = 4 * self.lead + except_vec * self.stride
            free[lo:lo + self.n] = True
            lo = 4 * self.lead + self.vv_words + 2 * except_vec * self.nch
            free[lo:lo + 2 * self.nch] = True
        bad = np.flatnonzero(~free & (before != after))
        assert bad.size == 0, (f"{what}: {bad.size} 16-bit words of the basis buffer changed, first at int16 "
                               f"{int(bad[0]) - 4 * self.lead} of the basis (n {self.n}, stride {self.stride}): "
                               f"{int(before[bad[0]]):#x} -> {int(after[bad[0]]):#x}")

    def assert_stored(self, j, words, v, what):
        """Vector j holds block16's integers and exponents of v, in the kernels' layout; its pad is untouched."""
        q, E = b16.quantise(v)
        got = self.q_of(j, words)
        finite = np.repeat([e is not None for e in E], CHUNK)[:self.n]
        assert np.array_equal(got[self.idx][finite], q[finite]), f"{what}: the int16 words of vector {j}"
        assert np.array_equal(self.e_of(j, words), [NONFINITE if e is None else e for e in E]), \
            f"{what}: the exponents of vector {j}"
        used = np.zeros(self.stride, bool)
        used[self.idx] = True
        assert np.all(got.view(np.uint16)[~used] == GUARD16), f"{what}: the pad of vector {j}"

    # the launchers
    def round_store(self, j, stop=False):
        wk = self.wk
        return self.L.mspi_cb16_round_store(self.ctx.h, wk.ptr("cur"), wk.ptr("cur"), self.vv(j), self.ex(j), self.n,
                                            wk.ptr("h"), wk.p_stop if stop else None)

    def mdot(self, nv):
        wk = self.wk
        return self.L.mspi_cb16_mdot(self.ctx.h, wk.ptr("w"), nv, self.base, self.stride, self.ebase, wk.ptr("sc"),
                                     self.n, wk.ptr("h"), wk.p_stop)

    def maxpy_norm_update(self, nv, out):
        wk = self.wk
        return self.L.mspi_cb16_maxpy_norm_update(self.ctx.h, wk.ptr("w"), wk.ptr("cur"), self.vv(out), self.ex(out),
                                                  nv, self.base, self.stride, self.ebase, wk.ptr("sc"), self.n, wk.g,
                                                  M, wk.p_stop)

    def accum(self, nv):
        wk = self.wk
        return self.L.mspi_cb16_accum(self.ctx.h, wk.ptr("x"), wk.p_nbuild, self.base, self.stride, self.ebase,
                                      wk.ptr("sc"), self.n, wk.ptr("grs"), nv)


def _crafted(n, r):
    """Vector 0: the clamp, a tie in each direction, and (where n has the chunks) a zero chunk between non-zero
    chunks and a chunk whose maximum is subnormal."""
    v = r.uniform(-0.9, 0.9, n)
    u = 2.0 ** -15                                   # chunk 0: E = 0
    special = [1.0 - 2.0 ** -20, 0.5, 0.5 * u, 1.5 * u, 2.5 * u, -0.5 * u, -1.5 * u, -2.5 * u, -0.0]
    k = min(len(special), n)
    v[:k] = special[:k]
    if n > CHUNK + 1:                                # 8193: [crafted][zero][one entry]
        v[CHUNK:2 * CHUNK] = 0.0
        v[CHUNK + 5] = -0.0
    return v


def _subnormal_max(n, r):
    """Every chunk's maximum is subnormal (the last full one's, or the only one's, is the smallest subnormal)."""
    v = r.integers(-3, 4, n).astype(np.float64) * 2.0 ** -1074
    v[0] = 5 * 2.0 ** -1074
    lo = (n - 1) // CHUNK * CHUNK
    v[lo:] = 0.0
    v[n - 1] = -2.0 ** -1074
    return v


def _vectors(n):
    r = np.random.default_rng(1000 + n)
    V = [_crafted(n, r), _subnormal_max(n, r)]
    while len(V) < M + 1:
        V.append(r.standard_normal(n) * 10.0 ** r.integers(-3, 4, n) * 10.0 ** r.integers(-30, 30))
    return V, r


def _store_all(wkb, V, oracle, check=True):
    wk, D = wkb.wk, oracle.REDUCE_DBR
    S = []
    _, words = wkb.snapshot()
    for j, v in enumerate(V):
        s = b16.block16(v)
        S.append(s)
        wk.put("cur", v)
        wk.put_bits("h", UNWRITTEN_BITS, 0, 1)
        before = wk.snapshot()
        assert wkb.round_store(j) == 0, gs.last_error()
        if not check:
            continue
        what = f"mspi_cb16_round_store of vector {j}"
        after, new = wkb.snapshot()
        wk.check_guards(after)
        wk.assert_unchanged(before, after, ["cur", ("h", 0, 1)], what)
        assert_same_bits(wk.get("cur", after), s, f"{what}: the current vector")
        with np.errstate(all="ignore"):
            assert_same_bits(wk.get("h", after)[0], oracle.dot(s, s, D), f"{what}: the sum of squares")
        wkb.assert_basis_unchanged(words, new, j, what)
        wkb.assert_stored(j, new, v, what)
        words = new
    return S


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 8193])
def test_block16_launchers_one_call_at_a_time(ctx, oracle, n):
    D = oracle.REDUCE_DBR
    wkb = Work(ctx, n)
    wk = wkb.wk
    V, r = _vectors(n)
    wk.init_state()
    S = _store_all(wkb, V, oracle)
    sc = r.uniform(0.5, 2.0, M + 2)
    Vs = [s * sc[j] for j, s in enumerate(S)]
    out = M + 1
    for nv in NVS:
        # MDot
        w = r.uniform(-1, 1, n)
        wk.init_state()
        wk.put("sc", sc)
        wk.put("w", w)
        wk.put_bits("h", UNWRITTEN_BITS, 0, nv)
        before, words = wkb.snapshot()
        assert wkb.mdot(nv) == 0, gs.last_error()
        after, new = wkb.snapshot()
        what = f"mspi_cb16_mdot, nv {nv}"
        wk.check_guards(after)
        wk.assert_unchanged(before, after, [("h", 0, nv)], what)
        wkb.assert_basis_unchanged(words, new, None, what)
        assert_same_bits(wk.get("h", after)[:nv], oracle.mdot(w, Vs[:nv], D), f"{what}: h")
        # MAXPY + norm + update: the coefficients wait in h(0..nv-1), the recurrence is at it = nv - 1
        h = r.uniform(-1, 1, nv)
        wk.init_state(it=nv - 1, its=nv - 1, res=1.0)
        wk.put("h", h)
        wk.put_bits("cur", UNWRITTEN_BITS)
        before, words = wkb.snapshot()
        assert wkb.maxpy_norm_update(nv, out) == 0, gs.last_error()
        after, new = wkb.snapshot()
        what = f"mspi_cb16_maxpy_norm_update, nv {nv}"
        m2 = M + 2
        wk.check_guards(after)
        wk.assert_unchanged(before, after, ["cur", ("h", nv, nv + 1), ("sc", nv, nv + 1), "hist", "state",
                                            ("hh", (nv - 1) * m2, (nv - 1) * m2 + nv + 1), ("cc", nv - 1, nv),
                                            ("ss", nv - 1, nv), ("grs", nv - 1, nv + 1)], what)
        wkb.assert_basis_unchanged(words, new, out, what)
        v = oracle.maxpy(w, -h, Vs[:nv])
        s = b16.block16(v)
        q = oracle.dot(s, s, D)
        assert_same_bits(wk.get("cur", after), s, f"{what}: the current vector")
        assert_same_bits(wk.get("h", after)[nv], q, f"{what}: the sum of squares")
        assert_same_bits(wk.get("sc", after)[nv], 1.0 / np.sqrt(q) if q != 0.0 else 1.0, f"{what}: sc")
        wkb.assert_stored(out, new, v, what)
        # BuildSoln's accumulate
        coef, x = r.uniform(-1, 1, nv), r.uniform(-1, 1, n)
        wk.init_state(nbuild=nv)
        wk.put("sc", sc)
        wk.put("grs", coef)
        wk.put("x", x)
        before, words = wkb.snapshot()
        assert wkb.accum(nv) == 0, gs.last_error()
        after, new = wkb.snapshot()
        what = f"mspi_cb16_accum, nv {nv}"
        wk.check_guards(after)
        wk.assert_unchanged(before, after, ["x"], what)
        wkb.assert_basis_unchanged(words, new, None, what)
        assert_same_bits(wk.get("x", after), x + 1.0 * oracle.maxpy(np.zeros(n), coef, Vs[:nv]), f"{what}: x")
    # the stop flag: success, and no store
    nv = 5
    wk.init_state(it=nv - 1, its=nv - 1, res=1.0, stop=1)
    wk.put("sc", sc)
    wk.put_bits("h", UNWRITTEN_BITS, 0, nv + 1)
    wk.put_bits("cur", UNWRITTEN_BITS)
    before, words = wkb.snapshot()
    for what, call in (("mspi_cb16_round_store", lambda: wkb.round_store(out, stop=True)),
                       ("mspi_cb16_mdot", lambda: wkb.mdot(nv)),
                       ("mspi_cb16_maxpy_norm_update", lambda: wkb.maxpy_norm_update(nv, out))):
        assert call() == 0, (what, gs.last_error())
        after, new = wkb.snapshot()
        wk.assert_unchanged(before, after, what=f"{what} under stop")
        wkb.assert_basis_unchanged(words, new, None, f"{what} under stop")
    # BuildSoln has no stop by design: with nbuild = 0 it combines nothing
    wk.init_state(nbuild=0)
    before, words = wkb.snapshot()
    assert wkb.accum(nv) == 0, gs.last_error()
    after, new = wkb.snapshot()
    wk.assert_unchanged(before, after, what="mspi_cb16_accum with nbuild = 0")
    wkb.assert_basis_unchanged(words, new, None, "mspi_cb16_accum with nbuild = 0")


@pytest.mark.parametrize("n", [4097, 8193])
def test_non_finite_entries_poison_their_chunk_only(ctx, oracle, n):
    """A NaN in the first chunk only and an inf in the partial last chunk only: exactly that chunk reads back NaN,
    in the current vector and through MDot, MAXPY and the accumulate; the sum of squares is NaN."""
    D = oracle.REDUCE_DBR
    wkb = Work(ctx, n)
    wk = wkb.wk
    r = np.random.default_rng(n)
    V = [r.uniform(-1, 1, n) for _ in range(3)]
    V[0][7] = np.nan
    V[2][n - 1] = -np.inf
    wk.init_state()
    S = _store_all(wkb, V, oracle)
    assert np.all(np.isnan(S[0][:CHUNK])) and not np.any(np.isnan(S[0][CHUNK:]))
    last = (n - 1) // CHUNK * CHUNK
    assert np.all(np.isnan(S[2][last:])) and not np.any(np.isnan(S[2][:last]))
    sc = r.uniform(0.5, 2.0, M + 2)
    Vs = [s * sc[j] for j, s in enumerate(S)]
    nv, out = 3, 3
    w, h, coef, x = r.uniform(-1, 1, n), r.uniform(-1, 1, nv), r.uniform(-1, 1, nv), r.uniform(-1, 1, n)
    with np.errstate(all="ignore"):
        wk.put("sc", sc)
        wk.put("w", w)
        assert wkb.mdot(nv) == 0, gs.last_error()
        got = wk.get("h")[:nv]
        assert_same_bits(got, oracle.mdot(w, Vs, D), "mspi_cb16_mdot: h")
        assert np.isnan(got[0]) and np.isfinite(got[1]) and np.isnan(got[2])
        wk.init_state(it=nv - 1, its=nv - 1, res=1.0)
        wk.put("h", h)
        _, words = wkb.snapshot()
        assert wkb.maxpy_norm_update(nv, out) == 0, gs.last_error()
        after, new = wkb.snapshot()
        v = oracle.maxpy(w, -h, Vs)
        s = b16.block16(v)
        assert_same_bits(wk.get("cur", after), s, "mspi_cb16_maxpy_norm_update: the current vector")
        assert np.isnan(wk.get("h", after)[nv])
        wkb.assert_basis_unchanged(words, new, out, "mspi_cb16_maxpy_norm_update")
        wkb.assert_stored(out, new, v, "mspi_cb16_maxpy_norm_update")
        wk.init_state(nbuild=nv)
        wk.put("sc", sc)
        wk.put("grs", coef)
        wk.put("x", x)
        assert wkb.accum(nv) == 0, gs.last_error()
        assert_same_bits(wk.get("x"), x + 1.0 * oracle.maxpy(np.zeros(n), coef, Vs), "mspi_cb16_accum: x")
    wk.check_guards()

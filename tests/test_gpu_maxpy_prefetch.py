"""The one-plane form of the W-free CGS MAXPY (k_box_maxpy_march with msk_set_maxpy_prefetch != 0).

Where the kernel runs one plane per workgroup (the default) the one-plane form carries no x planes, reads x(z) back
from its own LDS window and issues the loads of the first vector group's first two vectors under the stencil
prologue; its wide form streams two groups of four per burst.  Only the order in which loads are issued differs
from the marched form, so everything here is bit for bit: whole solves against the marched form (switch 0), the
stored-W step (msk_set_gm_wfree(0)) and the DBR oracle, over both burst widths and the launcher's own choice; one
launcher call at a time on guarded buffers (tests/gmres_step.py) against the oracle's step; the stop flag; the
re-keying of captured cycles; and the paths the switch must leave alone (MSPLIT_MAXPY_ZT=2) or combine with
(MSPLIT_MAXPY_REV=1, the top-planes-first workgroup order).
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
from contextlib import contextmanager

import numpy as np
import pytest

import gmres_step as gs
from guarded import UNWRITTEN_BITS
from medane_tchakorom_ufc_thesis_repository_amd import _lib
from medane_tchakorom_ufc_thesis_repository_amd.petsc import KSP, Mat, Options, Vec
from test_gpu_gmres_step import Driver, Kind, _box, _box_reached, _rhs
from test_gpu_wfree import wfree

pytestmark = pytest.mark.gpu

SEED = 20261021
PECLET = (0.5, -0.25, 0.3)
MODES = [1, 2, 3]            # the launcher's choice, the 4-vector burst, the 8-vector burst


def _L():
    L = _lib.load()
    L.msk_set_maxpy_prefetch.argtypes = [ctypes.c_int]
    L.msk_set_maxpy_prefetch.restype = None
    L.msk_get_maxpy_prefetch.restype = ctypes.c_int
    L.msk_get_shape_epoch.restype = ctypes.c_int
    return L


@contextmanager
def switched(get, set_, value):
    """A library switch with a getter and a setter, at value inside the block and back at what it was after it."""
    old = get()
    set_(value)
    try:
        assert get() == value
        yield
    finally:
        set_(old)


def prefetch(mode):
    L = _L()
    return switched(L.msk_get_maxpy_prefetch, L.msk_set_maxpy_prefetch, mode)


def _make(ctx, shape, peclet):
    nx, ny, nz = shape
    if peclet is None:
        return Mat.box_stencil(ctx, 3, nx, ny, nz)
    return Mat.box_convdiff(ctx, 3, nx, ny, nz, False, False, peclet)


def _ksp(ctx, A, restart, max_it):
    ksp = KSP(ctx)
    ksp.set_operators(A)
    ksp.set_from_options(Options(f"-ksp_type gmres -pc_type none -ksp_norm_type unpreconditioned "
                                 f"-ksp_gmres_restart {restart} -ksp_max_it {max_it} -ksp_rtol 1e-30"))
    return ksp


def _run(ctx, ksp, b):
    x = Vec(ctx, b.size)
    ksp.solve(Vec.from_array(ctx, b), x)
    return ksp.get_iteration_number(), ksp.get_residual_history(), x.get_array()


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


_refs = {}


def _reference(ctx, oracle, shape, peclet, restart, max_it, seed=SEED):
    """(A, b, result) with the result of the marched form (switch 0), once per case and never modified; it is held
    to the stored-W step and to the oracle here, so every mode is compared with all three."""
    key = (shape, peclet, restart, max_it, seed)
    if key not in _refs:
        A = _make(ctx, shape, peclet)
        n = A.shape[0]
        b = np.random.default_rng(seed).uniform(-1, 1, n)
        with prefetch(0):
            with wfree(1):
                ref = _run(ctx, _ksp(ctx, A, restart, max_it), b)
            with wfree(0):
                stored = _run(ctx, _ksp(ctx, A, restart, max_it), b)
        O = oracle.Mat.from_arrays(n, n, *A.get_csr())
        xo, ro = oracle.gmres(O, b, reduce_mode=oracle.REDUCE_DBR, guess_nonzero=0, restart=restart, max_it=max_it,
                              rtol=1e-30)
        assert _same(ref, stored) and _same(ref, (ro["its"], ro["hist"], xo))
        _refs[key] = (A, b, ref)
    return _refs[key]


# (64, 64, 1): a single plane, no z neighbours; (2048, 2, 3): halo lines longer than the workgroup, the strided
# halo loop; (512, 256, 2): 32 tiles per plane, the XCD-contiguous workgroup order (the others take the plain one)
SHAPES = [(64, 64, 1), (64, 64, 2), (64, 64, 3), (2048, 2, 3), (256, 16, 7), (512, 256, 2)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("peclet", [None, PECLET])
def test_whole_solves_bitwise(ctx, oracle, peclet, shape, mode):
    """GMRES(30) over 34 iterations (every nv 1..30, then the start of a second cycle)."""
    A, b, ref = _reference(ctx, oracle, shape, peclet, 30, 34)
    with prefetch(mode), wfree(1):
        assert _same(_run(ctx, _ksp(ctx, A, 30, 34), b), ref)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("restart", [1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 31, 32])
def test_every_group_shape(ctx, oracle, restart, mode):
    """nv over every nv & 3, with no full group, one, an even and an odd number of them (the wide form's pairs, its
    single group before the last, its last group alone)."""
    A, b, ref = _reference(ctx, oracle, (64, 64, 3), None, restart, 2 * restart + 2, seed=SEED + restart)
    with prefetch(mode), wfree(1):
        assert _same(_run(ctx, _ksp(ctx, A, restart, 2 * restart + 2), b), ref)


@pytest.mark.parametrize("timing", [False, True])
def test_eager_and_captured_one_ksp(ctx, oracle, timing):
    """Per-kernel timing on: eager launches; off: the cycle is captured once and replayed as a HIP graph.  The
    switch is flipped between solves of ONE KSP: the setter bumps the shape epoch, which is part of the graph key,
    so each setting replays a capture of its own kernels."""
    A, b, ref = _reference(ctx, oracle, (128, 64, 4), None, 30, 64)
    L = _L()
    ksp = _ksp(ctx, A, 30, 64)
    ctx.set_timing(timing)
    try:
        with wfree(1):
            for mode in (0, 2, 0, 3, 1, 0):
                e0 = L.msk_get_shape_epoch()
                with prefetch(mode):
                    assert L.msk_get_shape_epoch() > e0
                    assert _same(_run(ctx, ksp, b), ref), mode
                    assert _same(_run(ctx, ksp, b), ref), mode      # the replay of that setting's capture
    finally:
        ctx.set_timing(False)


# ------------------------------------------------------------------------------- one launcher call, guarded buffers
class PrefetchKind(Kind):
    """The W-free step with the one-plane form switched on."""

    def __init__(self, mode, *a, **k):
        super().__init__(*a, **k)
        self.mode = mode

    @contextmanager
    def active(self, monkeypatch):
        with super().active(monkeypatch), prefetch(self.mode):
            yield


_ops = {}


def _kind(ctx, oracle, shape, mode):
    if shape not in _ops:
        A = _box(*shape)(ctx)
        _ops[shape] = (A, oracle.Mat.from_arrays(A.shape[0], A.shape[0], *A.get_csr()))
    return (PrefetchKind(mode, "wfree", _box(*shape), reached=_box_reached(*shape, 1)),) + _ops[shape]


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("shape", [(64, 64, 3), (64, 64, 5)])
def test_launcher_on_guarded_buffers(ctx, oracle, shape, mode, monkeypatch):
    """mspi_maxpy_norm_update_march at nv = 1 .. 9 (1, 2, 3, 4, 5, 8, 9 among them), each call followed by a
    read-back of everything: VV(it + 1), the ||.||^2 it folds and the recurrence block are the oracle's bits, and
    every pad, tail and other basis vector is unchanged (the guards are NaNs: one read into a result would show)."""
    kind, A, O = _kind(ctx, oracle, shape, mode)
    with kind.active(monkeypatch):
        d = Driver(ctx, oracle, kind, A, O, _rhs(A.shape[0]))
        for it in range(9):
            d.step(it)
        for j in range(10):
            assert not np.isnan(d.wk.get(f"vv{j}")).any()
        assert not np.isnan(d.wk.get("h")[:10]).any() and not np.isnan(d.wk.get("sc")[:10]).any()


@pytest.mark.parametrize("mode", [2, 3])
def test_stop_flag_makes_the_launch_a_no_op(ctx, oracle, mode, monkeypatch):
    """With st->stop set the launch returns success and stores nothing: VV(it + 1) keeps its unwritten pattern and
    no other word changes."""
    kind, A, O = _kind(ctx, oracle, (64, 64, 3), mode)
    it = 5
    with kind.active(monkeypatch):
        d = Driver(ctx, oracle, kind, A, O, _rhs(A.shape[0]), check=False)
        for j in range(it):
            d.step(j)
        d.wk.set_stop(1)
        before = d.wk.snapshot()
        assert (d.wk.words(f"vv{it + 1}", before) == UNWRITTEN_BITS).all()
        assert d.wk.maxpy_norm_update_march(A, it) == 0, gs.last_error()
        after = d.wk.assert_unchanged(before, what="mspi_maxpy_norm_update_march under stop")
        d.wk.check_guards(after)


# ------------------------------------------------------------------- settings read once per process: subprocesses
_ENV_SCRIPT = r"""
import ctypes, hashlib, json, sys
import numpy as np
import torch
from medane_tchakorom_ufc_thesis_repository_amd import _lib
from medane_tchakorom_ufc_thesis_repository_amd.petsc import KSP, Context, Mat, Options, Vec
L = _lib.load()
L.msk_set_maxpy_prefetch.argtypes = [ctypes.c_int]
L.msk_set_maxpy_prefetch.restype = None
ctx = Context(0)
A = Mat.box_stencil(ctx, 3, 64, 64, 5)
n = A.shape[0]
b = Vec.from_array(ctx, np.random.default_rng(7).uniform(-1, 1, n))
out = {}
for mode in (0, 2, 3):
    L.msk_set_maxpy_prefetch(mode)
    ksp = KSP(ctx)
    ksp.set_operators(A)
    ksp.set_from_options(Options("-ksp_type gmres -pc_type none -ksp_norm_type unpreconditioned "
                                 "-ksp_gmres_restart 30 -ksp_max_it 40 -ksp_rtol 1e-30"))
    x = Vec(ctx, n)
    ksp.solve(b, x)
    out[str(mode)] = {"hist": [float(h).hex() for h in ksp.get_residual_history()],
                      "x": hashlib.sha256(x.get_array().tobytes()).hexdigest()}
print(json.dumps(out))
"""


def _in_process(env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _ENV_SCRIPT], env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=240, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_zt_and_rev_settings(ctx, oracle):
    """MSPLIT_MAXPY_ZT=2 (two planes per workgroup: the switch must leave the marched form in place) and
    MSPLIT_MAXPY_REV=1 (top planes first, with the one-plane form) are read once per process; both together start
    on the ragged top group (nz = 5: plane 4 alone).  Each process solves with the switch at 0, 2 and 3; every
    result is this process's oracle-checked reference."""
    A, b, ref = _reference(ctx, oracle, (64, 64, 5), None, 30, 40, seed=7)
    want = {"hist": [float(h).hex() for h in ref[1]], "x": hashlib.sha256(ref[2].tobytes()).hexdigest()}
    for env in ({"MSPLIT_MAXPY_ZT": "2"}, {"MSPLIT_MAXPY_REV": "1"}, {"MSPLIT_MAXPY_ZT": "2", "MSPLIT_MAXPY_REV": "1"}):
        got = _in_process(env)
        for mode in ("0", "2", "3"):
            assert got[mode] == want, (env, mode)

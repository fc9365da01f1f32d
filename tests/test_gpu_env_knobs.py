"""Kernels that only an environment knob read once per process selects.

  MSPLIT_RV_PREFETCH=4|2       k_box_spmv_mdot_march<., ., 1, 4|2>: the stencil storage's fused MatMult + MDot with four
                               or two row pairs' values loaded before the barriers (the default loads all eight)
  MSPLIT_MAXPY_MARCH_U2=1      k_box_maxpy_march<33, true, 0>: the W-free MAXPY's group loop unrolled by two
  MSPLIT_BOXMDOT_ZT, _REV      the fused kernels' planes per workgroup and their top-groups-first order

They ship with the promise "same bits" and no test launched them.  One fresh process per setting solves GMRES(30)
over 40 iterations on the 64 x 64 x 5 Poisson box (DV storage, the W-free step) and on the same box with per-cell
coefficients made unsymmetric (STENCIL storage, k_box_march_chunk_rv, W stored); history and x must be this
process's, which are the oracle's.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from medane_tchakorom_ufc_thesis_repository_amd.petsc import KSP, Mat, Options, Vec
from medane_tchakorom_ufc_thesis_repository_amd.utils import heterogeneous_poisson3d
from test_gpu_dv import _unsymmetric

pytestmark = pytest.mark.gpu

SHAPE = (64, 64, 5)
OPTS = ("-ksp_type gmres -pc_type none -ksp_norm_type unpreconditioned -ksp_gmres_restart 30 -ksp_max_it 40 "
        "-ksp_rtol 1e-30")

_CHILD = r"""
import hashlib, json, sys
import numpy as np
from medane_tchakorom_ufc_thesis_repository_amd.petsc import KSP, Context, Mat, Options, Vec
ctx = Context(0)
csr = np.load(sys.argv[1])
N = len(csr["rp"]) - 1
ops = {"dv": Mat.box_stencil(ctx, 3, 64, 64, 5), "stencil": Mat.from_csr(ctx, N, N, csr["rp"], csr["col"], csr["val"])}
out = {}
for name, A in ops.items():
    n = A.shape[0]
    ksp = KSP(ctx)
    ksp.set_operators(A)
    ksp.set_from_options(Options(sys.argv[2]))
    x = Vec(ctx, n)
    ksp.solve(Vec.from_array(ctx, np.random.default_rng(7).uniform(-1, 1, n)), x)
    out[name] = {"storage": A.get_storage(), "kernel": A.spmv_kernel(),
                 "hist": [float(h).hex() for h in ksp.get_residual_history()],
                 "x": hashlib.sha256(x.get_array().tobytes()).hexdigest()}
print(json.dumps(out))
"""

_state = {}


def _reference(ctx, oracle, tmp_path_factory):
    """The parent's own solves, held to the oracle, and the file the children read the unsymmetric operator from."""
    if not _state:
        rp, col, val = heterogeneous_poisson3d(*SHAPE)
        val = _unsymmetric(rp, col, val)
        N = len(rp) - 1
        path = str(tmp_path_factory.mktemp("env_knobs") / "unsymmetric.npz")
        np.savez(path, rp=rp, col=col, val=val)
        want = {}
        for name, A in (("dv", Mat.box_stencil(ctx, 3, *SHAPE)), ("stencil", Mat.from_csr(ctx, N, N, rp, col, val))):
            n = A.shape[0]
            b = np.random.default_rng(7).uniform(-1, 1, n)
            ksp = KSP(ctx)
            ksp.set_operators(A)
            ksp.set_from_options(Options(OPTS))
            x = Vec(ctx, n)
            ksp.solve(Vec.from_array(ctx, b), x)
            O = oracle.Mat.from_arrays(n, n, *A.get_csr())
            xo, ro = oracle.gmres(O, b, reduce_mode=oracle.REDUCE_DBR, guess_nonzero=0, restart=30, max_it=40,
                                  rtol=1e-30)
            assert ro["its"] == 40 and np.array_equal(ksp.get_residual_history(), ro["hist"])
            assert np.array_equal(x.get_array(), xo)
            want[name] = {"storage": A.get_storage(), "kernel": A.spmv_kernel(),
                          "hist": [float(h).hex() for h in ro["hist"]], "x": hashlib.sha256(xo.tobytes()).hexdigest()}
        assert (want["dv"]["storage"], want["dv"]["kernel"]) == ("dv", "k_spmv_box_march")
        assert (want["stencil"]["storage"], want["stencil"]["kernel"]) == ("stencil", "k_box_march_chunk_rv")
        _state.update(path=path, want=want)
    return _state["path"], _state["want"]


@pytest.mark.parametrize("env", [{"MSPLIT_RV_PREFETCH": "4"}, {"MSPLIT_RV_PREFETCH": "2"},
                                 {"MSPLIT_MAXPY_MARCH_U2": "1"},
                                 {"MSPLIT_BOXMDOT_ZT": "3", "MSPLIT_BOXMDOT_REV": "1"}, {"MSPLIT_BOXMDOT_ZT": "1"}],
                         ids=lambda e: ",".join(f"{k[7:]}={v}" for k, v in e.items()))
def test_knob_selected_kernels_give_the_same_bits(ctx, oracle, tmp_path_factory, env):
    path, want = _reference(ctx, oracle, tmp_path_factory)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD, path, OPTS], env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=240, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == want, env

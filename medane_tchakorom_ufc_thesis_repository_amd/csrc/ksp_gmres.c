/*
 * ksp_gmres.c -- KSPGMRES host logic over device-resident Krylov vectors.
 *
 * Restates PETSc 3.22.1's KSPSolve_GMRES / KSPGMRESCycle / classical
 * Gram-Schmidt (KSP_GMRES_CGS_REFINE_NEVER, one pass, by default; msp_ksp_set_cgs_refinement: REFINE_IFNEEDED and
 * REFINE_ALWAYS, a second pass decided on the device) / KSPGMRESUpdateHessenberg / KSPGMRESBuildSoln /
 * KSPConvergedDefault with PCNONE -- the inner solve the reference calls from
 * inner_solver() (src/utils/utils.c:950-970) and gmres_solution.c:70.
 *
 * This file also holds what both KSP types share (struct msp_ksp is in ksp_impl.h): creation, options, the
 * preconditioner's set-up, the graph cache and the result getters; msp_ksp_set_up and msp_ksp_solve hand a KSP of
 * type MSP_KSP_CG to ksp_cg.c.
 *
 * Division of labour.  This file owns the solve: options, the restart loop of
 * KSPSolve_GMRES, the order of every operation, and the decision to start
 * another cycle.  The per-iteration scalar steps of KSPGMRESCycle (Givens
 * update, happy-breakdown and convergence tests, residual history) run in
 * one-lane device kernels (msplit_gmres.hip) on a device-resident state, so a
 * whole restart cycle is enqueued without a host round trip; the host reads
 * the state back once per cycle.  Iterations past a convergence are enqueued
 * speculatively and return at once on the device's stop flag.
 *
 * Per Arnoldi step (VV = basis in HBM, sc = its scales on the device):
 *   SpMV      W = A (sc[it]*VV(it))                  (VecNormalize of the
 *             previous vector deferred: VV(it) stays as the MAXPY stored it and
 *             every reader multiplies by sc[it] = 1/||VV(it)||, which rounds each
 *             element exactly as VecScale would have stored it)
 *   MDot      h(0..it) = W . sc.VV(0..it)            (DBR order)
 *   MAXPY     VV(it+1) = W - sum h_j sc[j] VV(j), and ||VV(it+1)||^2   (one pass)
 *   update    the Hessenberg column, Givens rotation, tests, sc[it+1] (one lane)
 * W is PETSc's VEC_VV(it+1) before the orthogonalisation.
 *
 * Step kinds (step_kind, asked before every solve).  The four lines above are one arithmetic; which kernels run
 * them, and whether W ever reaches HBM, depends on the operator and the basis precision:
 *   opfuse   DV storage in the 8-code ELL layout (MSK_TUNE_GM_OPFUSE): MDot and MAXPY each compute their rows of
 *            W from the operator's codes; no MatMult kernel, no W vector.
 *   wfree    box stencils (the default there): the MatMult is fused with MDot and W is not stored; the MAXPY
 *            recomputes its rows from VV(it).
 *   stored W every other operator: W is its own n-vector (k->tmp, allocated by the first cycle that needs it),
 *            written by the MatMult (fused with MDot where the operator allows) and read by the MAXPY, which writes
 *            a different vector than it reads (an in-place MAXPY measured 5 % slower, same box).
 *   f32      MSP_BASIS_F32 (msp_ksp_set_basis_precision): the basis is stored as float and the step is always
 *            MatMult, MDot, MAXPY as three kernels (msplit_cgs_basis.hip) over two f64 n-vectors: W and the "current
 *            vector", the newest basis vector's rounded values as doubles, which is the MatMult's input -- so every
 *            operator's scaled MatMult serves unchanged.  VV(it+1) = rnd(W - sum ...) is rounded when stored and
 *            its norm is the rounded values' norm; everything else is the same f64 arithmetic.  Neither opfuse nor
 *            wfree is taken, and the MDot / MAXPY variant flags of MSPLIT_TUNING do not apply.
 *   block16  MSP_BASIS_B16: the f32 step with another stored format (the same kernels' B16): 16-bit integers with one
 *            power-of-two exponent per DBR chunk and vector, the rounding rule of include/msplit.h.  Same launches,
 *            same two f64 n-vectors, same arithmetic; the whole double exponent range is representable and a
 *            non-finite entry ends the solve.  Inside one restart cycle the recurrence residual can run ahead of
 *            the true one by about 2^-13 of the cycle's initial residual (the next restart recomputes it in f64):
 *            for inexact inner solves and fixed-iteration steps, not for gaining many digits in a single cycle.
 *   jacobi   MSP_PC_JACOBI (msp_ksp_set_pc_type): PETSc's left Jacobi with the preconditioned norm on the f64 basis.
 *            MatMult, MDot, MAXPY as three kernels (msplit_cgs_basis.hip); the MatMult stores the raw W and the two CGS
 *            kernels form dinv .* W in registers as they load it (8 more bytes per row each, no rewrite of W).  The
 *            cycle's first kernel multiplies the initial residual by dinv in place; ||dinv .* b|| serves the
 *            convergence test's rnorm0.  Neither opfuse nor wfree is taken; the recurrence is unchanged.
 *   oper f32 MSP_OPER_F32 (msp_ksp_set_operator_precision), an operator whose products read its CSR arrays: the
 *            Arnoldi MatMult of a stored-W step (the f64, f32, block16 or jacobi one) reads a copy of the operator
 *            whose values are floats packed with their columns, 8 bytes per entry for 12 (msplit_csr32.hip,
 *            mspi_spmv_scaled_p32), and sums every row in f64 in the same order: the f64 MatMult on the matrix
 *            (double)(float)a, bit for bit.  Always MatMult, MDot, MAXPY as three kernels: neither opfuse nor wfree,
 *            nor the fused MatMult + MDot.  KSPInitialResidual at every restart, MatMult outside the step, the
 *            diagonal and Jacobi's dinv read the f64 values: the solve is GMRES on the rounded operator with an f64
 *            residual correction at each restart.  Inside one cycle the recurrence residual is the rounded
 *            operator's and can differ from the true one by about 2^-24 || |A| |dx| ||; from a zero guess within
 *            one cycle, x solves the rounded system.
 *   refined  MSP_CGS_REFINE_IFNEEDED / _ALWAYS (msp_ksp_set_cgs_refinement) on the f64 basis without Jacobi: a
 *            stored-W step of five launches, the same on every step so that a captured cycle replays it: MatMult
 *            (fused with MDot where the operator allows; the packed copy's under MSP_OPER_F32), pass 1 fused with
 *            pass 2's MDot stage 1 (k_maxpy_mdot: u = W - sum h_j v_j stored to VV(it+1), the partials of ||u||^2 and
 *            of every c_j = u . v_j, one sweep), the decide kernel (folds them; refine and skip), pass 2's MAXPY in
 *            place on VV(it+1) (k_maxpy_chunk, returning at once on skip), the update kernel (column h + c, tt from
 *            ss2 or ss1, then k_norm_update's statements).  Steps with it + 2 > MSPI_MAX_GROUP take
 *            mspi_maxpy_norm_basis then mspi_mdot_basis instead of the fused pass: the same bits.  Neither opfuse
 *            nor wfree (a W-free refined step is not built).
 *
 * Data layout: VV(0..min(m, max_it)) are one allocation of (min(m, max_it)+1) x stride elements; stride = n rounded
 * up to 512 doubles, to 1024 floats or to 2048 int16 (4 KiB each way); block16 keeps its int32 exponents,
 * [vector][chunk], behind the last vector in the same allocation.  W and the current vector are separate allocations.
 * KSPInitialResidual writes VV(0) (f32: the current vector, which the cycle's first kernel rounds into VV(0)).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "msplit.h"
#include "msplit_internal.h"
#include "ksp_impl.h"

int msp_ksp_get_default_opts(msp_ksp_opts *o) {
  if (!o) {
    mspi_set_error(MSP_ERR_ARG_NULL, "opts is NULL");
    return MSP_ERR_ARG_NULL;
  }
  o->restart = 30;
  o->max_it = 10000;
  o->rtol = 1e-5;
  o->abstol = 1e-50;
  o->divtol = 1e4;
  o->haptol = 1e-30;
  o->breakdowntol = 0.1;
  o->uirnorm = 0;
  o->guess_nonzero = 0;
  return MSP_SUCCESS;
}

int msp_ksp_create(msp_ctx *ctx, msp_ksp **out) {
  if (!ctx || !out) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  msp_ksp *k = (msp_ksp *)calloc(1, sizeof(msp_ksp));
  if (!k) {
    mspi_set_error(MSP_ERR_MEM, "KSP allocation failed");
    return MSP_ERR_MEM;
  }
  k->ctx = ctx;
  mspi_ctx_retain(ctx);
  msp_ksp_get_default_opts(&k->o);
  k->cg_route_set = MSPI_CG_ROUTE_AUTO;
  *out = k;
  return MSP_SUCCESS;
}

void ksp_drop_graphs(msp_ksp *k) {
  for (int i = 0; i < KSP_NGRAPH; ++i) {
    mspi_graph_destroy(k->graphs[i].exec);
    memset(&k->graphs[i], 0, sizeof(k->graphs[i]));
  }
  k->gnext = 0;
}

void ksp_free_work(msp_ksp *k) {
  ksp_drop_graphs(k);
  if (k->basis) mspi_free(k->ctx, k->basis);
  if (k->tmp) mspi_free(k->ctx, k->tmp);
  if (k->cur) mspi_free(k->ctx, k->cur);
  if (k->dinv) mspi_free(k->ctx, k->dinv);
  if (k->gblock) mspi_free(k->ctx, k->gblock);
  if (k->hst) mspi_host_free(k->hst);
  if (k->cg_r) mspi_free(k->ctx, k->cg_r);
  if (k->cg_w) mspi_free(k->ctx, k->cg_w);
  if (k->cg_p) mspi_free(k->ctx, k->cg_p);
  if (k->cg_p2) mspi_free(k->ctx, k->cg_p2);
  if (k->cg_hst) mspi_host_free(k->cg_hst);
  k->cg_r = k->cg_w = k->cg_p = k->cg_p2 = k->cg_hist = NULL;
  k->cg_st = k->cg_hst = NULL;
  free(k->hist);
  k->basis = k->tmp = k->cur = k->dinv = NULL;
  k->dinv_valid = 0;
  k->expo = NULL;
  k->basis_bytes = k->gblock_bytes = k->vec_bytes = 0;
  k->gblock = NULL;
  k->rf = NULL;
  k->hst = NULL;
  k->hist = NULL;
  memset(&k->g, 0, sizeof(k->g));
  k->hist_cap = 0;
  k->setup = 0;
}

int msp_ksp_destroy(msp_ksp **pk) {
  if (!pk || !*pk) return MSP_SUCCESS;
  msp_ctx *c = (*pk)->ctx;
  msp_ctx_synchronize(c);
  ksp_free_work(*pk);
  free(*pk);
  *pk = NULL;
  mspi_ctx_release(c);
  return MSP_SUCCESS;
}

int msp_ksp_set_operators(msp_ksp *k, msp_mat *A) {
  if (!k || !A) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  int32_t nr, nc;
  mspi_mat_dims(A, &nr, &nc);
  if (nr != nc) {
    mspi_set_error(MSP_ERR_ARG_SIZ, "KSP operator must be square, got %d x %d", nr, nc);
    return MSP_ERR_ARG_SIZ;
  }
  if (mspi_mat_ctx(A) != k->ctx) {
    mspi_set_error(MSP_ERR_ARG_WRONG, "operator belongs to another context");
    return MSP_ERR_ARG_WRONG;
  }
  if (k->A && k->n != nr) ksp_free_work(k);
  ksp_drop_graphs(k); /* even for the same handle: a new matrix can reuse a destroyed one's address */
  k->A = A;
  k->n = nr;
  k->dinv_valid = 0; /* PCSetUp again: the next set-up or solve recomputes the diagonal's inverse */
  return MSP_SUCCESS;
}

int msp_ksp_set_opts(msp_ksp *k, const msp_ksp_opts *o) {
  if (!k || !o) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  if (o->restart < 1 || o->max_it < 0 || o->rtol < 0 || o->abstol < 0 || o->divtol < 0) {
    mspi_set_error(MSP_ERR_ARG_OUTOFRANGE, "invalid KSP options (restart %d, max_it %d)", o->restart, o->max_it);
    return MSP_ERR_ARG_OUTOFRANGE;
  }
  if (k->setup && (o->restart != k->o.restart || o->max_it + 2 > k->hist_cap)) ksp_free_work(k);
  k->o = *o;
  return MSP_SUCCESS;
}

int msp_ksp_get_opts(const msp_ksp *k, msp_ksp_opts *o) {
  if (!k || !o) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  *o = k->o;
  return MSP_SUCCESS;
}

int msp_ksp_set_basis_precision(msp_ksp *k, int prec) {
  if (!k) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  if (prec != MSP_BASIS_F64 && prec != MSP_BASIS_F32 && prec != MSP_BASIS_B16) {
    mspi_set_error(MSP_ERR_ARG_OUTOFRANGE,
                   "basis precision %d is none of MSP_BASIS_F64, MSP_BASIS_F32, MSP_BASIS_B16", prec);
    return MSP_ERR_ARG_OUTOFRANGE;
  }
  if (prec != k->basis_prec && k->setup) { /* another element type: new work vectors, no graph survives */
    msp_ctx_synchronize(k->ctx);
    ksp_free_work(k);
  }
  k->basis_prec = prec;
  return MSP_SUCCESS;
}

int msp_ksp_get_basis_precision(const msp_ksp *k, int *prec) {
  if (!k || !prec) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  *prec = k->basis_prec;
  return MSP_SUCCESS;
}

int msp_ksp_set_pc_type(msp_ksp *k, int pc_type) {
  if (!k) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  if (pc_type != MSP_PC_NONE && pc_type != MSP_PC_JACOBI) {
    mspi_set_error(MSP_ERR_ARG_OUTOFRANGE, "preconditioner %d is neither MSP_PC_NONE nor MSP_PC_JACOBI", pc_type);
    return MSP_ERR_ARG_OUTOFRANGE;
  }
  if (pc_type != k->pc_type && k->setup) { /* another step and other work vectors: no graph survives */
    msp_ctx_synchronize(k->ctx);
    ksp_free_work(k);
  }
  k->pc_type = pc_type;
  return MSP_SUCCESS;
}

int msp_ksp_get_pc_type(const msp_ksp *k, int *pc_type) {
  if (!k || !pc_type) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  *pc_type = k->pc_type;
  return MSP_SUCCESS;
}

int msp_ksp_set_type(msp_ksp *k, int type) {
  if (!k) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  if (type != MSP_KSP_GMRES && type != MSP_KSP_CG) {
    mspi_set_error(MSP_ERR_ARG_OUTOFRANGE, "KSP type %d is neither MSP_KSP_GMRES nor MSP_KSP_CG", type);
    return MSP_ERR_ARG_OUTOFRANGE;
  }
  if (type != k->type) { /* other work vectors and another state block: no graph survives */
    msp_ctx_synchronize(k->ctx);
    ksp_free_work(k);
  }
  k->type = type;
  return MSP_SUCCESS;
}

int msp_ksp_get_type(const msp_ksp *k, int *type) {
  if (!k || !type) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  *type = k->type;
  return MSP_SUCCESS;
}

int msp_ksp_set_norm_type(msp_ksp *k, int norm) {
  if (!k) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  if (norm != MSP_NORM_PRECONDITIONED && norm != MSP_NORM_UNPRECONDITIONED) {
    mspi_set_error(MSP_ERR_ARG_OUTOFRANGE,
                   "norm type %d is neither MSP_NORM_PRECONDITIONED nor MSP_NORM_UNPRECONDITIONED", norm);
    return MSP_ERR_ARG_OUTOFRANGE;
  }
  if (norm != k->norm_type) { /* another kernel in every captured CG cycle; the work vectors stay */
    msp_ctx_synchronize(k->ctx);
    ksp_drop_graphs(k);
  }
  k->norm_type = norm;
  return MSP_SUCCESS;
}

int msp_ksp_get_norm_type(const msp_ksp *k, int *norm) {
  if (!k || !norm) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  *norm = k->norm_type;
  return MSP_SUCCESS;
}

int msp_ksp_set_operator_precision(msp_ksp *k, int prec) {
  if (!k) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  if (prec != MSP_OPER_F64 && prec != MSP_OPER_F32) {
    mspi_set_error(MSP_ERR_ARG_OUTOFRANGE, "operator precision %d is neither MSP_OPER_F64 nor MSP_OPER_F32", prec);
    return MSP_ERR_ARG_OUTOFRANGE;
  }
  if (prec != k->oper_prec) { /* another MatMult kernel in every captured cycle; the work vectors stay */
    msp_ctx_synchronize(k->ctx);
    ksp_drop_graphs(k);
  }
  k->oper_prec = prec;
  return MSP_SUCCESS;
}

int msp_ksp_get_operator_precision(const msp_ksp *k, int *prec) {
  if (!k || !prec) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  *prec = k->oper_prec;
  return MSP_SUCCESS;
}

int msp_ksp_set_cgs_refinement(msp_ksp *k, int type) {
  if (!k) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  if (type != MSP_CGS_REFINE_NEVER && type != MSP_CGS_REFINE_IFNEEDED && type != MSP_CGS_REFINE_ALWAYS) {
    mspi_set_error(MSP_ERR_ARG_OUTOFRANGE,
                   "CGS refinement %d is none of MSP_CGS_REFINE_NEVER, MSP_CGS_REFINE_IFNEEDED, MSP_CGS_REFINE_ALWAYS",
                   type);
    return MSP_ERR_ARG_OUTOFRANGE;
  }
  if (type != k->cgs) { /* other launches in every captured cycle; the work vectors stay */
    msp_ctx_synchronize(k->ctx);
    ksp_drop_graphs(k);
  }
  k->cgs = type;
  return MSP_SUCCESS;
}

int msp_ksp_get_cgs_refinement(const msp_ksp *k, int *type) {
  if (!k || !type) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  *type = k->cgs;
  return MSP_SUCCESS;
}

int msp_ksp_get_cgs_refinement_count(const msp_ksp *k, int32_t *n) {
  if (!k || !n) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  *n = k->nrefine;
  return MSP_SUCCESS;
}

int msp_ksp_get_work_bytes(const msp_ksp *k, int64_t *bytes) {
  if (!k || !bytes) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  *bytes = (int64_t)(k->basis_bytes + k->gblock_bytes + (k->tmp ? k->vec_bytes : 0) + (k->cur ? k->vec_bytes : 0) +
                    (k->cg_r ? 3 * k->vec_bytes : 0) + (k->cg_p2 ? k->vec_bytes : 0) +
                    (k->dinv ? (size_t)k->n * sizeof(double) : 0));
  return MSP_SUCCESS;
}

/* PCSetUp of MSP_PC_JACOBI: dinv allocated with the work, computed once per operator */
int ksp_pc_set_up(msp_ksp *k) {
  if (k->pc_type != MSP_PC_JACOBI || k->dinv_valid) return MSP_SUCCESS;
  int rc = MSP_SUCCESS;
  if (!k->dinv) rc = mspi_malloc(k->ctx, (void **)&k->dinv, (size_t)(k->n ? k->n : 1) * sizeof(double));
  if (!rc) rc = mspi_pcj_diag_inv(k->A, k->dinv);
  if (!rc) k->dinv_valid = 1;
  return rc;
}

int msp_ksp_set_up(msp_ksp *k) {
  if (!k || !k->A) {
    mspi_set_error(MSP_ERR_ARG_WRONG, "KSPSetUp before KSPSetOperators");
    return MSP_ERR_ARG_WRONG;
  }
  if (k->type == MSP_KSP_CG) return ksp_cg_set_up(k);
  if (k->setup) return ksp_pc_set_up(k);
  const int64_t m = k->o.restart;
  /* a cycle runs K <= min(restart, max_it) steps and touches VV(0..K): with max_it < restart (the campaign's
   * inner solves, max_it 20 under GMRES(30)) only max_it + 1 basis vectors are ever used -- 11 of 32 GB less
   * per configs[3] block.  A larger max_it frees the work (hist_cap, msp_ksp_set_opts). */
  const int64_t mv = (k->o.max_it < m ? k->o.max_it : m) + 1;
  int64_t skew = 0; /* an extra skew between basis vectors measured no gain (profiles/r01/skew_ab) */
  const char *env = getenv("MSPLIT_BASIS_SKEW");
  const int f32 = k->basis_prec == MSP_BASIS_F32, b16 = k->basis_prec == MSP_BASIS_B16;
  const int64_t align = b16 ? 2048 : f32 ? 1024 : 512; /* elements in 4 KiB */
  if (env) skew = (atoll(env) + align - 1) / align * align;
  k->stride = (k->n + align - 1) / align * align + skew;
  k->hist_cap = k->o.max_it + 2;
  /* one device block for the recurrence: state, then hh, cc, ss, grs, h, sc, hist */
  const size_t nd = (size_t)((m + 2) * (m + 1) + 5 * (m + 2) + k->hist_cap);
  const size_t st_bytes = (sizeof(mspi_gmres_state) + 63) / 64 * 64;
  const size_t elem = b16 ? sizeof(int16_t) : f32 ? sizeof(float) : sizeof(double);
  const size_t vv_bytes = (size_t)mv * (size_t)k->stride * elem;
  k->nchunks = (k->n + MSPI_DBR_CHUNK - 1) / MSPI_DBR_CHUNK;
  k->basis_bytes = vv_bytes + (b16 ? (size_t)mv * (size_t)k->nchunks * sizeof(int32_t) : 0) + 4096;
  /* the CGS refinement's block (mode, refine, skip, count, ss1, ss2, c(0..m+1)) behind the arrays */
  k->gblock_bytes = st_bytes + nd * sizeof(double) + MSPI_REFINE_BYTES(m);
  k->vec_bytes = (size_t)((k->n + 511) / 512 * 512) * sizeof(double) + 4096;
  int rc = mspi_malloc(k->ctx, (void **)&k->basis, k->basis_bytes);
  /* W (k->tmp) is allocated by the first cycle that stores it (ensure_w): the W-free step never does */
  if (!rc) rc = mspi_malloc(k->ctx, &k->gblock, k->gblock_bytes);
  if (!rc) rc = mspi_host_malloc((void **)&k->hst, sizeof(mspi_gmres_state));
  k->hist = (double *)calloc((size_t)k->hist_cap, sizeof(double));
  if (!rc && !k->hist) {
    mspi_set_error(MSP_ERR_MEM, "host allocation failed");
    rc = MSP_ERR_MEM;
  }
  if (rc) {
    ksp_free_work(k);
    return rc;
  }
  k->expo = b16 ? (int32_t *)((char *)k->basis + vv_bytes) : NULL;
  double *d = (double *)((char *)k->gblock + st_bytes);
  k->g.st = (mspi_gmres_state *)k->gblock;
  k->g.hh = d;
  d += (m + 2) * (m + 1);
  k->g.cc = d;
  d += m + 2;
  k->g.ss = d;
  d += m + 2;
  k->g.grs = d;
  d += m + 2;
  k->g.h = d;
  d += m + 2;
  k->g.sc = d;
  d += m + 2;
  k->g.hist = d;
  k->rf = (mspi_gmres_refine *)(d + k->hist_cap);
  k->setup = 1;
  if ((rc = ksp_pc_set_up(k))) ksp_free_work(k);
  return rc;
}

static double *VV(const msp_ksp *k, int j) { return k->basis + (int64_t)j * k->stride; }
static float *VF(const msp_ksp *k, int j) { return (float *)k->basis + (int64_t)j * k->stride; } /* MSP_BASIS_F32 */
static int16_t *VH(const msp_ksp *k, int j) { return (int16_t *)k->basis + (int64_t)j * k->stride; } /* MSP_BASIS_B16 */
static int32_t *EX(const msp_ksp *k, int j) { return k->expo + (int64_t)j * k->nchunks; }
static int compressed(const msp_ksp *k) { return k->basis_prec != MSP_BASIS_F64; }

/* Which Arnoldi step a cycle runs: the operator computed inside MDot and MAXPY (opfuse), the W-free step on a box
 * stencil (wfree), or W stored between the MatMult and the CGS kernels (neither).  The W-free choice follows the
 * operator and msk_set_gm_wfree, so it is asked again before every solve. */
static void step_kind(const msp_ksp *k, int *opfuse, int *wfree) {
  if (k->oper_prec == MSP_OPER_F32) { /* the packed copy has a MatMult only: a stored-W step */
    *opfuse = *wfree = 0;
    return;
  }
  if (compressed(k)) { /* those kernels read an f64 basis: the f32 / block16 step stores W */
    *opfuse = *wfree = 0;
    return;
  }
  if (k->pc_type == MSP_PC_JACOBI) { /* w = dinv .* W is formed by the CGS kernels from the stored W */
    *opfuse = *wfree = 0;
    return;
  }
  if (k->cgs != MSP_CGS_REFINE_NEVER) { /* the refined step reads a stored W; a W-free one is not built */
    *opfuse = *wfree = 0;
    return;
  }
  *opfuse = mspi_op_fusable(k->A) && k->o.restart + 1 <= MSPI_MAX_GROUP;
  *wfree = !*opfuse && k->o.restart <= MSPI_MAX_GROUP && mspi_gm_wfree(k->A);
}

/* The stored-W step's n-vector, allocated the first time a cycle takes that step (before any graph capture: no
 * allocation inside a captured cycle) -- 134-537 MB per block that the default W-free step never touches. */
static int ensure_w(msp_ksp *k) {
  int opfuse, wfree;
  step_kind(k, &opfuse, &wfree);
  if (opfuse || wfree) return MSP_SUCCESS;
  int rc = MSP_SUCCESS;
  if (!k->tmp) rc = mspi_malloc(k->ctx, (void **)&k->tmp, k->vec_bytes);
  /* the f32 step's second f64 n-vector: the MatMult's input */
  if (!rc && compressed(k) && !k->cur) rc = mspi_malloc(k->ctx, (void **)&k->cur, k->vec_bytes);
  return rc;
}

/* The Arnoldi MatMult of a stored-W step, W = A (sc x): under MSP_OPER_F32 from the packed copy of the operator */
static int step_matmult(msp_ksp *k, const double *x, const double *sc, const int *stop) {
  if (k->oper_prec == MSP_OPER_F32) return mspi_spmv_scaled_p32(k->A, x, sc, k->tmp, stop);
  return mspi_spmv_scaled(k->A, x, sc, NULL, k->tmp, stop);
}

/* One KSPGMRESCycle from its initial residual in VV(0): VecNormalize (deferred),
 * up to K Arnoldi steps, BuildSoln(it-1) into x.  Enqueued, no host synchronisation. */
static int enqueue_cycle(msp_ksp *k, double *x, int K) {
  msp_ctx *c = k->ctx;
  const int *stop = &k->g.st->stop;
  const double *sc = k->g.sc;
  double *sumsq = &k->g.h[0];
  const int f32 = k->basis_prec == MSP_BASIS_F32, b16 = k->basis_prec == MSP_BASIS_B16;
  if (k->pc_type == MSP_PC_JACOBI) {
    /* left Jacobi on the f64 basis: VV(0) = dinv .* r in place and its norm; per step the raw W = A (sc[it] VV(it))
     * is stored, h = (dinv .* W) . sc.VV(0..it), VV(it+1) = dinv .* W - sum h_j sc[j] VV(j) and its norm -- both
     * kernels form dinv .* W as they load W.  The recurrence and BuildSoln are the unpreconditioned ones. */
    int rc = mspi_pcj_apply_norm(c, VV(k, 0), k->dinv, VV(k, 0), k->n, sumsq, NULL);
    if (!rc) rc = mspi_gm_cycle_start(c, k->g, sumsq);
    for (int it = 0; it < K && !rc; ++it) {
      rc = step_matmult(k, VV(k, it), sc + it, stop);
      if (!rc) rc = mspi_pcj_mdot(c, k->tmp, k->dinv, it + 1, k->basis, k->stride, sc, k->n, k->g.h, stop);
      if (!rc)
        rc = mspi_pcj_maxpy_norm_update(c, k->tmp, k->dinv, VV(k, it + 1), it + 1, k->basis, k->stride, sc, k->n,
                                        k->g, k->o.restart, stop);
    }
    if (!rc) rc = mspi_gm_build(c, k->g, (int)k->o.restart);
    if (!rc) rc = mspi_maxpy_accum_basis(c, x, &k->g.st->nbuild, k->basis, k->stride, sc, k->n, k->g.grs, K);
    return rc;
  }
  /* f32 / block16: the initial residual waits in the current vector; VV(0) = rnd(r), the vector's norm is the
   * rounded one's */
  int rc = f32   ? mspi_cb_round_store(c, k->cur, k->cur, VF(k, 0), k->n, sumsq, NULL)
           : b16 ? mspi_cb16_round_store(c, k->cur, k->cur, VH(k, 0), EX(k, 0), k->n, sumsq, NULL)
                 : mspi_norm2sq(c, VV(k, 0), k->n, sumsq);
  if (!rc) rc = mspi_gm_cycle_start(c, k->g, sumsq);
  int opfuse, wfree;
  step_kind(k, &opfuse, &wfree);
  for (int it = 0; it < K && !rc && f32; ++it) {
    /* W = A (sc[it] s_it) from the current vector (s_it as doubles), h = W . sc.VV(0..it) over the float basis,
     * then s_{it+1} = rnd(W - sum h_j sc[j] VV(j)) to VV(it+1) and back into the current vector, ||s_{it+1}||^2 */
    rc = step_matmult(k, k->cur, sc + it, stop);
    if (!rc) rc = mspi_cb_mdot(c, k->tmp, it + 1, VF(k, 0), k->stride, sc, k->n, k->g.h, stop);
    if (!rc)
      rc = mspi_cb_maxpy_norm_update(c, k->tmp, k->cur, VF(k, it + 1), it + 1, VF(k, 0), k->stride, sc, k->n, k->g,
                                     k->o.restart, stop);
  }
  if (f32) {
    if (!rc) rc = mspi_gm_build(c, k->g, (int)k->o.restart);
    if (!rc) rc = mspi_cb_accum(c, x, &k->g.st->nbuild, VF(k, 0), k->stride, sc, k->n, k->g.grs, K);
    return rc;
  }
  for (int it = 0; it < K && !rc && b16; ++it) { /* the f32 step, the basis read and written as block16 */
    rc = step_matmult(k, k->cur, sc + it, stop);
    if (!rc) rc = mspi_cb16_mdot(c, k->tmp, it + 1, VH(k, 0), k->stride, EX(k, 0), sc, k->n, k->g.h, stop);
    if (!rc)
      rc = mspi_cb16_maxpy_norm_update(c, k->tmp, k->cur, VH(k, it + 1), EX(k, it + 1), it + 1, VH(k, 0), k->stride,
                                       EX(k, 0), sc, k->n, k->g, k->o.restart, stop);
  }
  if (b16) {
    if (!rc) rc = mspi_gm_build(c, k->g, (int)k->o.restart);
    if (!rc)
      rc = mspi_cb16_accum(c, x, &k->g.st->nbuild, VH(k, 0), k->stride, EX(k, 0), sc, k->n, k->g.grs, K);
    return rc;
  }
  for (int it = 0; it < K && !rc && opfuse; ++it) {
    /* W = A (sc[it] VV(it)) never reaches HBM: MDot and MAXPY each compute their rows of it from the operator's
     * one-byte codes and VV(it) (which both stream anyway), bitwise the separate MatMult's W */
    rc = mspi_mdot_op(k->A, VV(k, it), sc + it, it + 1, k->basis, k->stride, sc, k->g.h, stop);
    if (!rc)
      rc = mspi_maxpy_norm_update_op(k->A, VV(k, it), sc + it, VV(k, it + 1), it + 1, k->basis, k->stride, sc, k->g,
                                     k->o.restart, stop);
  }
  /* box stencils: W is not stored; the MAXPY recomputes its rows from VV(it) (which it streams anyway) */
  for (int it = 0; it < K && !rc && wfree; ++it) {
    rc = mspi_spmv_mdot(k->A, VV(k, it), sc + it, NULL, it + 1, k->basis, k->stride, sc, k->g.h, stop);
    if (!rc)
      rc = mspi_maxpy_norm_update_march(k->A, VV(k, it), sc + it, VV(k, it + 1), it + 1, k->basis, k->stride, sc,
                                        k->g, k->o.restart, stop);
  }
  for (int it = 0; it < K && !rc && k->cgs != MSP_CGS_REFINE_NEVER; ++it) {
    /* the refined step: MatMult (+ MDot), pass 1 (+ pass 2's MDot), decide, pass 2's MAXPY, update -- the same five
     * launches whatever the device decides (a step that does not refine returns from the fourth on rf->skip) */
    const int nv = it + 1;
    rc = k->oper_prec == MSP_OPER_F32 ? MSP_ERR_SUP /* the fused kernel reads the f64 values */
                                      : mspi_spmv_mdot(k->A, VV(k, it), sc + it, k->tmp, nv, k->basis, k->stride, sc,
                                                       k->g.h, stop);
    if (rc == MSP_ERR_SUP) {
      rc = step_matmult(k, VV(k, it), sc + it, stop);
      if (!rc) rc = mspi_mdot_basis(c, k->tmp, nv, k->basis, k->stride, sc, k->n, k->g.h, stop);
    }
    if (!rc && mspi_gm_refine_fused(nv)) {
      rc = mspi_maxpy_norm_mdot_basis(c, k->tmp, VV(k, it + 1), nv, k->basis, k->stride, sc, k->n, k->g.h, NULL, NULL,
                                      stop);
      if (!rc) rc = mspi_gm_refine_decide(c, k->g, k->rf, mspi_ctx_partial(c), k->nchunks);
    } else if (!rc) { /* more rows than the partial buffer holds: the two kernels the fused one restates */
      rc = mspi_maxpy_norm_basis(c, k->tmp, VV(k, it + 1), nv, k->basis, k->stride, sc, k->n, k->g.h, &k->rf->ss1,
                                 stop);
      if (!rc)
        rc = mspi_mdot_basis(c, VV(k, it + 1), nv, k->basis, k->stride, sc, k->n, MSPI_REFINE_C(k->rf), stop);
      if (!rc) rc = mspi_gm_refine_decide(c, k->g, k->rf, NULL, k->nchunks);
    }
    if (!rc) rc = mspi_gm_refine_maxpy2(c, VV(k, it + 1), nv, k->basis, k->stride, sc, k->n, k->rf);
    if (!rc) rc = mspi_gm_refine_update(c, k->g, k->rf, mspi_ctx_partial(c), k->nchunks, (int)k->o.restart);
  }
  for (int it = 0; it < K && !rc && !opfuse && !wfree && k->cgs == MSP_CGS_REFINE_NEVER; ++it) {
    /* W = A (sc[it] VV(it))  (KSP_PCApplyBAorAB with PCNONE on the normalised VV(it)),
     * CGS: h = VecMDot(W, VV(0..it)) -- one fused launch where the operator allows */
    rc = k->oper_prec == MSP_OPER_F32 ? MSP_ERR_SUP /* the fused kernel reads the f64 values */
                                      : mspi_spmv_mdot(k->A, VV(k, it), sc + it, k->tmp, it + 1, k->basis, k->stride,
                                                       sc, k->g.h, stop);
    if (rc == MSP_ERR_SUP) {
      rc = step_matmult(k, VV(k, it), sc + it, stop);
      if (!rc) rc = mspi_mdot_basis(c, k->tmp, it + 1, k->basis, k->stride, sc, k->n, k->g.h, stop);
    }
    /* then VV(it+1) = W - sum h_j VV(j); ||VV(it+1)||^2 */
    /* then h(it+1) = ||VV(it+1)||^2, sc[it+1] and the Hessenberg column update */
    if (!rc)
      rc = mspi_maxpy_norm_update(c, k->tmp, VV(k, it + 1), it + 1, k->basis, k->stride, sc, k->n, k->g, it,
                                  k->o.restart, stop);
  }
  /* KSPGMRESBuildSoln: back-solve (one lane, H staged in LDS), then x += sum nrs_j VV(j) */
  if (!rc) rc = mspi_gm_build(c, k->g, (int)k->o.restart);
  if (!rc) rc = mspi_maxpy_accum_basis(c, x, &k->g.st->nbuild, k->basis, k->stride, sc, k->n, k->g.grs, K);
  return rc;
}

/* A cycle from the graph cache: captured the first time its key is seen, then
 * replayed with one hipGraphLaunch (the host enqueues ~5 launches per Arnoldi
 * step otherwise, which small systems feel).  Same kernels, same arguments,
 * same order: results are those of the eager enqueue. */
int ksp_run_cycle(msp_ksp *k, double *x, int K, int (*enqueue_cycle)(msp_ksp *, double *, int)) {
  msp_ctx *c = k->ctx;
  if (k->graphs_off || !mspi_graphs_enabled(c)) return enqueue_cycle(k, x, K);
  int rc = mspi_reserve_partial(c, k->n); /* before the lookup: it may reallocate (a new epoch) */
  if (rc) return rc;
  const uint64_t aver = mspi_mat_version(k->A), epoch = mspi_ctx_epoch(c);
  /* the basis precision is not in the key: changing it frees the work, and with it every captured cycle; changing
   * the operator precision drops the captured cycles */
  const int tuning = msk_get_tuning(), shape = msk_get_shape_epoch();
  for (int i = 0; i < KSP_NGRAPH; ++i) {
    const ksp_graph *g = &k->graphs[i];
    if (g->exec && g->A == k->A && g->aver == aver && g->epoch == epoch && g->x == x && g->K == K &&
        g->tuning == tuning && g->shape == shape && g->type == k->type)
      return mspi_graph_launch(c, g->exec);
  }
  if (mspi_capture_begin(c)) { /* stream cannot be captured: run it eagerly */
    k->graphs_off = 1;
    return enqueue_cycle(k, x, K);
  }
  rc = enqueue_cycle(k, x, K);
  void *exec = NULL;
  const int rc2 = mspi_capture_end(c, rc == 0, &exec);
  if (rc) return rc;
  if (rc2 || !exec) { /* nothing ran: the capture only recorded the cycle */
    k->graphs_off = 1;
    return enqueue_cycle(k, x, K);
  }
  ksp_graph *g = &k->graphs[k->gnext];
  k->gnext = (k->gnext + 1) % KSP_NGRAPH;
  mspi_graph_destroy(g->exec);
  g->exec = exec;
  g->A = k->A;
  g->aver = aver;
  g->epoch = epoch;
  g->x = x;
  g->K = K;
  g->tuning = tuning;
  g->shape = shape;
  g->type = k->type;
  return mspi_graph_launch(c, exec);
}

int msp_ksp_solve(msp_ksp *k, const msp_vec *b, msp_vec *x) {
  if (!k || !b || !x) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  if (!k->A) {
    mspi_set_error(MSP_ERR_ARG_WRONG, "KSPSolve before KSPSetOperators");
    return MSP_ERR_ARG_WRONG;
  }
  if (b->n != k->n || x->n != k->n) {
    mspi_set_error(MSP_ERR_ARG_SIZ, "KSPSolve sizes: operator %lld, b %lld, x %lld", (long long)k->n,
                   (long long)b->n, (long long)x->n);
    return MSP_ERR_ARG_SIZ;
  }
  if (b->d == x->d) {
    mspi_set_error(MSP_ERR_ARG_WRONG, "b and x must be different vectors");
    return MSP_ERR_ARG_WRONG;
  }
  if (k->type == MSP_KSP_CG) return ksp_cg_solve(k, b, x);
  if (compressed(k) && mspi_reduce_seq(k->ctx)) {
    mspi_set_error(MSP_ERR_SUP, "%s needs the DBR reduction: MSP_REDUCE_SEQ reproduces PETSc's f64 "
                                "sums bit for bit, which a rounded basis cannot",
                   k->basis_prec == MSP_BASIS_B16 ? "MSP_BASIS_B16" : "MSP_BASIS_F32");
    return MSP_ERR_SUP;
  }
  if (k->pc_type == MSP_PC_JACOBI && compressed(k)) {
    mspi_set_error(MSP_ERR_SUP, "MSP_PC_JACOBI is built for the double basis only, not %s",
                   k->basis_prec == MSP_BASIS_B16 ? "MSP_BASIS_B16" : "MSP_BASIS_F32");
    return MSP_ERR_SUP;
  }
  if (k->pc_type == MSP_PC_JACOBI && mspi_reduce_seq(k->ctx)) {
    mspi_set_error(MSP_ERR_SUP, "MSP_PC_JACOBI needs the DBR reduction: its fused kernels have no MSP_REDUCE_SEQ form");
    return MSP_ERR_SUP;
  }
  if (k->oper_prec == MSP_OPER_F32 && mspi_reduce_seq(k->ctx)) {
    mspi_set_error(MSP_ERR_SUP, "MSP_OPER_F32 needs the DBR reduction: MSP_REDUCE_SEQ reproduces PETSc's f64 solve bit "
                                "for bit, which a rounded operator cannot");
    return MSP_ERR_SUP;
  }
  if (k->cgs != MSP_CGS_REFINE_NEVER) {
    const char *w = k->cgs == MSP_CGS_REFINE_ALWAYS ? "MSP_CGS_REFINE_ALWAYS" : "MSP_CGS_REFINE_IFNEEDED";
    if (compressed(k)) {
      mspi_set_error(MSP_ERR_SUP, "%s is built for the double basis only, not %s: the second pass runs before the "
                                  "store's rounding and cannot repair it",
                     w, k->basis_prec == MSP_BASIS_B16 ? "MSP_BASIS_B16" : "MSP_BASIS_F32");
      return MSP_ERR_SUP;
    }
    if (k->pc_type == MSP_PC_JACOBI) {
      mspi_set_error(MSP_ERR_SUP, "%s is not built with MSP_PC_JACOBI: its fused kernels have no second pass", w);
      return MSP_ERR_SUP;
    }
    if (mspi_reduce_seq(k->ctx)) {
      mspi_set_error(MSP_ERR_SUP, "%s needs the DBR reduction: its fused kernel has no MSP_REDUCE_SEQ form", w);
      return MSP_ERR_SUP;
    }
  }
  int rc = mspi_set_device(k->ctx);
  /* the packed copy, built or rebuilt before any capture; an operator whose products do not read its CSR arrays
   * and values beyond the float range are refused here, before any work is allocated */
  if (!rc && k->oper_prec == MSP_OPER_F32) rc = mspi_mat_ensure_p32(k->A);
  if (!rc) rc = msp_ksp_set_up(k);
  if (!rc) rc = ensure_w(k);
  if (rc) return rc;
  msp_ctx *c = k->ctx;
  const int guess_zero = !k->o.guess_nonzero;

  /* KSPSolve_GMRES state, initialised on the host and pushed once */
  mspi_gmres_state *h = k->hst;
  memset(h, 0, sizeof(*h));
  h->rnorm = -1.0; /* special marker for KSPGMRESCycle() */
  h->guess_zero = guess_zero;
  h->m = k->o.restart;
  h->max_it = k->o.max_it;
  h->uirnorm = k->o.uirnorm;
  h->hist_cap = k->hist_cap;
  h->rtol = k->o.rtol;
  h->abstol = k->o.abstol;
  h->divtol = k->o.divtol;
  h->haptol = k->o.haptol;
  h->breakdowntol = k->o.breakdowntol;
  h->scale = 1.0;
  if (!guess_zero && !k->o.uirnorm) { /* KSPConvergedDefault at n == 0 needs ||b|| */
    double bb = 0.0;
    /* under Jacobi ||dinv .* b||, the product written to W (free until the first MatMult) */
    if (k->pc_type == MSP_PC_JACOBI) rc = mspi_pcj_apply_norm(c, b->d, k->dinv, k->tmp, k->n, k->g.h, NULL);
    else rc = mspi_norm2sq(c, b->d, k->n, k->g.h);
    if (rc) return rc;
    if ((rc = mspi_d2h_sync(c, &bb, k->g.h, sizeof(double)))) return rc;
    h->bnorm = sqrt(bb);
  }
  if ((rc = mspi_h2d_async(c, k->g.st, h, sizeof(*h)))) return rc;
  k->nrefine = 0;
  if (k->cgs != MSP_CGS_REFINE_NEVER) { /* skip = 1 outside a step's decide..update window */
    const mspi_gmres_refine r0 = {k->cgs, 0, 1, 0, 0.0, 0.0};
    if ((rc = mspi_h2d_sync(c, k->rf, &r0, sizeof(r0)))) return rc;
    if ((rc = mspi_reserve_partial(c, k->n))) return rc; /* the cycle hands the buffer's address to its kernels */
  }
  if (guess_zero && (rc = mspi_set(c, x->d, k->n, 0.0))) return rc; /* KSPSolve zeroes x */

  int cycle_zero_guess = guess_zero, itcount = 0, its = 0, reason = 0;
  while (!reason) {
    /* KSPInitialResidual: VV(0) = b - A x (VecCopy + VecAXPY(-1)), or b for a zero guess */
    double *r0 = compressed(k) ? k->cur : VV(k, 0); /* f32 / block16: rounded into VV(0) by the cycle */
    if (!cycle_zero_guess) rc = mspi_residual(k->A, b->d, x->d, r0);
    else rc = mspi_copy(c, r0, b->d, k->n);
    if (rc) return rc;
    int K = k->o.max_it - its;
    if (K > k->o.restart) K = k->o.restart;
    if (K < 0) K = 0;
    if ((rc = ksp_run_cycle(k, x->d, K, enqueue_cycle))) return rc;
    if ((rc = mspi_d2h_sync(c, h, k->g.st, sizeof(*h)))) return rc; /* the one sync per cycle */
    its = h->its;
    reason = h->reason;
    itcount += h->it;
    if (itcount >= k->o.max_it) {
      if (!reason) reason = MSP_DIVERGED_ITS;
      break;
    }
    cycle_zero_guess = 0;
  }
  k->its = its;
  k->reason = reason;
  k->rnorm = h->rnorm;
  k->nhist = h->nhist < k->hist_cap ? h->nhist : k->hist_cap;
  if (k->nhist && (rc = mspi_d2h_sync(c, k->hist, k->g.hist, (size_t)k->nhist * sizeof(double)))) return rc;
  if (k->cgs != MSP_CGS_REFINE_NEVER) {
    mspi_gmres_refine r1;
    if ((rc = mspi_d2h_sync(c, &r1, k->rf, sizeof(r1)))) return rc;
    k->nrefine = r1.count;
  }
  return MSP_SUCCESS;
}

int msp_ksp_get_iteration_number(const msp_ksp *k, int32_t *its) {
  if (!k || !its) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  *its = k->its;
  return MSP_SUCCESS;
}

int msp_ksp_get_residual_norm(const msp_ksp *k, double *rnorm) {
  if (!k || !rnorm) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  *rnorm = k->rnorm;
  return MSP_SUCCESS;
}

int msp_ksp_get_converged_reason(const msp_ksp *k, int32_t *reason) {
  if (!k || !reason) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  *reason = k->reason;
  return MSP_SUCCESS;
}

int msp_ksp_get_residual_history(const msp_ksp *k, const double **hist, int32_t *n) {
  if (!k || !hist || !n) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  *hist = k->hist;
  *n = k->nhist;
  return MSP_SUCCESS;
}

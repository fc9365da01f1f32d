/*
 * ksp_cg.c -- KSPCG (MSP_KSP_CG) host logic over device-resident vectors.
 *
 * Restates PETSc 3.22.1's KSPSolve_CG (KSP_CG_SYMMETRIC, left PCNONE or PCJACOBI, the preconditioned or the
 * unpreconditioned norm taken every iteration) with KSPConvergedDefault; tests/cg_twin.py is the same statements
 * in numpy and the definition the device is held to.  PETSc itself has not been run against either.
 *
 * Division of labour, as for GMRES: this file owns the solve (the refusals, the work vectors, the initial
 * residual, the order of the launches, the decision to enqueue another cycle); the scalar recurrence runs in
 * one-lane kernels on a device-resident mspi_cg_state (msplit_k_cg.hip), so a cycle of up to 32 iterations is
 * enqueued, or replayed as one captured graph, without a host round trip, and the host reads the state once per
 * cycle.  Iterations past the end of the solve return at once on the state's stop flag.
 *
 * The route of p, w = A p and p . w (MSPI_CG_ROUTE_*) is decided once per solve, from what the operator takes.
 *
 * Work: r, w, p (one n-vector each; a second p under the forced march route) and the state block with the residual history behind it; under Jacobi the
 * n doubles of dinv.  z = dinv .* r is never stored: every kernel that needs it forms it in registers.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "msplit.h"
#include "msplit_internal.h"
#include "ksp_impl.h"

#define CG_CYCLE 32 /* iterations enqueued between two host reads of the state */

int ksp_cg_set_up(msp_ksp *k) {
  if (k->setup) return ksp_pc_set_up(k);
  k->nchunks = (k->n + MSPI_DBR_CHUNK - 1) / MSPI_DBR_CHUNK;
  k->hist_cap = k->o.max_it + 2;
  const size_t st_bytes = (sizeof(mspi_cg_state) + 63) / 64 * 64;
  k->gblock_bytes = st_bytes + (size_t)k->hist_cap * sizeof(double);
  k->vec_bytes = (size_t)((k->n + 511) / 512 * 512) * sizeof(double) + 4096;
  int rc = mspi_malloc(k->ctx, &k->gblock, k->gblock_bytes);
  if (!rc) rc = mspi_malloc(k->ctx, (void **)&k->cg_r, k->vec_bytes);
  if (!rc) rc = mspi_malloc(k->ctx, (void **)&k->cg_w, k->vec_bytes);
  if (!rc) rc = mspi_malloc(k->ctx, (void **)&k->cg_p, k->vec_bytes);
  if (!rc) rc = mspi_host_malloc((void **)&k->cg_hst, sizeof(mspi_cg_state));
  k->hist = (double *)calloc((size_t)k->hist_cap, sizeof(double));
  if (!rc && !k->hist) {
    mspi_set_error(MSP_ERR_MEM, "host allocation failed");
    rc = MSP_ERR_MEM;
  }
  if (rc) {
    ksp_free_work(k);
    return rc;
  }
  k->cg_st = (mspi_cg_state *)k->gblock;
  k->cg_hist = (double *)((char *)k->gblock + st_bytes);
  k->setup = 1;
  if ((rc = ksp_pc_set_up(k))) ksp_free_work(k);
  return rc;
}

/* K iterations of KSPSolve_CG's loop from the state the last kernel left.  Enqueued, no host synchronisation. */
static int enqueue_cycle(msp_ksp *k, double *x, int K) {
  msp_ctx *c = k->ctx;
  const double *dinv = k->pc_type == MSP_PC_JACOBI ? k->dinv : NULL;
  const int unpre = k->norm_type == MSP_NORM_UNPRECONDITIONED;
  int rc = MSP_SUCCESS;
  for (int i = 0; i < K && !rc; ++i) {
    double *p = k->cg_p;
    if (k->cg_route == MSPI_CG_ROUTE_MARCH) {
      /* p ping-pongs: halo rows of p_new are recomputed from r and p_old, which no tile writes.  Every cycle starts
       * at an even iteration (ksp_cg_solve), so iteration i of a cycle writes cg_p when i is even */
      double *pold = (i & 1) ? k->cg_p : k->cg_p2;
      p = (i & 1) ? k->cg_p2 : k->cg_p;
      rc = mspi_cg_march(k->A, k->cg_r, dinv, pold, p, k->cg_w, k->cg_st);
    } else {
      rc = mspi_cg_aypx(c, k->cg_r, dinv, p, k->n, k->cg_st);
      if (!rc) rc = mspi_cg_matmult_dot(k->A, p, k->cg_w, k->cg_st, k->cg_route);
    }
    if (!rc) rc = mspi_cg_pw(c, k->cg_st);
    if (!rc) rc = mspi_cg_update(c, x, p, k->cg_r, k->cg_w, dinv, unpre, k->n, k->cg_st);
    if (!rc) rc = mspi_cg_iter_end(c, k->cg_st, k->cg_hist, k->n);
  }
  return rc;
}

int mspi_ksp_cg_set_route(msp_ksp *k, int route) {
  if (!k) {
    mspi_set_error(MSP_ERR_ARG_NULL, "NULL argument");
    return MSP_ERR_ARG_NULL;
  }
  if (route < MSPI_CG_ROUTE_AUTO || route > MSPI_CG_ROUTE_MARCH) {
    mspi_set_error(MSP_ERR_ARG_OUTOFRANGE, "KSPCG route %d", route);
    return MSP_ERR_ARG_OUTOFRANGE;
  }
  if (route != k->cg_route_set) { /* other launches in every captured cycle */
    msp_ctx_synchronize(k->ctx);
    ksp_drop_graphs(k);
  }
  k->cg_route_set = route;
  return MSP_SUCCESS;
}

/* The route of this solve, decided once: the best the operator takes, or the forced one if it takes that */
static int pick_route(msp_ksp *k) {
  const int best = mspi_cg_best_route(k->A), want = k->cg_route_set;
  int ok = want == MSPI_CG_ROUTE_AUTO || want == MSPI_CG_ROUTE_TWO;
  if (want == MSPI_CG_ROUTE_FUSED) ok = mspi_spmv_mdot_takes(k->A);
  if (want == MSPI_CG_ROUTE_MARCH) ok = mspi_cg_march_fits(k->A);
  if (!ok) {
    mspi_set_error(MSP_ERR_SUP, "MSP_KSP_CG: the operator does not take the forced route %d", want);
    return MSP_ERR_SUP;
  }
  const int route = want == MSPI_CG_ROUTE_AUTO ? best : want;
  if (route != k->cg_route) ksp_drop_graphs(k); /* e.g. the operator's storage was switched between two solves */
  k->cg_route = route;
  if (route == MSPI_CG_ROUTE_MARCH && !k->cg_p2) return mspi_malloc(k->ctx, (void **)&k->cg_p2, k->vec_bytes);
  return MSP_SUCCESS;
}

int ksp_cg_solve(msp_ksp *k, const msp_vec *b, msp_vec *x) {
  if (k->basis_prec != MSP_BASIS_F64) {
    mspi_set_error(MSP_ERR_SUP, "MSP_KSP_CG keeps no Krylov basis: %s applies to MSP_KSP_GMRES only",
                   k->basis_prec == MSP_BASIS_B16 ? "MSP_BASIS_B16" : "MSP_BASIS_F32");
    return MSP_ERR_SUP;
  }
  if (k->oper_prec != MSP_OPER_F64) {
    mspi_set_error(MSP_ERR_SUP, "MSP_KSP_CG is not built with MSP_OPER_F32: its recurrence has no restart that "
                                "would correct the rounded operator's residual");
    return MSP_ERR_SUP;
  }
  if (k->cgs != MSP_CGS_REFINE_NEVER) {
    mspi_set_error(MSP_ERR_SUP, "MSP_KSP_CG has no Gram-Schmidt step: %s applies to MSP_KSP_GMRES only",
                   k->cgs == MSP_CGS_REFINE_ALWAYS ? "MSP_CGS_REFINE_ALWAYS" : "MSP_CGS_REFINE_IFNEEDED");
    return MSP_ERR_SUP;
  }
  if (mspi_reduce_seq(k->ctx)) {
    mspi_set_error(MSP_ERR_SUP, "MSP_KSP_CG needs the DBR reduction: its fused kernels have no MSP_REDUCE_SEQ form");
    return MSP_ERR_SUP;
  }
  int rc = mspi_set_device(k->ctx);
  if (!rc) rc = msp_ksp_set_up(k);
  if (!rc) rc = pick_route(k); /* before any capture: it may allocate the second p buffer */
  if (!rc) rc = mspi_reserve_partial(k->ctx, k->n); /* the cycle hands the buffer's address to its kernels */
  if (rc) return rc;
  msp_ctx *c = k->ctx;
  const int jac = k->pc_type == MSP_PC_JACOBI;
  const double *dinv = jac ? k->dinv : NULL;
  const int unpre = k->norm_type == MSP_NORM_UNPRECONDITIONED;
  const int guess_zero = !k->o.guess_nonzero;

  mspi_cg_state *h = k->cg_hst;
  memset(h, 0, sizeof(*h));
  h->max_it = k->o.max_it;
  h->hist_cap = k->hist_cap;
  h->guess_zero = guess_zero;
  h->uirnorm = k->o.uirnorm;
  h->jacobi = jac;
  h->one = 1.0;
  h->rtol = k->o.rtol;
  h->abstol = k->o.abstol;
  h->divtol = k->o.divtol;
  if (!guess_zero && !k->o.uirnorm) { /* KSPConvergedDefault at n == 0 needs ||b||, under Jacobi ||dinv .* b|| */
    double bb = 0.0;
    if (jac) rc = mspi_pcj_apply_norm(c, b->d, k->dinv, k->cg_w, k->n, &k->cg_st->pw, NULL);
    else rc = mspi_norm2sq(c, b->d, k->n, &k->cg_st->pw);
    if (rc) return rc;
    if ((rc = mspi_d2h_sync(c, &bb, &k->cg_st->pw, sizeof(double)))) return rc;
    h->bnorm = sqrt(bb);
  }
  if ((rc = mspi_h2d_async(c, k->cg_st, h, sizeof(*h)))) return rc;
  /* x = 0 ; r = b, or r = b - A x for a nonzero guess */
  if (guess_zero) {
    if ((rc = mspi_set(c, x->d, k->n, 0.0))) return rc;
    rc = mspi_copy(c, k->cg_r, b->d, k->n);
  } else {
    rc = mspi_residual(k->A, b->d, x->d, k->cg_r);
  }
  if (!rc) rc = mspi_cg_sums(c, k->cg_r, dinv, unpre, k->n);
  if (!rc) rc = mspi_cg_start(c, k->cg_st, k->cg_hist, k->n);
  if (rc) return rc;
  int done = 0;
  for (;;) {
    int K = k->o.max_it - done;
    if (K > CG_CYCLE) K = CG_CYCLE;
    if (K > 0 && (rc = ksp_run_cycle(k, x->d, K, enqueue_cycle))) return rc;
    if ((rc = mspi_d2h_sync(c, h, k->cg_st, sizeof(*h)))) return rc; /* the one sync per cycle */
    if (h->stop || K <= 0) break;
    done = h->i;
  }
  k->its = h->its;
  k->reason = h->reason;
  k->rnorm = h->rnorm;
  k->nhist = h->nhist < k->hist_cap ? h->nhist : k->hist_cap;
  if (k->nhist && (rc = mspi_d2h_sync(c, k->hist, k->cg_hist, (size_t)k->nhist * sizeof(double)))) return rc;
  return MSP_SUCCESS;
}

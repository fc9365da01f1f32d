/*
 * ksp_impl.h -- struct msp_ksp, shared by the two KSP types' host logic: ksp_gmres.c (KSPGMRES, and everything
 * both types share: creation, options, the preconditioner's set-up, the graph cache, the result getters) and
 * ksp_cg.c (KSPCG).  Private to those two files.
 */
#ifndef MSPLIT_KSP_IMPL_H
#define MSPLIT_KSP_IMPL_H

#include "msplit.h"
#include "msplit_internal.h"

/* Captured cycles (HIP graphs), keyed by everything the capture baked
 * in: the operator and the kernels its products launch, the context's DBR
 * partial buffer (its epoch), x, the cycle length K, the KSP type, the tuning flags and the launch-shape overrides.
 * The work vectors and the device state are fixed between ksp_free_work calls, which drop the cache. */
#define KSP_NGRAPH 4
typedef struct {
  void *exec;
  const msp_mat *A;
  uint64_t aver, epoch;
  const double *x;
  int K, tuning, shape, type;
} ksp_graph;

struct msp_ksp {
  msp_ctx *ctx;
  ksp_graph graphs[KSP_NGRAPH];
  int gnext;
  int graphs_off; /* a capture failed on this KSP's stream (e.g. the legacy null stream): eager from then on */
  msp_mat *A;
  msp_ksp_opts o;
  int type;                 /* MSP_KSP_GMRES / MSP_KSP_CG */
  int norm_type;            /* MSP_NORM_PRECONDITIONED / MSP_NORM_UNPRECONDITIONED: read by MSP_KSP_CG only */
  int setup;
  int64_t n, stride;
  int basis_prec;           /* MSP_BASIS_F64 / MSP_BASIS_F32 / MSP_BASIS_B16: the element type behind basis */
  double *basis;            /* device: (m+1) * stride, stored unnormalised (scales in g.sc); floats when F32, int16
                               followed by the exponent table when B16 */
  int32_t *expo;            /* device, B16 only: exponents [vector][nchunks], inside the basis allocation */
  int64_t nchunks;          /* DBR chunks per vector */
  double *tmp;              /* device: W = A VV(it) before the orthogonalisation */
  double *cur;              /* device, F32 / B16: the newest basis vector's rounded values as doubles */
  int pc_type;              /* MSP_PC_NONE / MSP_PC_JACOBI */
  double *dinv;             /* device, Jacobi: n doubles, 1 / a_ii by PCSetUp's rule */
  int dinv_valid;           /* dinv holds the current operator's (reset by msp_ksp_set_operators) */
  int oper_prec;            /* MSP_OPER_F64 / MSP_OPER_F32: what the Arnoldi MatMult reads */
  int cgs;                  /* MSP_CGS_REFINE_NEVER / _IFNEEDED / _ALWAYS */
  mspi_gmres_refine *rf;    /* device: the refinement's block, behind the recurrence arrays in gblock */
  int nrefine;              /* steps of the last solve that ran pass 2 */
  size_t basis_bytes, gblock_bytes, vec_bytes; /* sizes of the allocations (vec_bytes: tmp and cur, each) */
  mspi_gmres_dev g;         /* device-resident recurrence state and arrays */
  void *gblock;             /* the single device allocation behind g (CG: behind cg_st and cg_hist) */
  mspi_gmres_state *hst;    /* pinned host mirror of *g.st */
  /* MSP_KSP_CG: r, w, p (vec_bytes each), the state at the head of gblock with the history behind it */
  double *cg_r, *cg_w, *cg_p;
  double *cg_p2;            /* device: the second p buffer of MSPI_CG_ROUTE_MARCH (p ping-pongs), allocated by the
                               first solve that takes that route */
  mspi_cg_state *cg_st;     /* device */
  double *cg_hist;          /* device: hist_cap */
  mspi_cg_state *cg_hst;    /* pinned host mirror of *cg_st */
  int cg_route_set;         /* mspi_ksp_cg_set_route: MSPI_CG_ROUTE_AUTO (after creation) or a forced route */
  int cg_route;             /* the route of the running solve */
  double *hist;             /* host copy of the residual history */
  int hist_cap, nhist;
  int its, reason;
  double rnorm;
};

/* ksp_gmres.c */
void ksp_free_work(msp_ksp *k);
void ksp_drop_graphs(msp_ksp *k);
int ksp_pc_set_up(msp_ksp *k); /* PCSetUp of MSP_PC_JACOBI: dinv allocated with the work, computed once per operator */
/* K iterations through the graph cache: captured the first time the key is seen, then replayed; eager where graphs
 * are off.  enqueue(k, x, K) enqueues them without a host synchronisation. */
int ksp_run_cycle(msp_ksp *k, double *x, int K, int (*enqueue)(msp_ksp *, double *, int));

/* ksp_cg.c */
int ksp_cg_set_up(msp_ksp *k);
int ksp_cg_solve(msp_ksp *k, const msp_vec *b, msp_vec *x);

#endif

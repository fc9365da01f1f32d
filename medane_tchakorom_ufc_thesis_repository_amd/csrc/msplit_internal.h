/*
 * msplit_internal.h -- what the C host side (ksp_gmres.c) needs from the HIP
 * side (msplit_runtime.hip / msplit_kernels.hip / msplit_k_*.hip).  Raw device pointers, all
 * work stream-ordered on the context's stream.
 */
#ifndef MSPLIT_INTERNAL_H
#define MSPLIT_INTERNAL_H

#include <stddef.h>
#include <stdint.h>

#include "msplit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest number of vectors one MDot / MAXPY launch handles; more are split
 * into groups (the per-vector arithmetic does not depend on the grouping). */
#define MSPI_MAX_GROUP 32
#define MSPI_DBR_CHUNK 4096 /* elements per DBR chunk (MSK_DBR_CHUNK) */

struct msp_vec {
  msp_ctx *ctx;
  int64_t n;
  double *d;
  int owned;
};

void mspi_set_error(int code, const char *fmt, ...);

/* scratch: device doubles (>= 2*MSPI_MAX_GROUP+8) and pinned host doubles (same) */
double *mspi_dev_scratch(msp_ctx *ctx);
double *mspi_host_scratch(msp_ctx *ctx);
int mspi_malloc(msp_ctx *ctx, void **p, size_t bytes);
/* hipMalloc of a large buffer, physically contiguous from 64 MiB where the driver can (MSPLIT_ALLOC_CONTIGUOUS=0: plain) */
int mspi_big_alloc(void **p, size_t bytes); /* 0 = hipSuccess */
int mspi_free(msp_ctx *ctx, void *p);
/* pinned host memory (for per-iteration scalars) */
int mspi_host_malloc(void **p, size_t bytes);
int mspi_host_free(void *p);
int mspi_set_device(msp_ctx *ctx);
/* reference counting of the context by the objects made on it (msp_ctx_destroy releases the caller's) */
void mspi_ctx_retain(msp_ctx *ctx);
void mspi_ctx_release(msp_ctx *ctx);
/* async device->host copy followed by a stream synchronise */
int mspi_d2h_sync(msp_ctx *ctx, void *host, const void *dev, size_t bytes);

int mspi_mat_dims(const msp_mat *A, int32_t *nrows, int32_t *ncols);
msp_ctx *mspi_mat_ctx(const msp_mat *A);
typedef struct {
  const int32_t *rowptr, *col;
  const double *val;
  int64_t nnz;
  int compressed;
  int32_t lds_cap; /* LDS entries per 256-row block for the staged kernels (0: rows too long) */
} mspi_csr_view;
mspi_csr_view mspi_mat_csr(const msp_mat *A);
/* R = A S over DV storage (ELL layout); MSP_ERR_SUP when A is not in it */
int mspi_mat_spmm_dv(msp_mat *A, const double *S, int64_t lds, int nc, int64_t srows, double *R, int64_t ldr);
/* the same into a float R (each f64 row sum rounded once); always the ELL SpMM */
int mspi_mat_spmm_dv_f32(msp_mat *A, const double *S, int64_t lds, int nc, int64_t srows, float *R, int64_t ldr);

/* dense row block, column-major, lda (in elements) a multiple of 512 (doubles) or 1024 (floats) */
struct msp_dense {
  msp_ctx *ctx;
  int64_t nrows;
  int32_t ncols;
  int64_t lda;
  double *d; /* the storage; floats when prec == MSP_DENSE_F32 */
  int view; /* msp_dense_create_view: columns of another block, storage not freed */
  int prec; /* MSP_DENSE_F64 / MSP_DENSE_F32 */
};

/* y = A[:, 0:nc] coef (+ (*nal_dev) U when U != NULL, skipped when *nal_dev == 0); usc_dev != NULL: U is
 * stored unscaled and its value is U * (*usc_dev) (a deferred VecScale, rounded as the scale would have been);
 * sumsq_dev != NULL: also ||y||^2 (DBR; partial holds nchunks doubles). */
int mspi_dense_gemv(msp_ctx *ctx, const double *A, int64_t lda, int nc, int64_t n, const double *coef_dev,
                    const double *nal_dev, const double *U, const double *usc_dev, double *y, double *partial,
                    double *sumsq_dev, const int *stop);
/* sc_dev != NULL: w = win * (*sc_dev) first, stored to wout unless wout == NULL (deferred: the next reader
 * scales); out_dev[j] = column_j . w (DBR), j < nc.
 * partial holds nchunks*32 doubles. */
int mspi_dense_scaled_dots(msp_ctx *ctx, const double *win, double *wout, const double *sc_dev, const double *A,
                           int64_t lda, int nc, int64_t n, double *partial, double *out_dev, const int *stop);
/* one LSQR step's U1 = A coef + nal (U usc) (unscaled) with out[0] = ||U1||^2, out[1 + v] = A_v . U1 (DBR),
 * in one pass over A where it can (msplit_dense.hip); partial: nchunks * (nc + 1) doubles */
int mspi_dense_lsqr_onepass(msp_ctx *ctx, const double *A, int64_t lda, int nc, int64_t n, const double *coef_dev,
                            const double *nal_dev, const double *U, const double *usc_dev, double *y,
                            double *partial, double *out_dev, const int *stop);
/* out_dev[j] = ||column j||^2 (DBR) */
int mspi_dense_colsumsq(msp_ctx *ctx, const double *A, int64_t lda, int nc, int64_t n, double *partial,
                        double *out_dev);

/* The four above over a block of either precision: A points at its elements, prec is MSP_DENSE_F64 or
 * MSP_DENSE_F32 (floats promoted as read; every sum f64, in the same order).  MSP_REDUCE_SEQ with an F32 block:
 * MSP_ERR_SUP. */
int mspi_dense_gemv_p(msp_ctx *ctx, const void *A, int prec, int64_t lda, int nc, int64_t n, const double *coef_dev,
                      const double *nal_dev, const double *U, const double *usc_dev, double *y, double *partial,
                      double *sumsq_dev, const int *stop);
int mspi_dense_scaled_dots_p(msp_ctx *ctx, const double *win, double *wout, const double *sc_dev, const void *A,
                             int prec, int64_t lda, int nc, int64_t n, double *partial, double *out_dev,
                             const int *stop);
int mspi_dense_lsqr_onepass_p(msp_ctx *ctx, const void *A, int prec, int64_t lda, int nc, int64_t n,
                              const double *coef_dev, const double *nal_dev, const double *U, const double *usc_dev,
                              double *y, double *partial, double *out_dev, const int *stop);
int mspi_dense_colsumsq_p(msp_ctx *ctx, const void *A, int prec, int64_t lda, int nc, int64_t n, double *partial,
                          double *out_dev);

/* y = A x ; r = b - A x */
int mspi_spmv(msp_mat *A, const double *x, double *y);
int mspi_residual(msp_mat *A, const double *b, const double *x, double *r);
/* out_dev[j] = w . V[j] (DBR order), j < nv; any nv (grouped internally) */
int mspi_mdot(msp_ctx *ctx, const double *w, int nv, const double *const *V, int64_t n, double *out_dev);
/* out_dev[0] = x . x (DBR order) */
int mspi_norm2sq(msp_ctx *ctx, const double *x, int64_t n, double *out_dev);
/* w = w + sum_j a_j V[j] (PETSc 4-grouping), a_j = (negate ? -1 : 1) * alpha[j];
 * alpha is a host array (alpha_host) or a device array (alpha_dev).
 * accumulate_into_x: w_out = w + (0 + sum) instead (BuildSoln's VecSet(T,0);
 * VecMAXPY(T); VecAXPY(x,1,T) in one pass). */
int mspi_maxpy(msp_ctx *ctx, double *w, int nv, const double *const *V, int64_t n, const double *alpha_host,
               const double *alpha_dev, int negate, int accumulate_into_x);
int mspi_scale(msp_ctx *ctx, double *x, int64_t n, double alpha);
int mspi_copy(msp_ctx *ctx, double *dst, const double *src, int64_t n);
int mspi_set(msp_ctx *ctx, double *x, int64_t n, double alpha);

/* ---- device-resident KSPGMRES state (msplit_gmres.hip) ---- */
typedef struct {
  int32_t stop;        /* cycle over: later kernels of this cycle return at once */
  int32_t skip_build;  /* cycle returned before BuildSoln (PETSc's early PetscFunctionReturn) */
  int32_t it;          /* iterations done in this cycle */
  int32_t its;         /* ksp->its */
  int32_t reason;      /* KSPConvergedReason */
  int32_t nhist;       /* residual history entries written */
  int32_t nbuild;      /* vectors BuildSoln combines (it of BuildSoln + 1, or 0) */
  int32_t guess_zero;  /* the solve's original zero-guess flag (KSPConvergedDefault n == 0) */
  int32_t m, max_it, uirnorm, hist_cap;
  double res, rnorm, rnorm0, ttol, gm_rnorm0;
  double scale;        /* VecNormalize factor of the newest vector (also kept in sc[it]) */
  double bnorm;        /* ||b|| for the n == 0 test with a nonzero guess and no UIRNorm */
  double rtol, abstol, divtol, haptol, breakdowntol;
} mspi_gmres_state;

typedef struct {
  mspi_gmres_state *st; /* device */
  double *hh;           /* (m+2) x (m+1), HH(a,b) = hh[b*(m+2)+a] */
  double *cc, *ss, *grs; /* m+2 each */
  double *h;            /* m+2: MDot results h(0..it), then ||w||^2 at h(it+1) */
  double *sc;           /* m+2: deferred VecNormalize, VV(j) = stored VV(j) * sc[j] */
  double *hist;         /* hist_cap */
} mspi_gmres_dev;

/* one-lane kernels of the GMRES recurrence */
int mspi_gm_cycle_start(msp_ctx *ctx, mspi_gmres_dev g, const double *sumsq_dev);
int mspi_gm_iter_update(msp_ctx *ctx, mspi_gmres_dev g);
int mspi_gm_build(msp_ctx *ctx, mspi_gmres_dev g, int m); /* m: the restart H and GRS are sized for */
/* fold the ||w||^2 partials (stage-2 DBR) and run the Hessenberg update, one launch */
int mspi_gm_norm_update(msp_ctx *ctx, mspi_gmres_dev g, const double *partial, int64_t nchunks, int m);
/* CGS VecMAXPY + ||w||^2 partials, then mspi_gm_norm_update (h(it+1) = ||w||^2) */
int mspi_maxpy_norm_update(msp_ctx *ctx, const double *win, double *wout, int nv, const double *base, int64_t stride,
                           const double *scale, int64_t n, mspi_gmres_dev g, int it, int m, const int *stop);
/* data-path pieces with a stop flag; basis = VV(j) at base + j*stride, its value
   VV(j)[i] * scale[j] when scale (device) is not NULL */
int mspi_spmv_scaled(msp_mat *A, const double *x, const double *sdev, double *vout, double *y, const int *stop);
int mspi_spmv_mdot(msp_mat *A, const double *x, const double *sdev, double *y, int nv, const double *base,
                   int64_t stride, const double *scale, double *out_dev, const int *stop);
/* the W-free step for box stencils: mspi_spmv_mdot(.., y = NULL, ..) then mspi_maxpy_norm_update_march, which
   recomputes W = A (sdev[0] x) (x = VV(it), the basis' last vector) -- bitwise the stored-W step */
int mspi_gm_wfree(const msp_mat *A);
int mspi_maxpy_norm_update_march(msp_mat *A, const double *x, const double *sdev, double *wout, int nv,
                                 const double *base, int64_t stride, const double *scale, mspi_gmres_dev g, int m,
                                 const int *stop);
int mspi_mdot_basis(msp_ctx *ctx, const double *w, int nv, const double *base, int64_t stride, const double *scale,
                    int64_t n, double *out_dev, const int *stop);
int mspi_maxpy_norm_basis(msp_ctx *ctx, const double *win, double *wout, int nv, const double *base, int64_t stride,
                          const double *scale, int64_t n, const double *alpha_dev, double *sumsq_dev, const int *stop);
int mspi_maxpy_accum_basis(msp_ctx *ctx, double *x, const int *nvdev, const double *base, int64_t stride,
                           const double *scale, int64_t n, const double *coef_dev, int nv_expected);
int mspi_h2d_async(msp_ctx *ctx, void *dev, const void *host, size_t bytes);
/* ---- CGS iterative refinement (MSP_CGS_REFINE_IFNEEDED / _ALWAYS): a second Gram-Schmidt pass decided on the
   device.  The block lives behind the recurrence arrays in the KSP's device block (mspi_gmres_state and
   mspi_gmres_dev are unchanged); c follows the header, m + 2 doubles. ---- */
typedef struct {
  int32_t mode;   /* MSP_CGS_REFINE_* */
  int32_t refine; /* this step runs pass 2 (written by the decide kernel) */
  int32_t skip;   /* stop || !refine: the flag pass 2's MAXPY returns on; 1 outside a step's decide..update window */
  int32_t count;  /* steps of this solve that ran pass 2 */
  double ss1;     /* ||u||^2 after pass 1 */
  double ss2;     /* ||u'||^2 after pass 2 (written by the update kernel on a refined step) */
} mspi_gmres_refine;
/* c(0..it) = u . v_j: the m + 2 doubles behind the header */
#define MSPI_REFINE_C(rf) ((double *)((rf) + 1))
#define MSPI_REFINE_BYTES(m) (sizeof(mspi_gmres_refine) + (size_t)((m) + 2) * sizeof(double))
/* Pass 1 fused with pass 2's MDot stage 1 (k_maxpy_mdot): wout = win - sum_j alpha_j scale_j VV(j), then the DBR
   partials of wout . scale_v VV(v) in rows 0..nv-1 and of ||wout||^2 in row nv of the context's partial buffer: bit
   for bit mspi_maxpy_norm_basis followed by mspi_mdot_basis on wout.  c_dev != NULL: the rows are folded here
   (stage 2) into c_dev[0..nv-1] and sumsq_dev[0]; NULL: left for mspi_gm_refine_decide.  nv + 1 <= MSPI_MAX_GROUP
   and the DBR reduction, else MSP_ERR_SUP. */
int mspi_maxpy_norm_mdot_basis(msp_ctx *ctx, const double *win, double *wout, int nv, const double *base,
                               int64_t stride, const double *scale, int64_t n, const double *alpha_dev, double *c_dev,
                               double *sumsq_dev, const int *stop);
/* 1 when a refined step of nv vectors takes the fused kernel (nv + 1 <= MSPI_MAX_GROUP and MSPLIT_GM_REFINE_FUSED
   not 0) */
int mspi_gm_refine_fused(int nv);
/* The decision of step it = st->it (one workgroup).  partial != NULL: rows 0..it and row it + 1 of the fused pass'
   partials are folded into rf->c and rf->ss1 first (stage 2's order); NULL: both are already there.  Then refine,
   skip and count.  A no-op when st->stop is set. */
int mspi_gm_refine_decide(msp_ctx *ctx, mspi_gmres_dev g, mspi_gmres_refine *rf, const double *partial,
                          int64_t nchunks);
/* Pass 2's MAXPY in place, w = w - sum_j c_j scale_j VV(j) with the ||w||^2 partials (k_maxpy_chunk unchanged),
   returning at once when rf->skip is set */
int mspi_gm_refine_maxpy2(msp_ctx *ctx, double *w, int nv, const double *base, int64_t stride, const double *scale,
                          int64_t n, const mspi_gmres_refine *rf);
/* mspi_gm_norm_update with the column h + c and tt = sqrt(refine ? ss2 : ss1); ss2 folded from partial on a refined
   step.  Leaves rf->skip = 1. */
int mspi_gm_refine_update(msp_ctx *ctx, mspi_gmres_dev g, mspi_gmres_refine *rf, const double *partial,
                          int64_t nchunks, int m);
/* the context's DBR partial buffer (valid after mspi_reserve_partial; enqueued work points at it) */
const double *mspi_ctx_partial(msp_ctx *ctx);
/* ---- MSP_BASIS_F32: the same steps over a basis stored as float (msplit_cgs_basis.hip), VV(j) = base + j*stride with its
   value (double)VV(j)[i] * scale[j]; all arithmetic f64, DBR only.  rnd(v) = (double)(float)v. ---- */
/* cur = rnd(r) (f64; may be r itself), v0 = the same as float, sumsq_dev[0] = sum rnd(r)^2 */
int mspi_cb_round_store(msp_ctx *ctx, const double *r, double *cur, float *v0, int64_t n, double *sumsq_dev,
                        const int *stop);
int mspi_cb_mdot(msp_ctx *ctx, const double *w, int nv, const float *base, int64_t stride, const double *scale,
                 int64_t n, double *out_dev, const int *stop);
/* s = rnd(win - sum_j h_j VV(j)) stored to vout (float) and cur (f64), ||s||^2, then mspi_gm_norm_update */
int mspi_cb_maxpy_norm_update(msp_ctx *ctx, const double *win, double *cur, float *vout, int nv, const float *base,
                              int64_t stride, const double *scale, int64_t n, mspi_gmres_dev g, int m,
                              const int *stop);
int mspi_cb_accum(msp_ctx *ctx, double *x, const int *nvdev, const float *base, int64_t stride, const double *scale,
                  int64_t n, const double *coef_dev, int nv_expected);
/* ---- MSP_BASIS_B16: the same steps over a basis stored as int16 with one int32 exponent per DBR chunk and vector
   (msplit_cgs_basis.hip), VV(j) = base + j*stride, its exponents ebase + j*ceil(n/4096); all arithmetic f64, DBR only.
   rnd16 is the rule of include/msplit.h. ---- */
/* cur = rnd16(r) (f64; may be r itself), v0 / e0 = the same as block16, sumsq_dev[0] = sum rnd16(r)^2 */
int mspi_cb16_round_store(msp_ctx *ctx, const double *r, double *cur, int16_t *v0, int32_t *e0, int64_t n,
                          double *sumsq_dev, const int *stop);
int mspi_cb16_mdot(msp_ctx *ctx, const double *w, int nv, const int16_t *base, int64_t stride, const int32_t *ebase,
                   const double *scale, int64_t n, double *out_dev, const int *stop);
/* s = rnd16(win - sum_j h_j VV(j)) stored to vout / eout and cur (f64), ||s||^2, then mspi_gm_norm_update */
int mspi_cb16_maxpy_norm_update(msp_ctx *ctx, const double *win, double *cur, int16_t *vout, int32_t *eout, int nv,
                                const int16_t *base, int64_t stride, const int32_t *ebase, const double *scale,
                                int64_t n, mspi_gmres_dev g, int m, const int *stop);
int mspi_cb16_accum(msp_ctx *ctx, double *x, const int *nvdev, const int16_t *base, int64_t stride,
                    const int32_t *ebase, const double *scale, int64_t n, const double *coef_dev, int nv_expected);
/* ---- MSP_PC_JACOBI: left Jacobi preconditioning fused into the CGS kernels over the f64 basis (msplit_cgs_basis.hip);
   dinv = n doubles from mspi_pcj_diag_inv, w = W .* dinv formed as W is loaded (W stays as the MatMult wrote it),
   everything after that multiply the f64 step's arithmetic; DBR only. ---- */
/* d_i = a_ii (0.0 where row i stores none); MSP_ERR_SUP unless A holds its CSR arrays (not row-compressed, not
   matrix-free, not released), MSP_ERR_ARG_SIZ unless A is square */
int mspi_mat_diagonal(const msp_mat *A, double *d);
/* PCSetUp: dinv_i = 1 / a_ii, 1.0 where a_ii is +-0.0 or absent; the same refusals */
int mspi_pcj_diag_inv(const msp_mat *A, double *dinv);
/* z = r .* dinv (z may be r itself), sumsq_dev[0] = sum z^2 */
int mspi_pcj_apply_norm(msp_ctx *ctx, const double *r, const double *dinv, double *z, int64_t n, double *sumsq_dev,
                        const int *stop);
int mspi_pcj_mdot(msp_ctx *ctx, const double *w, const double *dinv, int nv, const double *base, int64_t stride,
                  const double *scale, int64_t n, double *out_dev, const int *stop);
/* vout = (win .* dinv) - sum_j h_j VV(j), ||vout||^2, then mspi_gm_norm_update */
int mspi_pcj_maxpy_norm_update(msp_ctx *ctx, const double *win, const double *dinv, double *vout, int nv,
                               const double *base, int64_t stride, const double *scale, int64_t n, mspi_gmres_dev g,
                               int m, const int *stop);
/* ---- MSP_OPER_F32: the Arnoldi MatMult over a single-precision copy of the CSR values (msplit_csr32.hip) ---- */
/* Build the copy, or rebuild a stale one (keyed to mspi_mat_version); allocates and synchronises, so never inside a
   graph capture.  MSP_ERR_SUP unless A's products read its CSR arrays (naming the storage), MSP_ERR_ARG_OUTOFRANGE
   with the count when finite values overflow the float range (no copy is kept). */
int mspi_mat_ensure_p32(msp_mat *A);
/* y = A~ (sdev[0] x): bit for bit mspi_spmv_scaled on a matrix whose values are (double)(float)a; honours stop */
int mspi_spmv_scaled_p32(msp_mat *A, const double *x, const double *sdev, double *y, const int *stop);
/* ---- the GMRES step's MatMult inside the CGS kernels (A in DV storage, 8-code ELL layout) ---- */
int mspi_op_fusable(const msp_mat *A);
/* h(0..nv-1) = (A (sdev[0] x)) . scale_j VV(j): stage 1 computes each row of A(sc x) in registers */
int mspi_mdot_op(msp_mat *A, const double *x, const double *sdev, int nv, const double *base, int64_t stride,
                 const double *scale, double *out_dev, const int *stop);
/* VV(it+1) = A (sdev[0] x) - sum_j h_j scale_j VV(j), ||VV(it+1)||^2, then the Hessenberg update */
int mspi_maxpy_norm_update_op(msp_mat *A, const double *x, const double *sdev, double *wout, int nv,
                              const double *base, int64_t stride, const double *scale, mspi_gmres_dev g, int m,
                              const int *stop);
/* ---- HIP graphs of enqueued work (a GMRES restart cycle is replayed as one graph launch) ---- */
/* 1 unless MSPLIT_GRAPHS=0 or per-kernel timing is on (its events need eager launches) */
int mspi_graphs_enabled(msp_ctx *ctx);
/* the DBR partial buffer sized for n-element work, so nothing allocates during a capture */
int mspi_reserve_partial(msp_ctx *ctx, int64_t n);
int mspi_capture_begin(msp_ctx *ctx);
/* ok = 0: the enqueue failed, end and drop the capture; *exec receives the instantiated graph otherwise */
int mspi_capture_end(msp_ctx *ctx, int ok, void **exec);
int mspi_graph_launch(msp_ctx *ctx, void *exec);
void mspi_graph_destroy(void *exec);
/* changes whenever the kernels a product of A launches change (storage switch, CSR release) */
uint64_t mspi_mat_version(const msp_mat *A);
/* changes whenever a context buffer that enqueued work points at (the DBR partials) is reallocated */
uint64_t mspi_ctx_epoch(const msp_ctx *ctx);
int msk_get_tuning(void);
/* bumped by every launch-shape override (msk_set_march_z / _lines / msk_set_spmv_group) */
int msk_get_shape_epoch(void);
int msk_get_gm_wfree(void);
int mspi_h2d_sync(msp_ctx *ctx, void *dev, const void *host, size_t bytes);
/* free and total HBM of the context's device (hipMemGetInfo) */
int mspi_mem_info(msp_ctx *ctx, size_t *free_bytes, size_t *total_bytes);
/* ---- HBM mailboxes shared between processes (msplit_ipc.hip) ---- */
#define MSPI_IPC_HANDLE_BYTES 64
int mspi_dev_alloc(msp_ctx *ctx, size_t bytes, void **p); /* zeroed */
int mspi_dev_free(void *p);
int mspi_ipc_export(void *p, uint8_t *handle);
int mspi_ipc_open(msp_ctx *ctx, const uint8_t *handle, void **p);
int mspi_ipc_close(void *p);
/* height rows of width bytes, pitched, device to device; synchronises the context's stream */
int mspi_d2d_sync(msp_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width,
                  size_t height);
/* page-lock a host range (shared-memory mailboxes) for DMA */
/* the asynchronous device slots (amsg.c): a copy enqueued without waiting, and a word of a registered host region
 * stored by the stream once the work before it is done (system-scope release) */
int mspi_d2d_async(msp_ctx *ctx, void *dst, const void *src, size_t bytes);
int mspi_d2d_async2d(msp_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width,
                     size_t height);
int mspi_host_device_ptr(void *host, void **dev);
uint64_t mspi_stream_key(const msp_ctx *ctx);
int mspi_stream_store_u64(msp_ctx *ctx, uint64_t *dev_word, uint64_t v);
int mspi_stream_store_u32(msp_ctx *ctx, uint32_t *dev_word, uint32_t v);
int mspi_host_register(void *p, size_t bytes);
int mspi_host_unregister(void *p);

/* ---- cross-process all-gather (msplit_comm.hip); comm may be NULL (1 rank) ---- */
int mspi_comm_allgather(msp_comm *comm, const double *send_dev, double *recv_dev, int64_t count);
int mspi_comm_size(const msp_comm *comm, int32_t *nranks, int32_t *rank);

/* ---- device-resident KSPLSQR state (msplit_lsqr.hip) ---- */
typedef struct {
  int32_t stop;        /* solve over: later kernels return at once */
  int32_t reason, its, nhist;
  int32_t i;           /* loop counter of KSPSolve_LSQR */
  int32_t max_it, conv_test, exact_norm, hist_cap;
  int32_t s;           /* columns of R */
  int32_t nblk;        /* row blocks over all ranks */
  int32_t pad;
  double rnorm, rnorm0, ttol, arnorm, anorm;
  double alpha, beta, phibar, rhobar;
  double uscale;       /* VecScale factor of the newest U (1/beta, or 1 when beta == 0) */
  double nalpha;       /* -alpha of VecAXPY(U1, -alpha, U) */
  double rtol, abstol, divtol;
} mspi_lsqr_state;

typedef struct {
  mspi_lsqr_state *st;  /* device */
  double *V, *V1, *W, *X; /* s entries each (X: the solution vector) */
  double *g;            /* all-gathered block partials, nblk * m */
  double *hist;         /* hist_cap */
} mspi_lsqr_dev;

/* ---- device-resident KSPCG state and step launchers (msplit_k_cg.hip, driven by ksp_cg.c) ---- */
typedef struct {
  int32_t stop;        /* solve over: later kernels return at once */
  int32_t reason;      /* KSPConvergedReason */
  int32_t its;         /* ksp->its */
  int32_t i;           /* loop counter of KSPSolve_CG: the iteration the next launches run */
  int32_t nhist;       /* residual history entries written */
  int32_t max_it, hist_cap;
  int32_t guess_zero, uirnorm;
  int32_t jacobi;      /* two sums per sweep: row 0 = z . r, row 1 = ||z||^2 or ||r||^2 */
  int32_t pad[2];
  double one;          /* 1.0: the scale the fused MatMult + dot multiplies by */
  double a, na;        /* beta / dpi and its negation (VecAXPY's two scalars) */
  double b;            /* beta / betaold (VecAYPX's scalar) */
  double pw;           /* p . w as the dot's stage 2 left it; mspi_cg_pw moves it into dpi */
  double beta, betaold, dpi, dpiold;
  double dp, rnorm, rnorm0, ttol;
  double bnorm;        /* ||b|| resp. ||dinv .* b|| for KSPConvergedDefault(0) with a nonzero guess and no UIRNorm */
  double rtol, abstol, divtol;
} mspi_cg_state;

/* Every launcher below honours st->stop (no store), writes its outputs and nothing else, and neither sums nor
   writes beyond n.  DBR reduction only.  dinv == NULL: PCNONE (z is r). */
/* p = z + st->b p with z = dinv .* r formed in registers; p = z when st->i == 0 */
int mspi_cg_aypx(msp_ctx *ctx, const double *r, const double *dinv, double *p, int64_t n, const mspi_cg_state *st);
/* The routes of an iteration's p, w = A p and p . w; all give the same bits.  mspi_cg_best_route: the one a solve
   takes by default, asked once per solve (nothing is probed inside the cycle): FUSED where A takes it, else TWO.
   MARCH measured slower than FUSED and is taken only when mspi_ksp_cg_set_route forces it. */
#define MSPI_CG_ROUTE_AUTO (-1)
#define MSPI_CG_ROUTE_TWO 0   /* mspi_cg_aypx, MatMult, dot */
#define MSPI_CG_ROUTE_FUSED 1 /* mspi_cg_aypx, the operator's fused MatMult + self-dot (mspi_spmv_mdot_takes) */
#define MSPI_CG_ROUTE_MARCH 2 /* mspi_cg_march: the AYPX folded into the chunk-tile march (mspi_cg_march_fits) */
int mspi_spmv_mdot_takes(const msp_mat *A);
int mspi_cg_march_fits(const msp_mat *A);
int mspi_cg_best_route(const msp_mat *A);
/* w = A p and st->pw = p . w (both DBR stages) by MSPI_CG_ROUTE_FUSED or MSPI_CG_ROUTE_TWO */
int mspi_cg_matmult_dot(msp_mat *A, const double *p, double *w, mspi_cg_state *st, int route);
/* pnew = z + st->b pold (pnew = z at st->i == 0, pold not read), w = A pnew, st->pw = pnew . w; pnew != pold */
int mspi_cg_march(msp_mat *A, const double *r, const double *dinv, const double *pold, double *pnew, double *w,
                  mspi_cg_state *st);
/* Test and measurement hook: the route this KSP's CG solves take (MSPI_CG_ROUTE_AUTO, the default: the best one);
   a route the operator does not take is MSP_ERR_SUP at solve.  Drops the captured cycles. */
int mspi_ksp_cg_set_route(msp_ksp *ksp, int route);
/* the scalar step after p . w: the sign tests, betaold, a (one lane) */
int mspi_cg_pw(msp_ctx *ctx, mspi_cg_state *st);
/* x += a p ; r += (-a) w ; stage-1 partials of z . r (row 0) and, under Jacobi, of ||z||^2 or ||r||^2 (row 1) */
int mspi_cg_update(msp_ctx *ctx, double *x, const double *p, double *r, const double *w, const double *dinv,
                   int norm_unpre, int64_t n, const mspi_cg_state *st);
/* the same sums of the initial residual, nothing written but the partials; no stop flag */
int mspi_cg_sums(msp_ctx *ctx, const double *r, const double *dinv, int norm_unpre, int64_t n);
/* stage 2 of the initial sums, dp, hist[0], KSPConvergedDefault(0), beta and the tests of iteration 0 */
int mspi_cg_start(msp_ctx *ctx, mspi_cg_state *st, double *hist, int64_t n);
/* stage 2 of the sweep's sums, dp, history, KSPConvergedDefault(i + 1), beta, and the top of iteration i + 1 */
int mspi_cg_iter_end(msp_ctx *ctx, mspi_cg_state *st, double *hist, int64_t n);

/* ---- MSP_REDUCE_SEQ (msplit_seq.hip) ---- */
int mspi_reduce_seq(const msp_ctx *ctx);
#define MSPI_SEQ_MAXSEG 16
typedef struct {
  int32_t nseg;
  const double *x[MSPI_SEQ_MAXSEG]; /* segment k: column j at x[k] + j*ldx[k] */
  int64_t ldx[MSPI_SEQ_MAXSEG];
  const double *y[MSPI_SEQ_MAXSEG]; /* the vector each column is dotted with (unused by frob) */
  int64_t n[MSPI_SEQ_MAXSEG];
} mspi_seq_segs;
/* One sequential sum per column j < ncol of column_j . y chained over the segments in order
 * (frob != 0: one sum of the squares of every column, columns outer, segments inner).  out[k*m + j]
 * of the last segment k holds the sum (frob: the last segment's column ncol-1), every other slot
 * of the first ncol columns +0.0, so a block-order sum of the slots is the chained sum. */
int mspi_seq_chain(msp_ctx *ctx, const mspi_seq_segs *sg, int ncol, int frob, double *out, int m, const int *stop);

/* one-lane kernels of the LSQR recurrence (g holds nblk values / nblk*s values) */
int mspi_ls_start(msp_ctx *ctx, mspi_lsqr_dev d);
int mspi_ls_first(msp_ctx *ctx, mspi_lsqr_dev d, const double *gfrob);
int mspi_ls_beta(msp_ctx *ctx, mspi_lsqr_dev d);
int mspi_ls_step(msp_ctx *ctx, mspi_lsqr_dev d);
int mspi_ls_onepass_step(msp_ctx *ctx, mspi_lsqr_dev d);

#ifdef __cplusplus
}
#endif
#endif

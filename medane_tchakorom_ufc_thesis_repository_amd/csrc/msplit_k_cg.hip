// msplit_k_cg.hip -- the kernels of KSPCG (MSP_KSP_CG) and their launchers; ksp_cg.c owns the solve.
//
// One CG iteration is, in launch order:
//   k_cg_aypx      p = z + b p, z = dinv .* r formed in registers (p = z at i = 0)
//   MatMult + dot  w = A p and p . w: the operator's fused MatMult + self-dot (mspi_spmv_mdot with one vector, the
//                  vector being p itself) where it takes the operator, else MatMult and dot as two kernels
//   k_cg_pw        one lane: dpi, the sign tests, a = beta / dpi
//   k_cg_update    x += a p ; r += (-a) w ; the stage-1 partials of beta = z . r and, under Jacobi, of ||z||^2 or
//                  ||r||^2 (with PCNONE the norm is sqrt(beta): the oracle's norm2 is the square root of its dot)
//   k_cg_iter_end  stage 2 of those sums, dp, history, KSPConvergedDefault, beta, and the top of the next iteration
//                  (its, the beta tests, b = beta / betaold)
// Which of the two MatMult + dot forms an operator takes is asked once per solve (mspi_cg_best_route).  A third route,
// mspi_cg_march (msplit_runtime.hip; k_box_cg_march in msplit_kernels.hip, with the tile helpers it uses), folds the
// AYPX into the box march; it gives the same bits, measured slower, and runs only when mspi_ksp_cg_set_route asks.
// All scalars live in a device-resident mspi_cg_state; the host reads it once per cycle of 32 iterations.  Every
// kernel returns at once on st->stop.  The streaming kernels follow the DBR lane map (chunk of 4096, lane t takes
// base + j*512 + 2t, +1) with double2 accesses and non-temporal loads of what streams once; each element operation
// rounds once (no contraction), so x, r and p are PETSc's VecAXPY / VecAYPX element for element.
#include "msplit_ctx.hpp"
#include "msplit_kdev.hpp"

namespace msk {
namespace {

__device__ __forceinline__ bool bad(double v) { return isnan(v) || isinf(v); }
__device__ __forceinline__ double sgn(double v) { return v < 0.0 ? -1.0 : 1.0; }  // PetscSign

constexpr int kHalf = kIters / 2;  // slices loaded before the first store: 4 x up to 5 vectors in flight per lane

// z = dinv .* r (JAC) or r, in registers
template <bool JAC>
__device__ __forceinline__ double pc(double r, double d) {
  if constexpr (JAC) return r * d;
  else return r;
}

// One element of the update sweep: x and r advance, the sums take their terms in the lane's element order.
template <bool JAC, bool UNPRE>
__device__ __forceinline__ void upd(double& x, double p, double& r, double w, double d, double a, double na,
                                    double& s0, double& s1) {
  x = x + a * p;
  r = r + na * w;
  const double z = pc<JAC>(r, d);
  s0 = s0 + z * r;
  if constexpr (JAC) s1 = UNPRE ? s1 + r * r : s1 + z * z;
}

template <bool JAC, bool UNPRE, bool STORE>
__global__ __launch_bounds__(kT) void k_cg_update(double* __restrict__ x, const double* __restrict__ p,
                                                  double* __restrict__ r, const double* __restrict__ w,
                                                  const double* __restrict__ dinv, const mspi_cg_state* __restrict__ st,
                                                  int64_t n, double* __restrict__ partial, int64_t nchunks) {
  // STORE = false: the sums of r as it stands (the initial residual), nothing else read or written, no stop flag
  if (STORE && st->stop) return;
  __shared__ double red[2][4];
  const double a = STORE ? st->a : 0.0, na = STORE ? st->na : 0.0;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  double s0 = 0.0, s1 = 0.0;
  if ((c + 1) * kChunk <= n) {
#pragma unroll
    for (int h = 0; h < kIters; h += kHalf) {
      double2 xv[kHalf], pv[kHalf], rv[kHalf], wq[kHalf], dv[kHalf];
#pragma unroll
      for (int j = 0; j < kHalf; ++j) {
        const int64_t e = base + (h + j) * (2 * kT);
        rv[j] = ld_nt(reinterpret_cast<const double2*>(r + e));
        if constexpr (STORE) {
          xv[j] = ld_nt(reinterpret_cast<const double2*>(x + e));
          pv[j] = ld_nt(reinterpret_cast<const double2*>(p + e));
          wq[j] = ld_nt(reinterpret_cast<const double2*>(w + e));
        }
        if constexpr (JAC) dv[j] = ld_nt(reinterpret_cast<const double2*>(dinv + e));
      }
#pragma unroll
      for (int j = 0; j < kHalf; ++j) {
        const int64_t e = base + (h + j) * (2 * kT);
        if constexpr (STORE) {
          upd<JAC, UNPRE>(xv[j].x, pv[j].x, rv[j].x, wq[j].x, JAC ? dv[j].x : 0.0, a, na, s0, s1);
          upd<JAC, UNPRE>(xv[j].y, pv[j].y, rv[j].y, wq[j].y, JAC ? dv[j].y : 0.0, a, na, s0, s1);
          *reinterpret_cast<double2*>(x + e) = xv[j];
          *reinterpret_cast<double2*>(r + e) = rv[j];
        } else {
          const double z0 = pc<JAC>(rv[j].x, JAC ? dv[j].x : 0.0), z1 = pc<JAC>(rv[j].y, JAC ? dv[j].y : 0.0);
          s0 = s0 + z0 * rv[j].x;
          if constexpr (JAC) s1 = UNPRE ? s1 + rv[j].x * rv[j].x : s1 + z0 * z0;
          s0 = s0 + z1 * rv[j].y;
          if constexpr (JAC) s1 = UNPRE ? s1 + rv[j].y * rv[j].y : s1 + z1 * z1;
        }
      }
    }
  } else {  // the ragged last chunk: element by element, nothing at or beyond n read, summed or written
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const int64_t e = base + j * (2 * kT) + v;
        if (e >= n) continue;
        double rr = r[e];
        const double d = JAC ? dinv[e] : 0.0;
        if constexpr (STORE) {
          double xx = x[e];
          upd<JAC, UNPRE>(xx, p[e], rr, w[e], d, a, na, s0, s1);
          x[e] = xx;
          r[e] = rr;
        } else {
          const double z = pc<JAC>(rr, d);
          s0 = s0 + z * rr;
          if constexpr (JAC) s1 = UNPRE ? s1 + rr * rr : s1 + z * z;
        }
      }
    }
  }
  s0 = wave_butterfly(s0);
  if constexpr (JAC) s1 = wave_butterfly(s1);
  if (lane == 0) {
    red[0][wv] = s0;
    if constexpr (JAC) red[1][wv] = s1;
  }
  __syncthreads();
  if (t == 0) partial[c] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  if (JAC && t == 1) partial[nchunks + c] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
}

template <bool JAC>
__global__ __launch_bounds__(kT) void k_cg_aypx(const double* __restrict__ r, const double* __restrict__ dinv,
                                                double* __restrict__ p, const mspi_cg_state* __restrict__ st,
                                                int64_t n) {
  if (st->stop) return;
  const bool first = st->i == 0;  // VecCopy(Z, P): p_old is not read (it may hold anything)
  const double b = st->b;
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  if ((c + 1) * kChunk <= n) {
    double2 rv[kIters], dv[kIters], pv[kIters];
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      rv[j] = *reinterpret_cast<const double2*>(r + e);  // r is read again by the update sweep: a plain load
      if constexpr (JAC) dv[j] = ld_nt(reinterpret_cast<const double2*>(dinv + e));
      if (!first) pv[j] = ld_nt(reinterpret_cast<const double2*>(p + e));
    }
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      const double z0 = pc<JAC>(rv[j].x, JAC ? dv[j].x : 0.0), z1 = pc<JAC>(rv[j].y, JAC ? dv[j].y : 0.0);
      double2 o;
      o.x = first ? z0 : z0 + b * pv[j].x;
      o.y = first ? z1 : z1 + b * pv[j].y;
      *reinterpret_cast<double2*>(p + e) = o;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const int64_t e = base + j * (2 * kT) + v;
        if (e >= n) continue;
        const double z = pc<JAC>(r[e], JAC ? dinv[e] : 0.0);
        p[e] = first ? z : z + b * p[e];
      }
    }
  }
}

// ---------------------------------------------------------------- the scalar recurrence
// k_dot_stage2's order: lane t adds p[t], p[t+256], ..., wave butterfly, then (w0 + w1) + (w2 + w3)
__device__ inline double fold(const double* __restrict__ p, int64_t nchunks, double* red) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  double acc = 0.0;
  for (int64_t i = t; i < nchunks; i += kT) acc = acc + p[i];
  acc = wave_butterfly(acc);
  if (lane == 0) red[wv] = acc;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ inline void log_res(mspi_cg_state* st, double* hist, double r) {
  if (st->nhist < st->hist_cap) hist[st->nhist] = r;
  st->nhist++;
}

// KSPConvergedDefault (msplit_gmres.hip's statements on this state)
__device__ inline void converged(mspi_cg_state* st, int n, double rnorm) {
  st->reason = MSP_CONVERGED_ITERATING;
  if (n == 0) {
    if (!st->guess_zero && !st->uirnorm) {
      double snorm = st->bnorm;
      if (snorm == 0.0) snorm = rnorm;
      st->rnorm0 = snorm;
    } else {
      st->rnorm0 = rnorm;
    }
    const double t = st->rtol * st->rnorm0;
    st->ttol = t < st->abstol ? st->abstol : t;  // PetscMax
  }
  if (bad(rnorm)) st->reason = MSP_DIVERGED_NANORINF;
  else if (rnorm <= st->ttol) st->reason = (rnorm < st->abstol) ? MSP_CONVERGED_ATOL : MSP_CONVERGED_RTOL;
  else if (rnorm >= st->divtol * st->rnorm0) st->reason = MSP_DIVERGED_DTOL;
}

// The loop condition and the top of iteration st->i, up to VecAYPX's scalar.
__device__ inline void loop_top(mspi_cg_state* st) {
  if (!st->reason && !(st->i < st->max_it)) st->reason = MSP_DIVERGED_ITS;
  if (!st->reason) {
    st->its = st->i + 1;
    if (st->beta == 0.0) st->reason = MSP_CONVERGED_ATOL;
    else if (st->i > 0 && st->beta * st->betaold < 0.0) st->reason = MSP_DIVERGED_INDEFINITE_PC;
  }
  if (st->reason) {
    st->stop = 1;
    return;
  }
  st->b = st->i > 0 ? st->beta / st->betaold : 0.0;
}

// After the sums of a residual: START from the initial one (KSPConvergedDefault(0)), else the end of iteration i.
template <bool START>
__global__ __launch_bounds__(kT) void k_cg_iter_end(mspi_cg_state* st, double* __restrict__ hist,
                                                    const double* __restrict__ partial, int64_t nchunks) {
  __shared__ double red[2][4];
  const int jac = st->jacobi;
  const double s0 = fold(partial, nchunks, red[0]);
  const double s1 = jac ? fold(partial + nchunks, nchunks, red[1]) : s0;
  if (st->stop || threadIdx.x != 0) return;
  const double dp = sqrt(s1);
  st->dp = st->rnorm = dp;
  log_res(st, hist, dp);
  converged(st, START ? 0 : st->i + 1, dp);
  if (!st->reason) {
    st->beta = s0;
    if (bad(s0)) st->reason = MSP_DIVERGED_NANORINF;  // KSPCheckDot
  }
  if (!START && !st->reason) st->i = st->i + 1;
  loop_top(st);
}

__global__ void k_cg_pw(mspi_cg_state* st) {
  if (st->stop) return;
  const double dpiold = st->dpi, dpi = st->pw;
  st->dpiold = dpiold;
  st->dpi = dpi;
  st->betaold = st->beta;
  if (bad(dpi)) {  // KSPCheckDot
    st->reason = MSP_DIVERGED_NANORINF;
    st->stop = 1;
  } else if (dpi == 0.0 || (st->i > 0 && sgn(dpi) * sgn(dpiold) < 0.0)) {
    st->reason = MSP_DIVERGED_INDEFINITE_MAT;
    st->stop = 1;
  } else {
    st->a = st->beta / dpi;
    st->na = -st->a;
  }
}

template <bool STORE>
int launch_update(double* x, const double* p, double* r, const double* w, const double* dinv, int unpre,
                  const mspi_cg_state* st, int64_t n, double* partial, int64_t nch, hipStream_t s) {
  const int var = dinv ? (unpre ? 2 : 1) : 0;
  const bool ok = pick<0, 1, 2>(var, [&](auto v) {
    constexpr int V = decltype(v)::value;
    k_cg_update<V != 0, V == 2, STORE><<<dim3((unsigned)nch), dim3(kT), 0, s>>>(x, p, r, w, dinv, st, n, partial, nch);
  });
  return ok ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

}  // namespace
}  // namespace msk

// ===================================================================== launchers
using namespace msk;

static int cg_checks(msp_ctx* c, int64_t n) {
  ARGCHK(c->reduce == MSP_REDUCE_DBR, MSP_ERR_SUP, "KSPCG's kernels need the DBR reduction");
  ARGCHK(n >= 0 && nchunks_of(n) * 2 <= c->partial_cap, MSP_ERR_ARG_WRONG,
         "KSPCG step without mspi_reserve_partial for %lld rows", (long long)n);
  return MSP_SUCCESS;
}

extern "C" int mspi_cg_aypx(msp_ctx* c, const double* r, const double* dinv, double* p, int64_t n,
                            const mspi_cg_state* st) {
  const int64_t nch = nchunks_of(n);
  if (nch == 0) return MSP_SUCCESS;
  KTimer kt(c, MSP_KERNEL_MAXPY, 8.0 * (double)n * (dinv ? 4.0 : 3.0));
  if (dinv) k_cg_aypx<true><<<dim3((unsigned)nch), dim3(kT), 0, c->stream>>>(r, dinv, p, st, n);
  else k_cg_aypx<false><<<dim3((unsigned)nch), dim3(kT), 0, c->stream>>>(r, dinv, p, st, n);
  KCHK((int)hipGetLastError());
  return MSP_SUCCESS;
}

// MSPI_CG_ROUTE_MARCH is never picked: on the 256^3 Poisson box it measured 0.2895 ms per iteration against 0.2700
// for MSPI_CG_ROUTE_FUSED (profiles/cg/README.md) -- it saves one vector pass and recomputes p_new for three planes
// from two vectors each.  It is reached through mspi_ksp_cg_set_route only.
extern "C" int mspi_cg_best_route(const msp_mat* A) {
  return mspi_spmv_mdot_takes(A) ? MSPI_CG_ROUTE_FUSED : MSPI_CG_ROUTE_TWO;
}

extern "C" int mspi_cg_matmult_dot(msp_mat* A, const double* p, double* w, mspi_cg_state* st, int route) {
  msp_ctx* c = mspi_mat_ctx(A);
  int32_t nr, nc;
  mspi_mat_dims(A, &nr, &nc);
  // p * 1.0 is exact, so the scaled MatMult is MatMult; the dot's second factor is p itself
  if (route == MSPI_CG_ROUTE_FUSED) {
    const int rc = mspi_spmv_mdot(A, p, &st->one, w, 1, p, 0, &st->one, &st->pw, &st->stop);
    if (rc == MSP_ERR_SUP) mspi_set_error(MSP_ERR_SUP, "KSPCG's fused MatMult + dot on an operator that does not take it");
    return rc;
  }
  ARGCHK(route == MSPI_CG_ROUTE_TWO, MSP_ERR_ARG_OUTOFRANGE, "KSPCG MatMult + dot route %d", route);
  int rc = mspi_spmv_scaled(A, p, &st->one, nullptr, w, &st->stop);
  if (!rc) rc = mspi_mdot_basis(c, w, 1, p, 0, &st->one, nr, &st->pw, &st->stop);
  return rc;
}

extern "C" int mspi_cg_pw(msp_ctx* c, mspi_cg_state* st) {
  k_cg_pw<<<dim3(1), dim3(1), 0, c->stream>>>(st);
  KCHK((int)hipGetLastError());
  return MSP_SUCCESS;
}

extern "C" int mspi_cg_update(msp_ctx* c, double* x, const double* p, double* r, const double* w, const double* dinv,
                              int norm_unpre, int64_t n, const mspi_cg_state* st) {
  int rc = cg_checks(c, n);
  if (rc) return rc;
  const int64_t nch = nchunks_of(n);
  if (nch == 0) return MSP_SUCCESS;
  // x, p, r, w read, x and r written (and dinv)
  KTimer kt(c, MSP_KERNEL_MAXPY, 8.0 * (double)n * (dinv ? 7.0 : 6.0));
  KCHK(launch_update<true>(x, p, r, w, dinv, norm_unpre, st, n, c->partial, nch, c->stream));
  return MSP_SUCCESS;
}

extern "C" int mspi_cg_sums(msp_ctx* c, const double* r, const double* dinv, int norm_unpre, int64_t n) {
  int rc = cg_checks(c, n);
  if (rc) return rc;
  const int64_t nch = nchunks_of(n);
  if (nch == 0) return MSP_SUCCESS;
  KTimer kt(c, MSP_KERNEL_NORM, 8.0 * (double)n * (dinv ? 2.0 : 1.0));
  KCHK(launch_update<false>(nullptr, nullptr, const_cast<double*>(r), nullptr, dinv, norm_unpre, nullptr, n,
                            c->partial, nch, c->stream));
  return MSP_SUCCESS;
}

extern "C" int mspi_cg_start(msp_ctx* c, mspi_cg_state* st, double* hist, int64_t n) {
  k_cg_iter_end<true><<<dim3(1), dim3(kT), 0, c->stream>>>(st, hist, c->partial, nchunks_of(n));
  KCHK((int)hipGetLastError());
  return MSP_SUCCESS;
}

extern "C" int mspi_cg_iter_end(msp_ctx* c, mspi_cg_state* st, double* hist, int64_t n) {
  k_cg_iter_end<false><<<dim3(1), dim3(kT), 0, c->stream>>>(st, hist, c->partial, nchunks_of(n));
  KCHK((int)hipGetLastError());
  return MSP_SUCCESS;
}

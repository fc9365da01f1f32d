// msplit_pcj.hip -- left Jacobi preconditioning of GMRES (MSP_PC_JACOBI), fused into the CGS kernels, for gfx950.
//
// PETSc's PCJACOBI (-pc_jacobi_type diagonal) on the left with the preconditioned residual norm:
//   PCSetUp   dinv_i = 1 / a_ii (one f64 division); 1.0 where row i stores no diagonal entry or a_ii == +-0.0
//   PCApply   z_i = r_i * dinv_i (VecPointwiseMult: one f64 multiply, never a division, never contracted)
// The Arnoldi step is MatMult, MDot, MAXPY as three kernels over the f64 basis: the MatMult stores the raw
// W = A (sc[it] VV(it)) and both CGS kernels form w = W .* dinv in registers as they load W (one multiply per
// element, before any product), so the raw W is never rewritten and the preconditioner costs one more 8-byte
// read per row in each kernel.  Everything after that multiply is the f64 step's arithmetic, statement for
// statement (-ffp-contract=off, the DBR reduction order of msplit_kdev.hpp, PETSc's VecMAXPY grouping).
//
// Lane map (the DBR map, as msplit_cb.hip): workgroup c owns elements [4096c, 4096c + 4096), lane t owns
// base + j*512 + 2t, +1 for j = 0..7, one double2 (16 bytes) per load; sums are per-lane sequential, then the
// wave64 butterfly, then (w0 + w1) + (w2 + w3) into partial[v * nchunks + c].  Stage 2 is msk_dot_stage2 /
// mspi_gm_norm_update, unchanged.  A partial last chunk (and odd n) takes the guarded element-wise path; nothing is
// read or written at or beyond n.  No vector needs more than 16-byte alignment.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "msplit_kernels.h"

namespace {

constexpr int kT = 256;                  // threads per workgroup (4 wave64)
constexpr int kIters = 8;                // two-element slices per thread per DBR chunk
constexpr int kChunk = kT * 2 * kIters;  // 4096 elements per DBR chunk
static_assert(kChunk == MSK_DBR_CHUNK, "DBR chunk must match the oracle");
static_assert(MSK_CB_MAX_GROUP <= kT, "one lane per vector writes the chunk's partials");

typedef double dx2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool stopped(const int* stop) { return stop && *stop; }

// the basis streams through once per kernel and is far larger than the MALL: non-temporal, as the f64 kernels' loads
__device__ __forceinline__ dx2 ld_nt(const double* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const dx2*>(p));
}

__device__ __forceinline__ double wave_butterfly(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// (w0 + w1) + (w2 + w3) of one value per lane into out[0] (lane 0 of the workgroup)
__device__ __forceinline__ void block_fold(double v, double* red, double* out) {
  const int t = threadIdx.x;
  v = wave_butterfly(v);
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  if (t == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
}

// the lane's 16 values of r .* dinv at its DBR positions (0 at and beyond n): PCApply as the vector is loaded
__device__ __forceinline__ void load_scaled(const double* r, const double* __restrict__ dinv, int64_t base, int64_t n,
                                            bool full, double (&wr)[2 * kIters]) {
  if (full) {
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const double2 q = *reinterpret_cast<const double2*>(r + base + j * (2 * kT));
      const double2 d = *reinterpret_cast<const double2*>(dinv + base + j * (2 * kT));
      wr[2 * j] = q.x * d.x;
      wr[2 * j + 1] = q.y * d.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      wr[2 * j] = e < n ? r[e] * dinv[e] : 0.0;
      wr[2 * j + 1] = e + 1 < n ? r[e + 1] * dinv[e + 1] : 0.0;
    }
  }
}

// ---------------------------------------------------------------------- PCSetUp
// out_i = a_ii of a CSR matrix (the first entry of row i in column i; 0.0 where the row stores none), or with INV
// its Jacobi inverse: 1 / a_ii, and 1.0 where a_ii == +-0.0 or is absent ("zero detected in diagonal, using 1").
// One lane per row; runs once per set-up.
template <bool INV>
__global__ __launch_bounds__(kT) void k_pcj_diag(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                 const double* __restrict__ val, int32_t n,
                                                 double* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (r >= n) return;
  double a = 0.0;
  for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
    if (col[k] == r) {
      a = val[k];
      break;
    }
  }
  out[r] = INV ? (a == 0.0 ? 1.0 : 1.0 / a) : a;
}

// -------------------------------------------------------------- apply and norm
// z = r .* dinv, partial[c] = this chunk's DBR partial of sum z^2 (dot_chunk's SELF order).  r and z may be the
// same vector (each lane reads its own elements before it writes them).
__global__ __launch_bounds__(kT) void k_pcj_apply_norm(const double* r, const double* __restrict__ dinv, double* z,
                                                       int64_t n, double* __restrict__ partial,
                                                       const int* __restrict__ stop) {
  if (stopped(stop)) return;
  __shared__ double red[4];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  const bool full = (c + 1) * kChunk <= n;
  double wr[2 * kIters];
  load_scaled(r, dinv, base, n, full, wr);
  double acc = 0.0;
  if (full) {
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      *reinterpret_cast<double2*>(z + e) = make_double2(wr[2 * j], wr[2 * j + 1]);
      acc = acc + wr[2 * j] * wr[2 * j];
      acc = acc + wr[2 * j + 1] * wr[2 * j + 1];
    }
  } else {
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      if (e < n) {
        z[e] = wr[2 * j];
        acc = acc + wr[2 * j] * wr[2 * j];
      }
      if (e + 1 < n) {
        z[e + 1] = wr[2 * j + 1];
        acc = acc + wr[2 * j + 1] * wr[2 * j + 1];
      }
    }
  }
  block_fold(acc, red, partial + c);
}

// ----------------------------------------------------------------------- MDot
// G vectors of a full chunk at once: all G*8 loads are issued before the first product (dot_group_full's shape),
// then G independent accumulations in dot_chunk's order, acc += w * (v * sc).
template <int G>
__device__ __forceinline__ void pcj_dot_group(const double (&wr)[2 * kIters], const double* __restrict__ vb,
                                              int64_t stride, const double* __restrict__ scale, int g, int64_t base,
                                              double (*red)[4], int lane, int wv) {
  dx2 q[G][kIters];
  double sv[G];
#pragma unroll
  for (int u = 0; u < G; ++u) {
    const double* __restrict__ y = vb + (int64_t)(g + u) * stride;
    sv[u] = scale[g + u];
#pragma unroll
    for (int j = 0; j < kIters; ++j) q[u][j] = ld_nt(y + base + j * (2 * kT));
  }
  double acc[G];
#pragma unroll
  for (int u = 0; u < G; ++u) {
    acc[u] = 0.0;
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      acc[u] = acc[u] + wr[2 * j] * (q[u][j].x * sv[u]);
      acc[u] = acc[u] + wr[2 * j + 1] * (q[u][j].y * sv[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < G; ++u) {
    acc[u] = wave_butterfly(acc[u]);
    if (lane == 0) red[g + u][wv] = acc[u];
  }
}

// partial[v * nchunks + c] = chunk c of (W .* dinv) . (sc[v] VV(v)), v < nv <= MSK_CB_MAX_GROUP; w = W .* dinv is
// formed as W is loaded and stays in registers while the nv basis vectors stream past in groups of four.
__global__ __launch_bounds__(kT) void k_pcj_mdot(const double* __restrict__ w, const double* __restrict__ dinv,
                                                 const double* __restrict__ vb, int64_t stride,
                                                 const double* __restrict__ scale, int nv, int64_t n,
                                                 double* __restrict__ partial, int64_t nchunks,
                                                 const int* __restrict__ stop) {
  if (stopped(stop)) return;
  __shared__ double red[MSK_CB_MAX_GROUP][4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  const bool full = (c + 1) * kChunk <= n;
  double wr[2 * kIters];
  load_scaled(w, dinv, base, n, full, wr);
  if (full) {
    int g = 0;
#pragma unroll 1
    for (; g + 4 <= nv; g += 4) pcj_dot_group<4>(wr, vb, stride, scale, g, base, red, lane, wv);
    const int rem = nv - g;  // uniform
    if (rem == 3) pcj_dot_group<3>(wr, vb, stride, scale, g, base, red, lane, wv);
    else if (rem == 2) pcj_dot_group<2>(wr, vb, stride, scale, g, base, red, lane, wv);
    else if (rem == 1) pcj_dot_group<1>(wr, vb, stride, scale, g, base, red, lane, wv);
  } else {
#pragma unroll 1
    for (int v = 0; v < nv; ++v) {
      const double* __restrict__ y = vb + (int64_t)v * stride;
      const double sv = scale[v];
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < kIters; ++j) {
        const int64_t e = base + j * (2 * kT);
        if (e < n) acc = acc + wr[2 * j] * (y[e] * sv);
        if (e + 1 < n) acc = acc + wr[2 * j + 1] * (y[e + 1] * sv);
      }
      acc = wave_butterfly(acc);
      if (lane == 0) red[v][wv] = acc;
    }
  }
  __syncthreads();
  if (t < nv) partial[t * nchunks + c] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
}

// ---------------------------------------------------------------------- MAXPY
// One group of PETSc's VecMAXPY over the lane's 16 running values (chunk_group's arithmetic): G == 1 is
// PetscKernelAXPY (s = a*p; s += U), G > 1 adds a0*p0 + a1*p1 (+ a2*p2 (+ a3*p3)), evaluated left to right, to U.
template <int G, bool FULL>
__device__ __forceinline__ void pcj_axpy_group(double (&u)[2 * kIters], const double* __restrict__ vb, int64_t stride,
                                               const double* __restrict__ scale, const double* __restrict__ adev,
                                               int g, int64_t base, int64_t n) {
  double a[G], sv[G];
  const double* vp[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {  // wave-uniform
    a[q] = -adev[g + q];
    vp[q] = vb + (int64_t)(g + q) * stride;
    sv[q] = scale[g + q];
  }
#pragma unroll
  for (int j = 0; j < kIters; ++j) {
    const int64_t e = base + j * (2 * kT);
    double p0[G], p1[G];
#pragma unroll
    for (int q = 0; q < G; ++q) {
      if (FULL) {
        const dx2 v = ld_nt(vp[q] + e);
        p0[q] = v.x * sv[q];
        p1[q] = v.y * sv[q];
      } else {
        p0[q] = e < n ? vp[q][e] * sv[q] : 0.0;
        p1[q] = e + 1 < n ? vp[q][e + 1] * sv[q] : 0.0;
      }
    }
    if constexpr (G == 1) {
      u[2 * j] = a[0] * p0[0] + u[2 * j];
      u[2 * j + 1] = a[0] * p1[0] + u[2 * j + 1];
    } else {
      double s0 = a[0] * p0[0] + a[1] * p0[1], s1 = a[0] * p1[0] + a[1] * p1[1];
      if constexpr (G > 2) {
        s0 = s0 + a[2] * p0[2];
        s1 = s1 + a[2] * p1[2];
      }
      if constexpr (G > 3) {
        s0 = s0 + a[3] * p0[3];
        s1 = s1 + a[3] * p1[3];
      }
      u[2 * j] = u[2 * j] + s0;
      u[2 * j + 1] = u[2 * j + 1] + s1;
    }
  }
}

// u -= sum_j h_j (sc[j] VV(j)) in PETSc's order: the nv & 3 leading vectors, then groups of four
template <bool FULL>
__device__ __forceinline__ void pcj_maxpy_body(double (&u)[2 * kIters], const double* __restrict__ vb, int64_t stride,
                                               const double* __restrict__ scale, const double* __restrict__ adev,
                                               int nv, int64_t base, int64_t n) {
  const int jrem = nv & 3;
  if (jrem == 3) pcj_axpy_group<3, FULL>(u, vb, stride, scale, adev, 0, base, n);
  else if (jrem == 2) pcj_axpy_group<2, FULL>(u, vb, stride, scale, adev, 0, base, n);
  else if (jrem == 1) pcj_axpy_group<1, FULL>(u, vb, stride, scale, adev, 0, base, n);
#pragma unroll 1
  for (int g = jrem; g < nv; g += 4) pcj_axpy_group<4, FULL>(u, vb, stride, scale, adev, g, base, n);
}

// VV(it+1) = (W .* dinv) - sum_j h_j (sc[j] VV(j)) (coefficients adev, negated) stored to vout, which is none of
// the nv vectors read; partial[c] = the chunk's DBR partial of its sum of squares.  win stays as the MatMult wrote it.
__global__ __launch_bounds__(kT) void k_pcj_maxpy_norm(const double* __restrict__ win,
                                                       const double* __restrict__ dinv, double* vout,
                                                       const double* vb, int64_t stride,
                                                       const double* __restrict__ scale,
                                                       const double* __restrict__ adev, int nv, int64_t n,
                                                       double* __restrict__ partial, const int* __restrict__ stop) {
  if (stopped(stop)) return;
  __shared__ double red[4];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  const bool full = (c + 1) * kChunk <= n;
  double u[2 * kIters];
  load_scaled(win, dinv, base, n, full, u);
  double acc = 0.0;
  if (full) {
    pcj_maxpy_body<true>(u, vb, stride, scale, adev, nv, base, n);
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      dx2 o;
      o.x = u[2 * j];
      o.y = u[2 * j + 1];
      __builtin_nontemporal_store(o, reinterpret_cast<dx2*>(vout + e));
      acc = acc + o.x * o.x;
      acc = acc + o.y * o.y;
    }
  } else {
    pcj_maxpy_body<false>(u, vb, stride, scale, adev, nv, base, n);
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      if (e < n) {
        vout[e] = u[2 * j];
        acc = acc + u[2 * j] * u[2 * j];
      }
      if (e + 1 < n) {
        vout[e + 1] = u[2 * j + 1];
        acc = acc + u[2 * j + 1] * u[2 * j + 1];
      }
    }
  }
  block_fold(acc, red, partial + c);
}

inline int nchunks32(int64_t n) { return (int)((n + kChunk - 1) / kChunk); }

}  // namespace

extern "C" int msk_pcj_diag(const int32_t* rowptr, const int32_t* col, const double* val, int32_t n, double* out,
                            int invert, hipStream_t s) {
  if (n <= 0) return 0;
  const unsigned g = (unsigned)((n + kT - 1) / kT);
  if (invert) k_pcj_diag<true><<<dim3(g), dim3(kT), 0, s>>>(rowptr, col, val, n, out);
  else k_pcj_diag<false><<<dim3(g), dim3(kT), 0, s>>>(rowptr, col, val, n, out);
  return (int)hipGetLastError();
}

extern "C" int msk_pcj_apply_norm(const double* r, const double* dinv, double* z, int64_t n, double* partial,
                                  const int* stop, hipStream_t s) {
  k_pcj_apply_norm<<<dim3(nchunks32(n)), dim3(kT), 0, s>>>(r, dinv, z, n, partial, stop);
  return (int)hipGetLastError();
}

extern "C" int msk_pcj_mdot(const double* w, const double* dinv, const double* vb, int64_t stride,
                            const double* scale, int nv, int64_t n, double* partial, int64_t nchunks,
                            const int* stop, hipStream_t s) {
  if (nv < 1 || nv > MSK_CB_MAX_GROUP || nchunks != nchunks32(n)) return (int)hipErrorInvalidValue;
  k_pcj_mdot<<<dim3(nchunks32(n)), dim3(kT), 0, s>>>(w, dinv, vb, stride, scale, nv, n, partial, nchunks, stop);
  return (int)hipGetLastError();
}

extern "C" int msk_pcj_maxpy_norm(const double* win, const double* dinv, double* vout, const double* vb,
                                  int64_t stride, const double* scale, const double* adev, int nv, int64_t n,
                                  double* partial, const int* stop, hipStream_t s) {
  if (nv < 1) return (int)hipErrorInvalidValue;
  k_pcj_maxpy_norm<<<dim3(nchunks32(n)), dim3(kT), 0, s>>>(win, dinv, vout, vb, stride, scale, adev, nv, n, partial,
                                                           stop);
  return (int)hipGetLastError();
}

// msplit_cb.hip -- compressed-basis GMRES (MSP_BASIS_F32): the CGS kernels over a Krylov basis stored in HBM as
// float, for gfx950.
//
// The basis is the step's traffic, so storing it in four bytes per entry instead of eight is what
// moves an HBM-bound step.  Only the storage changes: every value is promoted to double as it is loaded and all
// arithmetic is the f64 path's, statement for statement (-ffp-contract=off, the DBR reduction order of
// msplit_kdev.hpp, PETSc's VecMAXPY grouping).  A vector is rounded once, when it is stored:
//   rnd(v) = (double)(float)v   -- round to nearest even, gradual underflow, overflow to +-inf
// (v_cvt_f32_f64 under the kernel's default mode: f32 denormals are kept on gfx950 code objects), and its norm is
// taken of the rounded values -- what is in memory is the vector.
//
// Lane map (all four kernels; the DBR map): workgroup c owns elements [4096c, 4096c + 4096), lane t owns
// base + j*512 + 2t, +1 for j = 0..7, one float2 (8 bytes) per load; sums are per-lane sequential, then the wave64
// butterfly, then (w0 + w1) + (w2 + w3) into partial[v * nchunks + c].  Stage 2 is msk_dot_stage2 /
// mspi_gm_norm_update, unchanged.  A partial last chunk (and odd n) takes the guarded element-wise path; nothing is
// read or written at or beyond n.  The basis stride is a multiple of 1024 floats (4 KiB), so every float2 is aligned.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "msplit_kernels.h"

namespace {

constexpr int kT = 256;                  // threads per workgroup (4 wave64)
constexpr int kIters = 8;                // two-element slices per thread per DBR chunk
constexpr int kChunk = kT * 2 * kIters;  // 4096 elements per DBR chunk
static_assert(kChunk == MSK_DBR_CHUNK, "DBR chunk must match the oracle");
static_assert(MSK_CB_MAX_GROUP <= kT, "one lane per vector writes the chunk's partials");

typedef float fx2 __attribute__((ext_vector_type(2)));
typedef double dx2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool stopped(const int* stop) { return stop && *stop; }

// the basis streams through once per kernel and is far larger than the MALL: non-temporal, as the f64 kernels' loads
__device__ __forceinline__ fx2 ld_nt(const float* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const fx2*>(p));
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

// the lane's 16 values of an f64 vector at its DBR positions (0 at and beyond n)
__device__ __forceinline__ void load_w(const double* __restrict__ w, int64_t base, int64_t n, bool full,
                                       double (&wr)[2 * kIters]) {
  if (full) {
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const double2 q = *reinterpret_cast<const double2*>(w + base + j * (2 * kT));
      wr[2 * j] = q.x;
      wr[2 * j + 1] = q.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      wr[2 * j] = e < n ? w[e] : 0.0;
      wr[2 * j + 1] = e + 1 < n ? w[e + 1] : 0.0;
    }
  }
}

// ------------------------------------------------------------ round and store
// cur = rnd(r) as f64 (the next MatMult's input), v0 = the same values as f32, partial[c] = this chunk's DBR partial
// of sum rnd(r)^2 (dot_chunk's SELF order).  r and cur may be the same vector (each lane reads its own elements
// before it writes them).
__global__ __launch_bounds__(kT) void k_cb_round_store(const double* r, double* cur, float* __restrict__ v0, int64_t n,
                                                       double* __restrict__ partial, const int* __restrict__ stop) {
  if (stopped(stop)) return;
  __shared__ double red[4];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  const bool full = (c + 1) * kChunk <= n;
  double wr[2 * kIters];
  load_w(r, base, n, full, wr);
  double acc = 0.0;
  if (full) {
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      fx2 f;
      f.x = (float)wr[2 * j];
      f.y = (float)wr[2 * j + 1];
      const double d0 = (double)f.x, d1 = (double)f.y;
      __builtin_nontemporal_store(f, reinterpret_cast<fx2*>(v0 + e));
      *reinterpret_cast<double2*>(cur + e) = make_double2(d0, d1);
      acc = acc + d0 * d0;
      acc = acc + d1 * d1;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      if (e < n) {
        const float f = (float)wr[2 * j];
        const double d = (double)f;
        v0[e] = f;
        cur[e] = d;
        acc = acc + d * d;
      }
      if (e + 1 < n) {
        const float f = (float)wr[2 * j + 1];
        const double d = (double)f;
        v0[e + 1] = f;
        cur[e + 1] = d;
        acc = acc + d * d;
      }
    }
  }
  block_fold(acc, red, partial + c);
}

// ----------------------------------------------------------------------- MDot
// G vectors of a full chunk at once: all G*8 loads are issued before the first product (dot_group_full's shape),
// then G independent accumulations in dot_chunk's order, acc += w * (v * sc).
template <int G>
__device__ __forceinline__ void cb_dot_group(const double (&wr)[2 * kIters], const float* __restrict__ vb,
                                             int64_t stride, const double* __restrict__ scale, int g, int64_t base,
                                             double (*red)[4], int lane, int wv) {
  fx2 q[G][kIters];
  double sv[G];
#pragma unroll
  for (int u = 0; u < G; ++u) {
    const float* __restrict__ y = vb + (int64_t)(g + u) * stride;
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
      acc[u] = acc[u] + wr[2 * j] * ((double)q[u][j].x * sv[u]);
      acc[u] = acc[u] + wr[2 * j + 1] * ((double)q[u][j].y * sv[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < G; ++u) {
    acc[u] = wave_butterfly(acc[u]);
    if (lane == 0) red[g + u][wv] = acc[u];
  }
}

// partial[v * nchunks + c] = chunk c of W . (sc[v] VV(v)), v < nv <= MSK_CB_MAX_GROUP; W is f64 and stays in
// registers while the nv f32 vectors stream past in groups of four.
__global__ __launch_bounds__(kT) void k_cb_mdot(const double* __restrict__ w, const float* __restrict__ vb,
                                                int64_t stride, const double* __restrict__ scale, int nv, int64_t n,
                                                double* __restrict__ partial, int64_t nchunks,
                                                const int* __restrict__ stop) {
  if (stopped(stop)) return;
  __shared__ double red[MSK_CB_MAX_GROUP][4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  const bool full = (c + 1) * kChunk <= n;
  double wr[2 * kIters];
  load_w(w, base, n, full, wr);
  if (full) {
    int g = 0;
#pragma unroll 1
    for (; g + 4 <= nv; g += 4) cb_dot_group<4>(wr, vb, stride, scale, g, base, red, lane, wv);
    const int rem = nv - g;  // uniform
    if (rem == 3) cb_dot_group<3>(wr, vb, stride, scale, g, base, red, lane, wv);
    else if (rem == 2) cb_dot_group<2>(wr, vb, stride, scale, g, base, red, lane, wv);
    else if (rem == 1) cb_dot_group<1>(wr, vb, stride, scale, g, base, red, lane, wv);
  } else {
#pragma unroll 1
    for (int v = 0; v < nv; ++v) {
      const float* __restrict__ y = vb + (int64_t)v * stride;
      const double sv = scale[v];
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < kIters; ++j) {
        const int64_t e = base + j * (2 * kT);
        if (e < n) acc = acc + wr[2 * j] * ((double)y[e] * sv);
        if (e + 1 < n) acc = acc + wr[2 * j + 1] * ((double)y[e + 1] * sv);
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
__device__ __forceinline__ void cb_axpy_group(double (&u)[2 * kIters], const float* __restrict__ vb, int64_t stride,
                                              const double* __restrict__ scale, const double* __restrict__ adev,
                                              int negate, int g, int64_t base, int64_t n) {
  double a[G], sv[G];
  const float* vp[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {  // wave-uniform
    const double aq = adev[g + q];
    a[q] = negate ? -aq : aq;
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
        const fx2 v = ld_nt(vp[q] + e);
        p0[q] = (double)v.x * sv[q];
        p1[q] = (double)v.y * sv[q];
      } else {
        p0[q] = e < n ? (double)vp[q][e] * sv[q] : 0.0;
        p1[q] = e + 1 < n ? (double)vp[q][e + 1] * sv[q] : 0.0;
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

// u += sum_j a_j (sc[j] VV(j)) in PETSc's order: the nv & 3 leading vectors, then groups of four
template <bool FULL>
__device__ __forceinline__ void cb_maxpy_body(double (&u)[2 * kIters], const float* __restrict__ vb, int64_t stride,
                                              const double* __restrict__ scale, const double* __restrict__ adev,
                                              int negate, int nv, int64_t base, int64_t n) {
  const int jrem = nv & 3;
  if (jrem == 3) cb_axpy_group<3, FULL>(u, vb, stride, scale, adev, negate, 0, base, n);
  else if (jrem == 2) cb_axpy_group<2, FULL>(u, vb, stride, scale, adev, negate, 0, base, n);
  else if (jrem == 1) cb_axpy_group<1, FULL>(u, vb, stride, scale, adev, negate, 0, base, n);
  // one group of four per iteration: 32 float2 loads in flight per lane at 198 VGPRs (two workgroups per CU);
  // two groups per iteration take 298 VGPRs, one workgroup per CU
#pragma unroll 1
  for (int g = jrem; g < nv; g += 4) cb_axpy_group<4, FULL>(u, vb, stride, scale, adev, negate, g, base, n);
}

// w' = W - sum_j h_j (sc[j] VV(j)) (coefficients adev, negated), s = rnd(w') stored twice: as f32 to vout (the new
// basis vector) and as f64 to cur (the next MatMult's input); partial[c] = the chunk's DBR partial of sum s^2.
__global__ __launch_bounds__(kT) void k_cb_maxpy_norm(const double* __restrict__ win, double* __restrict__ cur,
                                                      float* vout, const float* vb, int64_t stride,
                                                      const double* __restrict__ scale,
                                                      const double* __restrict__ adev, int nv, int64_t n,
                                                      double* __restrict__ partial, const int* __restrict__ stop) {
  if (stopped(stop)) return;
  __shared__ double red[4];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  const bool full = (c + 1) * kChunk <= n;
  double u[2 * kIters];
  load_w(win, base, n, full, u);
  double acc = 0.0;
  if (full) {
    cb_maxpy_body<true>(u, vb, stride, scale, adev, 1, nv, base, n);
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      fx2 f;
      f.x = (float)u[2 * j];
      f.y = (float)u[2 * j + 1];
      const double d0 = (double)f.x, d1 = (double)f.y;
      __builtin_nontemporal_store(f, reinterpret_cast<fx2*>(vout + e));
      *reinterpret_cast<double2*>(cur + e) = make_double2(d0, d1);
      acc = acc + d0 * d0;
      acc = acc + d1 * d1;
    }
  } else {
    cb_maxpy_body<false>(u, vb, stride, scale, adev, 1, nv, base, n);
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      if (e < n) {
        const float f = (float)u[2 * j];
        const double d = (double)f;
        vout[e] = f;
        cur[e] = d;
        acc = acc + d * d;
      }
      if (e + 1 < n) {
        const float f = (float)u[2 * j + 1];
        const double d = (double)f;
        vout[e + 1] = f;
        cur[e + 1] = d;
        acc = acc + d * d;
      }
    }
  }
  block_fold(acc, red, partial + c);
}

// BuildSoln: x = x + (0 + sum_j nrs_j (sc[j] VV(j))), the vector count read from the device (*nvdev; 0: nothing)
__global__ __launch_bounds__(kT) void k_cb_accum(double* __restrict__ x, const int* __restrict__ nvdev,
                                                 const float* __restrict__ vb, int64_t stride,
                                                 const double* __restrict__ scale, const double* __restrict__ coef,
                                                 int64_t n, const int* __restrict__ stop) {
  if (stopped(stop)) return;
  const int nv = *nvdev;
  if (nv <= 0) return;
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  double u[2 * kIters];
#pragma unroll
  for (int j = 0; j < 2 * kIters; ++j) u[j] = 0.0;
  if ((c + 1) * kChunk <= n) {
    cb_maxpy_body<true>(u, vb, stride, scale, coef, 0, nv, base, n);
#pragma unroll
    for (int j = 0; j < kIters; ++j) {  // VecAXPY(x, 1.0, T): x + T
      const int64_t e = base + j * (2 * kT);
      const double2 q = *reinterpret_cast<const double2*>(x + e);
      *reinterpret_cast<double2*>(x + e) = make_double2(q.x + u[2 * j], q.y + u[2 * j + 1]);
    }
  } else {
    cb_maxpy_body<false>(u, vb, stride, scale, coef, 0, nv, base, n);
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      if (e < n) x[e] = x[e] + u[2 * j];
      if (e + 1 < n) x[e + 1] = x[e + 1] + u[2 * j + 1];
    }
  }
}

inline int nchunks32(int64_t n) { return (int)((n + kChunk - 1) / kChunk); }

}  // namespace

extern "C" int msk_cb_round_store(const double* r, double* cur, float* v0, int64_t n, double* partial, const int* stop,
                                  hipStream_t s) {
  k_cb_round_store<<<dim3(nchunks32(n)), dim3(kT), 0, s>>>(r, cur, v0, n, partial, stop);
  return (int)hipGetLastError();
}

extern "C" int msk_cb_mdot(const double* w, const float* vb, int64_t stride, const double* scale, int nv, int64_t n,
                           double* partial, int64_t nchunks, const int* stop, hipStream_t s) {
  if (nv < 1 || nv > MSK_CB_MAX_GROUP) return (int)hipErrorInvalidValue;
  k_cb_mdot<<<dim3(nchunks32(n)), dim3(kT), 0, s>>>(w, vb, stride, scale, nv, n, partial, nchunks, stop);
  return (int)hipGetLastError();
}

extern "C" int msk_cb_maxpy_norm(const double* win, double* cur, float* vout, const float* vb, int64_t stride,
                                 const double* scale, const double* adev, int nv, int64_t n, double* partial,
                                 const int* stop, hipStream_t s) {
  k_cb_maxpy_norm<<<dim3(nchunks32(n)), dim3(kT), 0, s>>>(win, cur, vout, vb, stride, scale, adev, nv, n, partial,
                                                          stop);
  return (int)hipGetLastError();
}

extern "C" int msk_cb_accum(double* x, const int* nvdev, const float* vb, int64_t stride, const double* scale,
                            const double* coef, int64_t n, const int* stop, hipStream_t s) {
  k_cb_accum<<<dim3(nchunks32(n)), dim3(kT), 0, s>>>(x, nvdev, vb, stride, scale, coef, n, stop);
  return (int)hipGetLastError();
}

// msplit_cb16.hip -- block-scaled GMRES basis (MSP_BASIS_B16): the CGS kernels over a Krylov basis stored in HBM as
// 16-bit integers with one power-of-two exponent per DBR chunk and vector, for gfx950.
//
// The four kernels are msplit_cb.hip's, statement for statement in their f64 arithmetic (-ffp-contract=off, the DBR
// lane map and order of msplit_kdev.hpp, PETSc's VecMAXPY grouping, (value * sc[j]) as its own multiply); only the
// rounding applied where a vector is stored, and the format it is read back from, differ.  Per chunk c of a vector
// (elements [4096c, min(4096(c+1), n))):
//   any element NaN or +-inf   every element reads back NaN; the stored exponent is kNonFinite
//   M = max |v_i| == 0         every element reads back +0.0
//   otherwise                  M = m 2^E, 0.5 <= m < 1 (frexp; subnormal M included, E >= -1073),
//                              q_i = clamp(rint(ldexp(v_i, 15 - E)), -32767, 32767)   (rint: ties to even),
//                              s_i = ldexp(q_i, E - 15)                               (IEEE ldexp, v_ldexp_f64)
// The workgroup that stores a vector holds the whole chunk in registers, so M costs one more workgroup reduction
// (one barrier) and no pass.  M and the non-finite test are one reduction: the maximum of the |v_i| bit patterns as
// unsigned integers orders finite doubles as fmax does and puts inf and every NaN above them (fmax would drop NaN).
// The norm is taken of the values read back -- what is in memory is the vector.
//
// Lane map: the DBR map for which elements a lane owns and in which order it sums them (lane t of workgroup c owns
// 4096c + j*512 + 2t, +1 for j = 0..7).  Layout inside a full chunk: two lane-contiguous halves -- the element at
// (lane t, slice j, half k) is int16 4096c + 2048 (j / 4) + 8t + 2 (j % 4) + k, so a lane fetches its 16 values with
// two 16-byte non-temporal loads, each of them fully coalesced (a wave covers 1 KiB contiguous per load, the
// workgroup 4 KiB).  Keeping a lane's 32 bytes contiguous instead (16t + 2j + k: every load touches half of each
// 128-byte line) measured 4.85 against 5.95 TB/s in the MAXPY, 256^3.  A partial last chunk (and odd n) is stored in
// natural order, element e at int16 e -- the permutation of a full chunk would scatter it beyond n -- and takes the
// guarded element-wise path: nothing is read or written at or beyond n, so the pad [n, stride) stays untouched with
// a stride of n rounded up to 2048 int16 (4 KiB).  The layout is private to this file: nothing else reads a block16
// basis.  Exponents: eb[v * nchunks + c], int32.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "msplit_kernels.h"

namespace {

constexpr int kT = 256;                  // threads per workgroup (4 wave64)
constexpr int kIters = 8;                // two-element slices per thread per DBR chunk
constexpr int kChunk = kT * 2 * kIters;  // 4096 elements per DBR chunk
static_assert(kChunk == MSK_DBR_CHUNK, "DBR chunk must match the oracle");
static_assert(MSK_CB_MAX_GROUP <= kT, "one lane per vector writes the chunk's partials");

constexpr int32_t kNonFinite = INT32_MIN;  // the exponent of a chunk that held a NaN or an inf
constexpr unsigned long long kAbsMask = 0x7fffffffffffffffull, kInfBits = 0x7ff0000000000000ull;

typedef int ix4 __attribute__((ext_vector_type(4)));

// a lane's 16 values of a full chunk: dword j holds (slice j, half 0) in its low and (slice j, half 1) in its high
// 16 bits; a = slices 0..3 (the chunk's first 4 KiB), b = slices 4..7 (its second)
struct Q16 {
  ix4 a, b;
};

__device__ __forceinline__ bool stopped(const int* stop) { return stop && *stop; }

// the basis streams through once per kernel and is far larger than the MALL: non-temporal
__device__ __forceinline__ Q16 ld16(const int16_t* p) {
  Q16 q;
  q.a = __builtin_nontemporal_load(reinterpret_cast<const ix4*>(p));
  q.b = __builtin_nontemporal_load(reinterpret_cast<const ix4*>(p + kChunk / 2));
  return q;
}
__device__ __forceinline__ int dword(const Q16& q, int j) { return j < 4 ? q.a[j & 3] : q.b[j & 3]; }
__device__ __forceinline__ int half0(int d) { return (int)(int16_t)(d & 0xffff); }
__device__ __forceinline__ int half1(int d) { return d >> 16; }

// how a reader sees one vector's chunk: value = ldexp(q, k) * sv, sv = NaN for a non-finite chunk (wave-uniform)
struct Deq {
  int k;
  double sv;
};
__device__ __forceinline__ Deq deq_of(int32_t e, double scale) {
  Deq d;
  d.k = e == kNonFinite ? 0 : e - 15;
  d.sv = e == kNonFinite ? __builtin_nan("") : scale;
  return d;
}
__device__ __forceinline__ double scaled(int q, const Deq& d) { return ldexp((double)q, d.k) * d.sv; }

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

// ------------------------------------------------------------------ quantiser
// The chunk's exponent from the 16 values of every lane (0 at and beyond n): E of M = m 2^E, 0 for a zero chunk,
// kNonFinite if any value is NaN or inf.  The maximum is order-free, so the butterfly and the four values through
// LDS are exact.  One barrier; the result is workgroup-uniform.
__device__ __forceinline__ int32_t chunk_exponent(const double (&u)[2 * kIters], unsigned long long* mred) {
  const int t = threadIdx.x;
  unsigned long long mb = 0;
#pragma unroll
  for (int i = 0; i < 2 * kIters; ++i) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(u[i]) & kAbsMask;
    mb = b > mb ? b : mb;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(mb, off, 64);
    mb = o > mb ? o : mb;
  }
  if ((t & 63) == 0) mred[t >> 6] = mb;
  __syncthreads();
  const unsigned long long m01 = mred[0] > mred[1] ? mred[0] : mred[1], m23 = mred[2] > mred[3] ? mred[2] : mred[3];
  mb = m01 > m23 ? m01 : m23;
  if (mb >= kInfBits) return kNonFinite;
  if (mb == 0) return 0;
  const int be = (int)(mb >> 52);  // frexp's exponent: biased - 1022, or counted from the top bit of a subnormal
  return be ? be - 1022 : -1074 + (64 - __clzll((long long)mb));
}

// q of one value and the value it reads back as (E finite: |ldexp(v, 15 - E)| < 2^15, the clamp is reachable)
__device__ __forceinline__ int quantise(double v, int32_t E, double* back) {
  if (E == kNonFinite) {  // workgroup-uniform
    *back = __builtin_nan("");
    return 0;
  }
  int q = (int)rint(ldexp(v, 15 - E));
  q = q > 32767 ? 32767 : (q < -32767 ? -32767 : q);
  *back = ldexp((double)q, E - 15);
  return q;
}

// s = rnd16(u) of the lane's 16 values: the int16 to vout (the two-halves layout in a full chunk, natural order in a
// partial one), the values read back to cur (f64, DBR positions), the chunk's exponent to eout[c]; returns the
// lane's part of sum s^2 in dot_chunk's SELF order.
__device__ __forceinline__ double store_chunk(const double (&u)[2 * kIters], double* cur, int16_t* vout,
                                              int32_t* eout, int64_t c, int64_t base, int64_t n, bool full,
                                              unsigned long long* mred) {
  const int t = threadIdx.x;
  const int32_t E = chunk_exponent(u, mred);
  if (t == 0) eout[c] = E;
  double acc = 0.0;
  if (full) {
    int dw[kIters];
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      double d0, d1;
      const int q0 = quantise(u[2 * j], E, &d0), q1 = quantise(u[2 * j + 1], E, &d1);
      dw[j] = (q0 & 0xffff) | (int)((unsigned)q1 << 16);
      *reinterpret_cast<double2*>(cur + e) = make_double2(d0, d1);
      acc = acc + d0 * d0;
      acc = acc + d1 * d1;
    }
    ix4 a, b;
    a.x = dw[0], a.y = dw[1], a.z = dw[2], a.w = dw[3];
    b.x = dw[4], b.y = dw[5], b.z = dw[6], b.w = dw[7];
    ix4* p = reinterpret_cast<ix4*>(vout + c * kChunk + 8 * t);
    __builtin_nontemporal_store(a, p);
    __builtin_nontemporal_store(b, reinterpret_cast<ix4*>(vout + c * kChunk + kChunk / 2 + 8 * t));
  } else {
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t e = base + j * (2 * kT);
      if (e < n) {
        double d;
        vout[e] = (int16_t)quantise(u[2 * j], E, &d);
        cur[e] = d;
        acc = acc + d * d;
      }
      if (e + 1 < n) {
        double d;
        vout[e + 1] = (int16_t)quantise(u[2 * j + 1], E, &d);
        cur[e + 1] = d;
        acc = acc + d * d;
      }
    }
  }
  return acc;
}

// ------------------------------------------------------------ round and store
// cur = rnd16(r) as f64 (the next MatMult's input), v0 / e0 = the same values as block16, partial[c] = this chunk's
// DBR partial of sum rnd16(r)^2.  r and cur may be the same vector (each lane reads its own elements before it
// writes them).
__global__ __launch_bounds__(kT) void k_cb16_round_store(const double* r, double* cur, int16_t* __restrict__ v0,
                                                         int32_t* __restrict__ e0, int64_t n,
                                                         double* __restrict__ partial, const int* __restrict__ stop) {
  if (stopped(stop)) return;
  __shared__ double red[4];
  __shared__ unsigned long long mred[4];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  const bool full = (c + 1) * kChunk <= n;
  double wr[2 * kIters];
  load_w(r, base, n, full, wr);
  const double acc = store_chunk(wr, cur, v0, e0, c, base, n, full, mred);
  block_fold(acc, red, partial + c);
}

// ----------------------------------------------------------------------- MDot
// G vectors of a full chunk at once: all 2G loads are issued before the first product (cb_dot_group's shape), then G
// independent accumulations in dot_chunk's order, acc += w * (v * sc).
template <int G>
__device__ __forceinline__ void cb16_dot_group(const double (&wr)[2 * kIters], const int16_t* __restrict__ vb,
                                               int64_t stride, const int32_t* __restrict__ eb, int64_t nchunks,
                                               const double* __restrict__ scale, int g, int64_t c, int t,
                                               double (*red)[4]) {
  Q16 q[G];
  Deq dq[G];
#pragma unroll
  for (int u = 0; u < G; ++u) {
    q[u] = ld16(vb + (int64_t)(g + u) * stride + c * kChunk + 8 * t);
    dq[u] = deq_of(eb[(int64_t)(g + u) * nchunks + c], scale[g + u]);
  }
  double acc[G];
#pragma unroll
  for (int u = 0; u < G; ++u) {
    acc[u] = 0.0;
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int d = dword(q[u], j);
      acc[u] = acc[u] + wr[2 * j] * scaled(half0(d), dq[u]);
      acc[u] = acc[u] + wr[2 * j + 1] * scaled(half1(d), dq[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < G; ++u) {
    acc[u] = wave_butterfly(acc[u]);
    if ((t & 63) == 0) red[g + u][t >> 6] = acc[u];
  }
}

// partial[v * nchunks + c] = chunk c of W . (sc[v] VV(v)), v < nv <= MSK_CB_MAX_GROUP; W is f64 and stays in
// registers while the nv block16 vectors stream past in groups of MSK_CB16_DOT_GROUP.
__global__ __launch_bounds__(kT) void k_cb16_mdot(const double* __restrict__ w, const int16_t* __restrict__ vb,
                                                  int64_t stride, const int32_t* __restrict__ eb,
                                                  const double* __restrict__ scale, int nv, int64_t n,
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
    for (; g + 8 <= nv; g += 8) cb16_dot_group<8>(wr, vb, stride, eb, nchunks, scale, g, c, t, red);
    if (g + 4 <= nv) {
      cb16_dot_group<4>(wr, vb, stride, eb, nchunks, scale, g, c, t, red);
      g += 4;
    }
    const int rem = nv - g;  // uniform
    if (rem == 3) cb16_dot_group<3>(wr, vb, stride, eb, nchunks, scale, g, c, t, red);
    else if (rem == 2) cb16_dot_group<2>(wr, vb, stride, eb, nchunks, scale, g, c, t, red);
    else if (rem == 1) cb16_dot_group<1>(wr, vb, stride, eb, nchunks, scale, g, c, t, red);
  } else {
#pragma unroll 1
    for (int v = 0; v < nv; ++v) {
      const int16_t* __restrict__ y = vb + (int64_t)v * stride;
      const Deq dq = deq_of(eb[(int64_t)v * nchunks + c], scale[v]);
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < kIters; ++j) {
        const int64_t e = base + j * (2 * kT);
        if (e < n) acc = acc + wr[2 * j] * scaled(y[e], dq);
        if (e + 1 < n) acc = acc + wr[2 * j + 1] * scaled(y[e + 1], dq);
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
// The group's 2G loads (full chunk) are issued before the first product.
template <int G, bool FULL>
__device__ __forceinline__ void cb16_axpy_group(double (&u)[2 * kIters], const int16_t* vb, int64_t stride,
                                                const int32_t* eb, int64_t nchunks,
                                                const double* __restrict__ scale, const double* __restrict__ adev,
                                                int negate, int g, int64_t c, int64_t base, int64_t n) {
  const int t = threadIdx.x;
  double a[G];
  Deq dq[G];
  Q16 qv[G];
  const int16_t* vp[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {  // wave-uniform but for the loads
    const double aq = adev[g + q];
    a[q] = negate ? -aq : aq;
    vp[q] = vb + (int64_t)(g + q) * stride;
    dq[q] = deq_of(eb[(int64_t)(g + q) * nchunks + c], scale[g + q]);
    if (FULL) qv[q] = ld16(vp[q] + c * kChunk + 8 * t);
  }
#pragma unroll
  for (int j = 0; j < kIters; ++j) {
    const int64_t e = base + j * (2 * kT);
    double p0[G], p1[G];
#pragma unroll
    for (int q = 0; q < G; ++q) {
      if (FULL) {
        const int d = dword(qv[q], j);
        p0[q] = scaled(half0(d), dq[q]);
        p1[q] = scaled(half1(d), dq[q]);
      } else {
        p0[q] = e < n ? scaled(vp[q][e], dq[q]) : 0.0;
        p1[q] = e + 1 < n ? scaled(vp[q][e + 1], dq[q]) : 0.0;
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
__device__ __forceinline__ void cb16_maxpy_body(double (&u)[2 * kIters], const int16_t* vb, int64_t stride,
                                                const int32_t* eb, int64_t nchunks,
                                                const double* __restrict__ scale, const double* __restrict__ adev,
                                                int negate, int nv, int64_t c, int64_t base, int64_t n) {
  const int jrem = nv & 3;
  if (jrem == 3) cb16_axpy_group<3, FULL>(u, vb, stride, eb, nchunks, scale, adev, negate, 0, c, base, n);
  else if (jrem == 2) cb16_axpy_group<2, FULL>(u, vb, stride, eb, nchunks, scale, adev, negate, 0, c, base, n);
  else if (jrem == 1) cb16_axpy_group<1, FULL>(u, vb, stride, eb, nchunks, scale, adev, negate, 0, c, base, n);
#pragma unroll 1
  for (int g = jrem; g < nv; g += 4)
    cb16_axpy_group<4, FULL>(u, vb, stride, eb, nchunks, scale, adev, negate, g, c, base, n);
}

// w' = W - sum_j h_j (sc[j] VV(j)) (coefficients adev, negated), s = rnd16(w') stored twice: as block16 to vout /
// eout (the new basis vector) and as f64 to cur (the next MatMult's input); partial[c] = the chunk's DBR partial of
// sum s^2.  vout is another vector of the basis vb and eout another row of eb: no restrict on those.
__global__ __launch_bounds__(kT) void k_cb16_maxpy_norm(const double* __restrict__ win, double* __restrict__ cur,
                                                        int16_t* vout, int32_t* eout, const int16_t* vb,
                                                        int64_t stride, const int32_t* eb, int64_t nchunks,
                                                        const double* __restrict__ scale,
                                                        const double* __restrict__ adev, int nv, int64_t n,
                                                        double* __restrict__ partial, const int* __restrict__ stop) {
  if (stopped(stop)) return;
  __shared__ double red[4];
  __shared__ unsigned long long mred[4];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  const bool full = (c + 1) * kChunk <= n;
  double u[2 * kIters];
  load_w(win, base, n, full, u);
  if (full) cb16_maxpy_body<true>(u, vb, stride, eb, nchunks, scale, adev, 1, nv, c, base, n);
  else cb16_maxpy_body<false>(u, vb, stride, eb, nchunks, scale, adev, 1, nv, c, base, n);
  const double acc = store_chunk(u, cur, vout, eout, c, base, n, full, mred);
  block_fold(acc, red, partial + c);
}

// BuildSoln: x = x + (0 + sum_j nrs_j (sc[j] VV(j))), the vector count read from the device (*nvdev; 0: nothing)
__global__ __launch_bounds__(kT) void k_cb16_accum(double* __restrict__ x, const int* __restrict__ nvdev,
                                                   const int16_t* __restrict__ vb, int64_t stride,
                                                   const int32_t* __restrict__ eb, int64_t nchunks,
                                                   const double* __restrict__ scale,
                                                   const double* __restrict__ coef, int64_t n,
                                                   const int* __restrict__ stop) {
  if (stopped(stop)) return;
  const int nv = *nvdev;
  if (nv <= 0) return;
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x, base = c * kChunk + 2 * t;
  double u[2 * kIters];
#pragma unroll
  for (int j = 0; j < 2 * kIters; ++j) u[j] = 0.0;
  if ((c + 1) * kChunk <= n) {
    cb16_maxpy_body<true>(u, vb, stride, eb, nchunks, scale, coef, 0, nv, c, base, n);
#pragma unroll
    for (int j = 0; j < kIters; ++j) {  // VecAXPY(x, 1.0, T): x + T
      const int64_t e = base + j * (2 * kT);
      const double2 q = *reinterpret_cast<const double2*>(x + e);
      *reinterpret_cast<double2*>(x + e) = make_double2(q.x + u[2 * j], q.y + u[2 * j + 1]);
    }
  } else {
    cb16_maxpy_body<false>(u, vb, stride, eb, nchunks, scale, coef, 0, nv, c, base, n);
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

extern "C" int msk_cb16_round_store(const double* r, double* cur, int16_t* v0, int32_t* e0, int64_t n,
                                    double* partial, const int* stop, hipStream_t s) {
  k_cb16_round_store<<<dim3(nchunks32(n)), dim3(kT), 0, s>>>(r, cur, v0, e0, n, partial, stop);
  return (int)hipGetLastError();
}

extern "C" int msk_cb16_mdot(const double* w, const int16_t* vb, int64_t stride, const int32_t* eb,
                             const double* scale, int nv, int64_t n, double* partial, int64_t nchunks,
                             const int* stop, hipStream_t s) {
  if (nv < 1 || nv > MSK_CB_MAX_GROUP || nchunks != nchunks32(n)) return (int)hipErrorInvalidValue;
  k_cb16_mdot<<<dim3(nchunks32(n)), dim3(kT), 0, s>>>(w, vb, stride, eb, scale, nv, n, partial, nchunks, stop);
  return (int)hipGetLastError();
}

extern "C" int msk_cb16_maxpy_norm(const double* win, double* cur, int16_t* vout, int32_t* eout, const int16_t* vb,
                                   int64_t stride, const int32_t* eb, const double* scale, const double* adev,
                                   int nv, int64_t n, double* partial, const int* stop, hipStream_t s) {
  k_cb16_maxpy_norm<<<dim3(nchunks32(n)), dim3(kT), 0, s>>>(win, cur, vout, eout, vb, stride, eb, nchunks32(n),
                                                            scale, adev, nv, n, partial, stop);
  return (int)hipGetLastError();
}

extern "C" int msk_cb16_accum(double* x, const int* nvdev, const int16_t* vb, int64_t stride, const int32_t* eb,
                              const double* scale, const double* coef, int64_t n, const int* stop, hipStream_t s) {
  k_cb16_accum<<<dim3(nchunks32(n)), dim3(kT), 0, s>>>(x, nvdev, vb, stride, eb, nchunks32(n), scale, coef, n,
                                                       stop);
  return (int)hipGetLastError();
}
